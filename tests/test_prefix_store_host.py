"""Host side of the engine's snapshot store, without a device: what a call
decides from the store's state before it touches the pool -- carry over, start the store empty (and
why), or do without it because another call holds it (fac_diag_rc_store_decide: the try-lock and
rc_store_decide as launch_pass takes them)."""
import numpy as np

from fuzzy_aho_corasick import _native

KEEP, FRESH, SIGNATURE, POOL, DIRECTORY, BUSY = range(6)
SIG = np.arange(1, 17, dtype=np.uint32)
NO_LIMIT = 2 ** 64 - 1


def decide(valid=1, calls=3, used=1000, cap=10_000, last_call=100, pending=KEEP, have=SIG, want=SIG, want_cap=10_000,
           cap_limit=NO_LIMIT, slots=None, keys=None, busy=0, sleep=0):
    slots = np.zeros(9, dtype=np.uint64) if slots is None else np.asarray(slots, dtype=np.uint64)
    keys = np.zeros(9, dtype=np.uint64) if keys is None else np.asarray(keys, dtype=np.uint64)
    have, want = np.ascontiguousarray(have, dtype=np.uint32), np.ascontiguousarray(want, dtype=np.uint32)
    return _native.lib.fac_diag_rc_store_decide(valid, calls, used, cap, last_call, pending, have.ctypes.data,
                                                want.ctypes.data, want_cap, cap_limit, slots.ctypes.data,
                                                keys.ctypes.data, busy, sleep)


def test_reason_names():
    names = [_native.lib.fac_diag_rc_reset_name(r).decode() for r in range(8)]
    assert names == ["none", "fresh", "signature", "pool", "directory", "busy", "off", "gated"]


def test_carries_over():
    assert decide() == KEEP


def test_empty_or_invalid_store_is_fresh():
    assert decide(valid=0) == FRESH
    assert decide(used=0) == FRESH
    # nothing to compare a signature with: an invalid store of another signature is fresh, not a reset
    assert decide(valid=0, want=SIG + 1) == FRESH


def test_signature_every_word_counts():
    for i in range(16):
        want = SIG.copy()
        want[i] ^= 1 << (i % 32)
        assert decide(want=want) == SIGNATURE, i


def test_pool_free_space():
    # a warm store expects what the previous call appended
    assert decide(used=9_900, last_call=100) == KEEP
    assert decide(used=9_901, last_call=100) == POOL
    # after the store's first call, which built every key: half of it
    assert decide(calls=1, used=6_000, last_call=6_000) == KEEP
    assert decide(calls=1, used=7_001, last_call=7_001) == POOL
    # never more than the call would allocate for itself
    assert decide(used=9_000, last_call=5_000, want_cap=1_000) == KEEP
    # the test knob lowers the pool's end; a store already past it is given up
    assert decide(used=1_000, last_call=100, cap_limit=1_099) == POOL
    assert decide(used=1_000, last_call=100, cap_limit=1_100) == KEEP
    assert decide(used=1_000, last_call=0, cap_limit=999) == POOL


def test_pool_sized_for_much_smaller_calls():
    assert decide(want_cap=20_000) == KEEP
    assert decide(want_cap=20_001) == POOL


def test_directory_load():
    slots, keys = [0] * 9, [0] * 9
    slots[5], keys[5] = 4096, 2048
    assert decide(slots=slots, keys=keys) == KEEP
    keys[5] = 2049
    assert decide(slots=slots, keys=keys) == DIRECTORY
    # a signature change is reported first: the directories are emptied either way
    assert decide(slots=slots, keys=keys, want=SIG + 1) == SIGNATURE


def test_pending_reason_of_the_previous_call():
    assert decide(pending=POOL) == POOL
    assert decide(pending=DIRECTORY) == DIRECTORY
    assert decide(pending=POOL, used=0) == FRESH  # dropped in between: nothing left to give up


def test_busy_store_is_left_alone():
    assert decide(busy=1) == BUSY
    assert decide(busy=1, want=SIG + 1) == BUSY
    assert decide(busy=0) == KEEP


def test_gate_for_unlike_text():
    gate = _native.lib.fac_diag_rc_store_gate
    assert decide(sleep=3) == 7 and decide(sleep=3, valid=0) == 7  # gated calls go without the store
    assert gate(10, 90, 0, 1) == 0  # a tenth carried: the store stays in use
    assert gate(9, 91, 0, 1) == 1 and gate(9, 91, 1, 1) == 2 and gate(9, 91, 32, 1) == 64 and gate(0, 100, 64, 1) == 64
    assert gate(50, 50, 8, 1) == 0  # like text again ends the back-off
    assert gate(0, 65535, 4, 65536) == 0 and gate(0, 65536, 4, 65536) == 8  # small calls are not judged
