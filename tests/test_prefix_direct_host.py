"""Host side of direct calls and of the emptied-store gate, without a device:
whether a call searches from the store's directories alone (fac_diag_rc_direct_decide), and the
back-off of a store that every call empties (fac_diag_rc_emptied_gate, with fac_diag_rc_store_gate
for the carrying call that ends it)."""
from fuzzy_aho_corasick import _native

KEEP, FRESH, SIGNATURE, POOL, DIRECTORY, BUSY, OFF, GATED = range(8)
MIN = 1 << 20


def direct(unknown_pm, floor_pm, margin_pm=10, sampled=16384, windows=MIN, min_windows=MIN):
    return _native.lib.fac_diag_rc_direct_decide(unknown_pm, floor_pm, margin_pm, sampled, windows, min_windows)


def test_direct_needs_a_floor():
    assert direct(0, -1) == 0
    assert direct(0, 0) == 1


def test_direct_needs_samples():
    assert direct(0, 30, sampled=0) == 0
    assert direct(0, 30, sampled=1) == 1


def test_direct_share_against_floor_and_margin():
    assert direct(39, 30) == 1
    assert direct(40, 30) == 1  # equal to floor + margin
    assert direct(41, 30) == 0
    assert direct(30, 30, margin_pm=0) == 1 and direct(31, 30, margin_pm=0) == 0
    assert direct(1000, 0, margin_pm=1000) == 1
    assert direct(1000, 999, margin_pm=2 ** 32 - 1) == 1  # no wrap-around


def test_direct_needs_enough_windows():
    assert direct(0, 30, windows=MIN - 1) == 0
    assert direct(0, 30, windows=MIN) == 1
    assert direct(0, 30, windows=1, min_windows=1) == 1


def ladder(reason):
    """Fresh-word text: a fill from empty, then `reason` empties the store. Returns the back-offs."""
    gate = _native.lib.fac_diag_rc_emptied_gate
    backoff, seen = 0, []
    for _ in range(9):
        backoff = gate(reason, 1, backoff)
        seen.append(backoff)
    return seen


def test_emptied_store_backs_off():
    assert ladder(POOL) == [1, 2, 4, 8, 16, 32, 64, 64, 64]
    assert ladder(DIRECTORY) == [1, 2, 4, 8, 16, 32, 64, 64, 64]


def test_emptied_store_only_right_after_a_fill():
    gate = _native.lib.fac_diag_rc_emptied_gate
    assert gate(POOL, 0, 0) == 0 and gate(DIRECTORY, 0, 8) == 0  # the call before carried over: an ordinary reset


def test_other_decisions_do_not_count():
    gate = _native.lib.fac_diag_rc_emptied_gate
    for reason in (KEEP, FRESH, SIGNATURE, BUSY, OFF, GATED):
        assert gate(reason, 1, 0) == 0 and gate(reason, 1, 4) == 0, reason


def test_carrying_call_ends_the_back_off():
    gate, carry = _native.lib.fac_diag_rc_emptied_gate, _native.lib.fac_diag_rc_store_gate
    backoff = gate(POOL, 1, gate(POOL, 1, 0))
    assert backoff == 2
    assert carry(10, 90, backoff, 1) == 0  # a tenth carried
    assert gate(POOL, 1, 0) == 1  # and the ladder starts over
    assert carry(9, 91, backoff, 1) == 4  # under a tenth: the same ladder goes on
