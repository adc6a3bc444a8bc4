"""Direct calls: a call whose text the engine's snapshot store already knows
probes the store's directories and runs no counts, selections or builds. Every call of every case
compares all fields of its records with the CPU oracle and with the same call under
FAC_RC_NO_CARRY=1; the `direct=` item of the FAC_RC_DEBUG line shows that a case exercised what it
claims. Shapes and knobs are those of test_gpu_prefix_carry.py, plus FAC_RC_DIRECT_MIN=1 (by default
calls under 2^20 windows never go direct)."""
import re
import threading

import pytest

from fuzzy_aho_corasick import FuzzyAhoCorasickBuilder as B, FuzzyLimits as L
from test_gpu_build_epilogue import Rng, _wordy, word
from test_gpu_prefix_carry import STATS, Info, oracle
from test_gpu_prefix_carry import knobs as carry_knobs

pytestmark = pytest.mark.gpu

DIRECT = ("FAC_RC_DIRECT_MIN", "FAC_RC_DIRECT_PM", "FAC_RC_NO_DIRECT")


def knobs(monkeypatch, k, levels):
    carry_knobs(monkeypatch, k, levels)
    for name in DIRECT:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("FAC_RC_DIRECT_MIN", "1")


class DInfo(Info):
    """Info plus the direct items of the carry part: direct (None without the line), the sampled
    unknown share and the store's floor (per mille, -1: none), and why a call did not go direct."""

    def __init__(self, err):
        super().__init__(err)
        m = re.search(r"direct=([01]) unknown_pm=(-?\d+) floor_pm=(-?\d+)(?: why=(\w+))?", self.line)
        self.direct = bool(int(m.group(1))) if m else None
        self.unknown_pm, self.floor_pm = (int(m.group(2)), int(m.group(3))) if m else (-1, -1)
        self.why = m.group(4) if m else None


def call(monkeypatch, capfd, staged, thr, want=None, **search):
    """test_gpu_prefix_carry.call with the direct items read."""
    monkeypatch.setenv("FAC_RC_DEBUG", "1")
    capfd.readouterr()
    rows, st = staged.search_windows(thr, **search)
    info = DInfo(capfd.readouterr().err)
    monkeypatch.setenv("FAC_RC_NO_CARRY", "1")
    cold, _ = staged.search_windows(thr, **search)
    monkeypatch.delenv("FAC_RC_NO_CARRY")
    monkeypatch.delenv("FAC_RC_DEBUG")
    capfd.readouterr()
    rows, cold = sorted(rows), sorted(cold)
    assert rows == cold
    if want is not None:
        assert rows == want
    print(f"records={len(rows)} direct={info.direct} why={info.why} unknown_pm={info.unknown_pm} floor_pm={info.floor_pm} "
          f"levels={info.levels} pool_words={info.pool_words} dir_keys={info.dir_keys} reset={info.reset} "
          f"popped={st.states_popped} cached={st.states_cached} lane={st.lane_windows}")
    return rows, st, info


def full_then_direct(monkeypatch, capfd, builder, pats, hay, thr, k, levels):
    """The same haystack twice: a fresh full call, then a direct call that finds the same snapshots."""
    knobs(monkeypatch, k, levels)
    want = oracle(builder, pats, hay, thr)
    staged = builder.build(pats).stage(hay.encode("utf-8"))
    rows1, st1, i1 = call(monkeypatch, capfd, staged, thr, want)
    rows2, st2, i2 = call(monkeypatch, capfd, staged, thr, want)
    assert i1.reset == "fresh" and i1.direct is False and i1.built > 0 and i1.floor_pm >= 0, i1.line
    assert i2.direct is True and i2.reset == "none" and not i2.levels, i2.line
    assert i2.unknown_pm == i1.floor_pm == i2.floor_pm, i2.line  # the same windows sampled over the same directories
    assert i2.pool_words == i1.pool_words and i2.dir_keys == i1.dir_keys
    for f in STATS:
        assert getattr(st1, f) == getattr(st2, f), f
    return rows1, i1, i2


# ---- 1. the same haystack twice
def test_same_haystack_unbeamed_two_edits(monkeypatch, capfd):
    pats, text = _wordy(0x2ed17, 120)
    rows, _, _ = full_then_direct(monkeypatch, capfd, B().fuzzy(L().edits(2)), pats, text, 0.6, "4", "5,6")
    assert rows


def test_same_haystack_one_edit(monkeypatch, capfd):
    pats, text = _wordy(0x1ed17, 120)
    rows, _, _ = full_then_direct(monkeypatch, capfd, B().fuzzy(L().edits(1)), pats, text, 0.6, "4", "5")
    assert rows


@pytest.mark.parametrize("levels,k", [("2,4", "2"), ("4,5,6", "3")])
@pytest.mark.parametrize("width", [4, 8])
def test_same_haystack_beamed(width, levels, k, monkeypatch, capfd):
    pats, text = _wordy(0xbea3 + width, 120)
    rows, i1, _ = full_then_direct(monkeypatch, capfd, B().fuzzy(L().edits(2)).beam_width(width), pats, text, 0.6, k, levels)
    assert rows and i1.final_open[1] > 0


# ---- 2. haystack B after A, sharing part of their words
def test_partly_shared_haystacks(monkeypatch, capfd):
    builder = B().fuzzy(L().edits(2))
    pats, text = _wordy(0x5ba7e, 120)
    words = text.split(" ")
    a = " ".join(words[:320])
    b = " ".join(words[200:])  # 120 words of A, the rest new
    wa, wb = oracle(builder, pats, a, 0.6), oracle(builder, pats, b, 0.6)
    knobs(monkeypatch, "4", "5,6")
    # margin 0: B's unknown share is above the floor A left, so B is a full call that builds
    monkeypatch.setenv("FAC_RC_DIRECT_PM", "0")
    engine = builder.build(pats)
    sa, sb = engine.stage(a.encode()), engine.stage(b.encode())
    _, _, ia = call(monkeypatch, capfd, sa, 0.6, wa)
    _, _, ib = call(monkeypatch, capfd, sb, 0.6, wb)
    assert ib.direct is False and ib.why == "share" and ib.unknown_pm > ia.floor_pm, ib.line
    assert ib.reset == "none" and ib.built > 0 and ib.dir_keys > ia.dir_keys, ib.line
    # any margin: B goes direct although many of its keys are unknown (they fall through to shallower
    # levels and to uncached searches), and the store stays as A left it
    monkeypatch.setenv("FAC_RC_DIRECT_PM", "1000")
    engine = builder.build(pats)
    sa, sb = engine.stage(a.encode()), engine.stage(b.encode())
    _, _, ia = call(monkeypatch, capfd, sa, 0.6, wa)
    _, _, ib = call(monkeypatch, capfd, sb, 0.6, wb)
    assert ib.direct is True and ib.unknown_pm > ia.floor_pm, ib.line
    assert ib.pool_words == ia.pool_words and ib.dir_keys == ia.dir_keys and ib.dir_slots == ia.dir_slots
    _, _, ia2 = call(monkeypatch, capfd, sa, 0.6, wa)
    assert ia2.direct is True and ia2.pool_words == ia.pool_words


# ---- 3. directories holding uncached marks (keys whose parent is final)
def test_final_snapshots_with_records(monkeypatch, capfd):
    rng = Rng(0xbe57)
    pats = sorted({word(rng, "abc", 2, 3) for _ in range(40)})
    hay = "".join(pats[rng.next() % len(pats)] if rng.next() % 3 == 0 else "xyz "[rng.next() % 4] * (1 + rng.next() % 5)
                  for _ in range(1500))[:6001]
    rows, i1, _ = full_then_direct(monkeypatch, capfd, B().fuzzy(L().edits(1)), pats, hay, 0.6, "4", "5")
    assert rows and i1.final_open[0] > 0


def test_final_snapshots_without_records(monkeypatch, capfd):
    rng = Rng(0xf17a1 + 2)
    pats = [word(rng, "abcdefgh", 6, 10) for _ in range(40)] + ["q"]
    hay = "".join("XYZW0123"[rng.next() % 8] for _ in range(4099))
    rows, i1, _ = full_then_direct(monkeypatch, capfd, B().fuzzy(L().edits(2)), pats, hay, 0.8, "4", "5,6")
    assert rows == [] and i1.final_open[0] > 0 and i1.final_open[1] == 0


# ---- 4. texts that end inside the keys; ASCII and non-ASCII segments in one call
def test_text_ends_inside_keys(monkeypatch, capfd):
    builder = B().fuzzy(L().edits(2))
    pats, text = _wordy(0x7e47, 120)
    knobs(monkeypatch, "4", "5,6")
    monkeypatch.setenv("FAC_RC_DIRECT_PM", "1000")  # a few windows: their share is anything
    engine = builder.build(pats)
    call(monkeypatch, capfd, engine.stage(text.encode()), 0.6, oracle(builder, pats, text, 0.6))
    start = text.index(pats[0][:4]) if pats[0][:4] in text else 0
    direct = 0
    for n in range(1, 10):
        hay = text[start:start + n]
        _, _, i = call(monkeypatch, capfd, engine.stage(hay.encode()), 0.6, oracle(builder, pats, hay, 0.6))
        direct += i.direct is True
    assert direct > 0


def test_mixed_text_kinds_in_one_call(monkeypatch, capfd):
    builder = B().fuzzy(L().edits(2)).case_insensitive(True)
    pats, text = _wordy(0x6a5c, 120)
    rng = Rng(0x6a5d)
    words = text.split(" ")
    # ASCII runs and runs with accents and characters past the 16-bit key units, at every key position
    astral = ["\U0001d4b3", "￿", "\U00010000"]
    mixed = []
    for n, w in enumerate(words):
        if (n // 40) % 2:
            p = rng.next() % (len(w) + 1)
            w = w[:p] + (astral[rng.next() % 3] if rng.next() % 2 else "é") + w[p:]
        mixed.append(w.upper() if rng.next() % 3 == 0 else w)
    hay = " ".join(mixed)[:5003]
    assert any(ord(c) >= 0xFFFF for c in hay) and hay[:100].isascii()
    knobs(monkeypatch, "4", "5,6")
    staged = builder.build(pats).stage(hay.encode("utf-8"))
    want = oracle(builder, pats, hay, 0.6)
    assert want
    _, st1, i1 = call(monkeypatch, capfd, staged, 0.6, want)
    _, st2, i2 = call(monkeypatch, capfd, staged, 0.6, want)
    assert i1.direct is False and i2.direct is True, i2.line
    for f in STATS:
        assert getattr(st1, f) == getattr(st2, f), f


# ---- 5. a changed threshold after a direct-eligible state
def test_signature_change(monkeypatch, capfd):
    builder = B().fuzzy(L().edits(2))
    pats, text = _wordy(0x51647, 120)
    knobs(monkeypatch, "4", "5,6")
    staged = builder.build(pats).stage(text.encode())
    want = {t: oracle(builder, pats, text, t) for t in (0.8, 0.6)}
    assert want[0.8] != want[0.6]
    _, _, i = call(monkeypatch, capfd, staged, 0.8, want[0.8])
    assert i.reset == "fresh" and i.direct is False
    _, _, i = call(monkeypatch, capfd, staged, 0.8, want[0.8])
    assert i.direct is True
    _, _, i = call(monkeypatch, capfd, staged, 0.6, want[0.6])
    assert i.reset == "signature" and i.direct is False and i.why == "reset" and i.built > 0, i.line
    _, _, i = call(monkeypatch, capfd, staged, 0.6, want[0.6])
    assert i.direct is True, i.line


# ---- 6. the pool runs out: the call after the pending reset
def test_pool_exhaustion(monkeypatch, capfd):
    builder = B().fuzzy(L().edits(2))
    pats, text = _wordy(0x9001, 120)
    knobs(monkeypatch, "4", "5,6")
    want = oracle(builder, pats, text, 0.6)
    _, _, i0 = call(monkeypatch, capfd, builder.build(pats).stage(text.encode()), 0.6, want)
    staged = builder.build(pats).stage(text.encode())
    monkeypatch.setenv("FAC_RC_POOL_WORDS", str(i0.pool_words // 2))  # the first call's snapshots do not fit
    _, _, i1 = call(monkeypatch, capfd, staged, 0.6, want)
    assert i1.reset == "fresh" and i1.direct is False
    _, _, i2 = call(monkeypatch, capfd, staged, 0.6, want)  # the store is to be emptied: nothing to go direct on
    assert i2.direct is False and i2.why == "reset" and i2.reset in ("pool", "gated"), i2.line
    monkeypatch.delenv("FAC_RC_POOL_WORDS")
    infos = [call(monkeypatch, capfd, staged, 0.6, want)[2] for _ in range(3)]
    assert infos[-1].direct is True, [i.line for i in infos]


# ---- 7. key partition after a warm whole-haystack call
def test_key_partition_after_warm_call(monkeypatch, capfd):
    builder = B().fuzzy(L().edits(2))
    pats, text = _wordy(0x9a27, 120)
    knobs(monkeypatch, "4", "5,6")
    monkeypatch.setenv("FAC_RC_DIRECT_PM", "1000")  # a part's windows are chosen by key: its share is its own
    staged = builder.build(pats).stage(text.encode())
    want = oracle(builder, pats, text, 0.6)
    call(monkeypatch, capfd, staged, 0.6, want)
    union = []
    for r in (0, 1):
        staged.set_key_partition(2, r)
        rows, _, i = call(monkeypatch, capfd, staged, 0.6)
        assert i.direct is True, i.line
        union += rows
    staged.set_key_partition(1, 0)
    assert sorted(union) == want


# ---- 8. two threads on one engine
def test_two_threads_one_engine(monkeypatch, capfd):
    builder = B().fuzzy(L().edits(2))
    pats, text = _wordy(0x7a2ead, 120)
    words = text.split(" ")
    hays = [" ".join(words[:300]), " ".join(words[150:])]
    knobs(monkeypatch, "4", "5,6")
    monkeypatch.setenv("FAC_RC_DIRECT_PM", "1000")
    engine = builder.build(pats)
    staged = [engine.stage(h.encode()) for h in hays]
    want = [oracle(builder, pats, h, 0.6) for h in hays]
    call(monkeypatch, capfd, staged[0], 0.6, want[0])
    monkeypatch.setenv("FAC_RC_DEBUG", "1")
    capfd.readouterr()
    got = [[], []]

    def work(t):
        for _ in range(4):
            got[t].append(sorted(staged[t].search_windows(0.6)[0]))

    threads = [threading.Thread(target=work, args=(t,)) for t in (0, 1)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    monkeypatch.delenv("FAC_RC_DEBUG")
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("FAC_RC windows=")]
    for t in (0, 1):
        assert len(got[t]) == 4
        for rows in got[t]:
            assert rows == want[t]
    infos = [DInfo(ln) for ln in lines]
    assert len(infos) == 8
    for i in infos:  # a call that found the store taken searched without it
        assert i.direct is False if i.reset == "busy" else i.direct is True, i.line


# ---- 9. drop_prefix_cache
def test_drop(monkeypatch, capfd):
    builder = B().fuzzy(L().edits(2))
    pats, text = _wordy(0xd209, 120)
    knobs(monkeypatch, "4", "5,6")
    engine = builder.build(pats)
    staged = engine.stage(text.encode())
    want = oracle(builder, pats, text, 0.6)
    _, _, i1 = call(monkeypatch, capfd, staged, 0.6, want)
    _, _, i2 = call(monkeypatch, capfd, staged, 0.6, want)
    assert i2.direct is True
    engine.drop_prefix_cache()
    _, _, i3 = call(monkeypatch, capfd, staged, 0.6, want)
    assert i3.reset == "fresh" and i3.direct is False and i3.levels == i1.levels, i3.line
    _, _, i4 = call(monkeypatch, capfd, staged, 0.6, want)
    assert i4.direct is True


# ---- 10. FAC_RC_NO_DIRECT=1: the full pipeline
def test_no_direct_knob(monkeypatch, capfd):
    builder = B().fuzzy(L().edits(2))
    pats, text = _wordy(0x2ed17, 120)
    knobs(monkeypatch, "4", "5,6")
    staged = builder.build(pats).stage(text.encode())
    want = oracle(builder, pats, text, 0.6)
    _, st1, i1 = call(monkeypatch, capfd, staged, 0.6, want)
    _, st2, i2 = call(monkeypatch, capfd, staged, 0.6, want)
    monkeypatch.setenv("FAC_RC_NO_DIRECT", "1")
    _, st3, i3 = call(monkeypatch, capfd, staged, 0.6, want)
    assert i2.direct is True and i3.direct is False and i3.why == "off", i3.line
    assert i3.reset == "none" and i3.built == 0 and i3.carried > 0 and set(i3.levels) == set(i1.levels), i3.line
    for f in STATS:
        assert getattr(st1, f) == getattr(st2, f) == getattr(st3, f), f


# ---- 11. a warm store, then haystacks a quarter and four times the size
def test_other_sizes_on_the_stores_levels(monkeypatch, capfd):
    builder = B().fuzzy(L().edits(2))
    pats, text = _wordy(0x51e5, 120)
    rng = Rng(0x51e6)
    words = text.split(" ")
    big = " ".join(words[rng.next() % len(words)] for _ in range(4 * len(words)))[:4 * len(text)]
    small = text[len(text) // 2: len(text) // 2 + len(text) // 4]
    # level 1 not pinned: the call's own choice of key length follows its window count
    knobs(monkeypatch, "4", "5,6")
    monkeypatch.delenv("FAC_RC_K")
    monkeypatch.setenv("FAC_RC_DIRECT_PM", "1000")
    engine = builder.build(pats)
    _, _, i0 = call(monkeypatch, capfd, engine.stage(text.encode()), 0.6, oracle(builder, pats, text, 0.6))
    assert i0.direct is False
    for hay in (small, big):
        _, _, i = call(monkeypatch, capfd, engine.stage(hay.encode()), 0.6, oracle(builder, pats, hay, 0.6))
        assert i.direct is True and i.pool_words == i0.pool_words and i.dir_keys == i0.dir_keys, i.line
