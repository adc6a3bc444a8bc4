"""The engine's snapshot store: prefix-cache snapshots are kept from call to
call, and a level's build runs only for the keys no earlier call built. Every call of every case
compares all fields of its records with the CPU oracle and with the same call under
FAC_RC_NO_CARRY=1 (the pool from call scratch, every key built); the `carry` part of the FAC_RC_DEBUG
line (per level `carried=` / `built=`, the store's pool words, `reset=`) shows that a case exercised
what it is meant to. Shapes and knobs are those of test_gpu_build_epilogue.py."""
import re
import threading

import pytest

from fuzzy_aho_corasick import FuzzyAhoCorasickBuilder as B, FuzzyLimits as L
from oracle_harness import OracleEngine
from test_gpu_build_epilogue import RC_KNOBS, Rng, _wordy, word

pytestmark = pytest.mark.gpu

OTHER = ("FAC_NO_RC", "FAC_RC_FULL_SWEEP", "FAC_RC_DEBUG", "FAC_RC_NO_CARRY", "FAC_RC_POOL_WORDS", "FAC_RC_POOL_MB",
         "FAC_RC_GATE_MIN")
STATS = ("states_popped", "states_cached", "lane_windows")


def knobs(monkeypatch, k, levels):
    for name in RC_KNOBS + OTHER:
        monkeypatch.delenv(name, raising=False)
    for name, v in (("FAC_RC_MIN", "1"), ("FAC_RC_MIN2", "1"), ("FAC_RC_STRIDE2", "1"), ("FAC_RC_T2", "1"),
                    ("FAC_RC_K", k), ("FAC_RC_LEVELS", levels)):
        monkeypatch.setenv(name, v)


class Info:
    """The carry part of one FAC_RC line: levels {k: (carried, built)}, pool words, reset reason.
    A call without the line (too few windows for the cache) has no levels."""

    def __init__(self, err):
        lines = [ln for ln in err.splitlines() if ln.startswith("FAC_RC windows=")]
        self.line = lines[-1] if lines else ""
        part = self.line.split("| carry", 1)[1] if "| carry" in self.line else ""
        self.levels = {int(k): (int(c), int(b)) for k, c, b in re.findall(r"k=(\d+) carried=(\d+) built=(\d+)", part)}
        m = re.search(r"store pool_words=(\d+) dir_keys=(\d+) dir_slots=(\d+) reset=(\w+)", part)
        self.pool_words, self.dir_keys, self.dir_slots = (int(m.group(i)) for i in (1, 2, 3)) if m else (0, 0, 0)
        self.reset = m.group(4) if m else None

    @property
    def final_open(self):  # cached keys over all levels: (final, open)
        c = re.findall(r"final=(\d+) open=(\d+)", self.line)
        return sum(int(f) for f, _ in c), sum(int(o) for _, o in c)

    @property
    def carried(self):
        return sum(c for c, _ in self.levels.values())

    @property
    def built(self):
        return sum(b for _, b in self.levels.values())


def call(monkeypatch, capfd, staged, thr, want=None, **search):
    """One search with the store, then the same search without it: equal records, both the oracle's
    when `want` is given. Returns (sorted rows, stats, Info of the call with the store)."""
    monkeypatch.setenv("FAC_RC_DEBUG", "1")
    capfd.readouterr()
    rows, st = staged.search_windows(thr, **search)
    info = Info(capfd.readouterr().err)
    monkeypatch.setenv("FAC_RC_NO_CARRY", "1")
    cold, st_cold = staged.search_windows(thr, **search)
    monkeypatch.delenv("FAC_RC_NO_CARRY")
    monkeypatch.delenv("FAC_RC_DEBUG")
    capfd.readouterr()
    rows, cold = sorted(rows), sorted(cold)
    assert rows == cold
    if want is not None:
        assert rows == want
    print(f"records={len(rows)} levels={info.levels} pool_words={info.pool_words} dir_keys={info.dir_keys} "
          f"reset={info.reset} popped={st.states_popped} cached={st.states_cached} lane={st.lane_windows}")
    return rows, st, info


def oracle(builder, pats, hay, thr):
    return sorted(OracleEngine(builder, pats).raw_rows(hay, thr))


def same_twice(monkeypatch, capfd, builder, pats, hay, thr, k, levels):
    knobs(monkeypatch, k, levels)
    want = oracle(builder, pats, hay, thr)
    staged = builder.build(pats).stage(hay.encode("utf-8"))
    rows1, st1, i1 = call(monkeypatch, capfd, staged, thr, want)
    rows2, st2, i2 = call(monkeypatch, capfd, staged, thr, want)
    assert i1.levels and i1.carried == 0 and i1.built > 0 and i1.reset == "fresh", i1.line
    assert i2.reset == "none" and set(i2.levels) == set(i1.levels), i2.line
    for k2, (c, b) in i2.levels.items():
        assert b == 0 and c > 0, (k2, i2.line)
    assert i2.pool_words == i1.pool_words  # nothing appended
    for f in STATS:
        assert getattr(st1, f) == getattr(st2, f), f
    return rows1, i1, i2


# ---- 1. the same haystack twice
def test_same_haystack_unbeamed_two_edits(monkeypatch, capfd):
    pats, text = _wordy(0x2ed17, 120)
    rows, _, _ = same_twice(monkeypatch, capfd, B().fuzzy(L().edits(2)), pats, text, 0.6, "4", "5,6")
    assert rows


def test_same_haystack_one_edit(monkeypatch, capfd):
    pats, text = _wordy(0x1ed17, 120)
    rows, _, _ = same_twice(monkeypatch, capfd, B().fuzzy(L().edits(1)), pats, text, 0.6, "4", "5")
    assert rows


@pytest.mark.parametrize("levels,k", [("2,4", "2"), ("4,5,6", "3")])
@pytest.mark.parametrize("width", [4, 8])
def test_same_haystack_beamed(width, levels, k, monkeypatch, capfd):
    """Open snapshots with check entries (ncheck > 0) carried into the lane kernel's and the live pass's
    dedup-free resumes (test_gpu_build_epilogue.test_beamed_engine_check_entries shows they have them)."""
    pats, text = _wordy(0xbea3 + width, 120)
    rows, i1, _ = same_twice(monkeypatch, capfd, B().fuzzy(L().edits(2)).beam_width(width), pats, text, 0.6, k, levels)
    assert rows and i1.final_open[1] > 0


# ---- 2. haystack B after A, sharing part of their words; then A again
def test_partly_shared_haystacks(monkeypatch, capfd):
    builder = B().fuzzy(L().edits(2))
    pats, text = _wordy(0x5ba7e, 120)
    words = text.split(" ")
    a = " ".join(words[:320])
    b = " ".join(words[200:])  # 120 words of A, the rest new
    knobs(monkeypatch, "4", "5,6")
    engine = builder.build(pats)
    sa, sb = engine.stage(a.encode()), engine.stage(b.encode())
    _, _, ia = call(monkeypatch, capfd, sa, 0.6, oracle(builder, pats, a, 0.6))
    _, _, ib = call(monkeypatch, capfd, sb, 0.6, oracle(builder, pats, b, 0.6))
    assert ia.carried == 0 and ib.reset == "none"
    assert any(c > 0 and bl > 0 for c, bl in ib.levels.values()), ib.line  # skipped and built side by side
    assert ib.pool_words > ia.pool_words and ib.dir_keys > ia.dir_keys
    _, _, ia2 = call(monkeypatch, capfd, sa, 0.6, oracle(builder, pats, a, 0.6))
    assert ia2.reset == "none" and ia2.built == 0 and ia2.carried > 0, ia2.line  # the directory accumulates
    assert ia2.pool_words == ib.pool_words


# ---- 3. final snapshots with and without records
def test_final_snapshots_with_records(monkeypatch, capfd):
    rng = Rng(0xbe57)
    pats = sorted({word(rng, "abc", 2, 3) for _ in range(40)})
    hay = "".join(pats[rng.next() % len(pats)] if rng.next() % 3 == 0 else "xyz "[rng.next() % 4] * (1 + rng.next() % 5)
                  for _ in range(1500))[:6001]
    rows, i1, _ = same_twice(monkeypatch, capfd, B().fuzzy(L().edits(1)), pats, hay, 0.6, "4", "5")
    assert rows and i1.final_open[0] > 0


def test_final_snapshots_without_records(monkeypatch, capfd):
    rng = Rng(0xf17a1 + 2)
    pats = [word(rng, "abcdefgh", 6, 10) for _ in range(40)] + ["q"]
    hay = "".join("XYZW0123"[rng.next() % 8] for _ in range(4099))
    rows, i1, _ = same_twice(monkeypatch, capfd, B().fuzzy(L().edits(2)), pats, hay, 0.8, "4", "5,6")
    assert rows == [] and i1.final_open[0] > 0 and i1.final_open[1] == 0


# ---- 4. a signature change empties the store
def test_signature_change(monkeypatch, capfd):
    builder = B().fuzzy(L().edits(2))
    pats, text = _wordy(0x51647, 120)
    knobs(monkeypatch, "4", "5,6")
    staged = builder.build(pats).stage(text.encode())
    want = {t: oracle(builder, pats, text, t) for t in (0.8, 0.6)}
    assert want[0.8] != want[0.6]
    _, _, i = call(monkeypatch, capfd, staged, 0.8, want[0.8])
    assert i.reset == "fresh"
    for thr in (0.6, 0.8):
        _, _, i = call(monkeypatch, capfd, staged, thr, want[thr])
        assert i.reset == "signature" and i.carried == 0 and i.built > 0, i.line
    _, _, i = call(monkeypatch, capfd, staged, 0.8, want[0.8])
    assert i.reset == "none" and i.built == 0, i.line


# ---- 5. texts that end inside the keys, after a warm call
def test_text_ends_inside_keys(monkeypatch, capfd):
    builder = B().fuzzy(L().edits(2))
    pats, text = _wordy(0x7e47, 120)
    knobs(monkeypatch, "4", "5,6")
    engine = builder.build(pats)
    call(monkeypatch, capfd, engine.stage(text.encode()), 0.6, oracle(builder, pats, text, 0.6))
    start = text.index(pats[0][:4]) if pats[0][:4] in text else 0
    seen = 0
    for n in range(1, 10):
        hay = text[start:start + n]
        _, _, i = call(monkeypatch, capfd, engine.stage(hay.encode()), 0.6, oracle(builder, pats, hay, 0.6))
        seen += len(i.levels)
    assert seen > 0  # the short texts ran the cache (window counts below the levels' key lengths)
    _, _, i = call(monkeypatch, capfd, engine.stage(text.encode()), 0.6, oracle(builder, pats, text, 0.6))
    assert i.carried > 0


# ---- 6. ASCII and non-ASCII text alternating on a case-insensitive engine
def test_mixed_text_kinds(monkeypatch, capfd):
    builder = B().fuzzy(L().edits(2)).case_insensitive(True)
    pats, text = _wordy(0x6a5c, 120)
    rng = Rng(0x6a5d)
    uni = " ".join((w.upper() if rng.next() % 3 == 0 else w) + ("é" if rng.next() % 4 == 0 else "")
                   for w in text.split(" "))[:5003]
    knobs(monkeypatch, "4", "5,6")
    engine = builder.build(pats)
    sa, su = engine.stage(text.encode()), engine.stage(uni.encode("utf-8"))
    wa, wu = oracle(builder, pats, text, 0.6), oracle(builder, pats, uni, 0.6)
    assert wa and wu
    infos = []
    for _ in range(2):
        infos.append(call(monkeypatch, capfd, sa, 0.6, wa)[2])
        infos.append(call(monkeypatch, capfd, su, 0.6, wu)[2])
    assert infos[1].carried > 0  # folded upper-case words meet the ASCII haystack's keys
    assert infos[2].built == 0 and infos[3].built == 0 and infos[3].carried > 0


# ---- 7. the pool runs out
def test_pool_exhaustion(monkeypatch, capfd):
    builder = B().fuzzy(L().edits(2))
    pats, text = _wordy(0x9001, 120)
    words = text.split(" ")
    hays = [" ".join(words[i::3]) for i in range(3)]
    knobs(monkeypatch, "4", "5,6")
    engine = builder.build(pats)
    staged = [engine.stage(h.encode()) for h in hays]
    want = [oracle(builder, pats, h, 0.6) for h in hays]
    _, _, i0 = call(monkeypatch, capfd, staged[0], 0.6, want[0])
    _, _, i1 = call(monkeypatch, capfd, staged[1], 0.6, want[1])
    assert i1.reset == "none" and i1.pool_words > i0.pool_words
    # room for less than the second call appended: the third haystack cannot count on its append
    monkeypatch.setenv("FAC_RC_POOL_WORDS", str(i1.pool_words + (i1.pool_words - i0.pool_words) // 2))
    _, _, i2 = call(monkeypatch, capfd, staged[2], 0.6, want[2])
    assert i2.reset == "pool" and i2.carried == 0, i2.line
    monkeypatch.delenv("FAC_RC_POOL_WORDS")
    _, _, i3 = call(monkeypatch, capfd, staged[2], 0.6, want[2])
    assert i3.reset == "none" and i3.carried > 0 and i3.built == 0, i3.line


# ---- 8. two engines on one device
def test_two_engines_alternating(monkeypatch, capfd):
    builder = B().fuzzy(L().edits(2))
    pats, text = _wordy(0x2e61, 120)
    pa, pb = pats[: len(pats) // 2], pats[len(pats) // 2:]
    knobs(monkeypatch, "4", "5,6")
    ea, eb = builder.build(pa), builder.build(pb)
    sa, sb = ea.stage(text.encode()), eb.stage(text.encode())
    wa, wb = oracle(builder, pa, text, 0.6), oracle(builder, pb, text, 0.6)
    assert wa and wb and wa != wb
    for r in range(2):
        _, _, ia = call(monkeypatch, capfd, sa, 0.6, wa)
        _, _, ib = call(monkeypatch, capfd, sb, 0.6, wb)
        assert (ia.carried == 0 and ib.carried == 0) if r == 0 else (ia.built == 0 and ib.built == 0)


# ---- 9. key partition after a warm whole-haystack call
def test_key_partition_after_warm_call(monkeypatch, capfd):
    builder = B().fuzzy(L().edits(2))
    pats, text = _wordy(0x9a27, 120)
    knobs(monkeypatch, "4", "5,6")
    staged = builder.build(pats).stage(text.encode())
    want = oracle(builder, pats, text, 0.6)
    call(monkeypatch, capfd, staged, 0.6, want)
    union, carried = [], 0
    for r in (0, 1):
        staged.set_key_partition(2, r)
        rows, _, i = call(monkeypatch, capfd, staged, 0.6)
        union += rows
        carried += i.carried
    staged.set_key_partition(1, 0)
    assert sorted(union) == want and carried > 0


# ---- 10. two threads on one engine
def test_two_threads_one_engine(monkeypatch, capfd):
    builder = B().fuzzy(L().edits(2))
    pats, text = _wordy(0x7a2ead, 120)
    words = text.split(" ")
    hays = [" ".join(words[:300]), " ".join(words[150:])]
    knobs(monkeypatch, "4", "5,6")
    engine = builder.build(pats)
    staged = [engine.stage(h.encode()) for h in hays]
    want = [oracle(builder, pats, h, 0.6) for h in hays]
    got = [[], []]

    def work(t):
        for _ in range(4):
            got[t].append(sorted(staged[t].search_windows(0.6)[0]))

    threads = [threading.Thread(target=work, args=(t,)) for t in (0, 1)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for t in (0, 1):
        assert len(got[t]) == 4
        for rows in got[t]:
            assert rows == want[t]


# ---- 11. drop_prefix_cache
def test_drop(monkeypatch, capfd):
    builder = B().fuzzy(L().edits(2))
    pats, text = _wordy(0xd209, 120)
    knobs(monkeypatch, "4", "5,6")
    engine = builder.build(pats)
    staged = engine.stage(text.encode())
    want = oracle(builder, pats, text, 0.6)
    _, _, i1 = call(monkeypatch, capfd, staged, 0.6, want)
    engine.drop_prefix_cache()
    _, _, i2 = call(monkeypatch, capfd, staged, 0.6, want)
    assert i2.reset == "fresh" and i2.carried == 0 and i2.levels == i1.levels, i2.line
    _, _, i3 = call(monkeypatch, capfd, staged, 0.6, want)
    assert i3.built == 0 and i3.carried > 0


# ---- 12. the gate for unlike text
def test_gate_for_unlike_text(monkeypatch, capfd):
    """A carrying call that finds under a tenth of its entries sends the next call past the store
    (reset=gated, every key built from call scratch); the call after that starts the store empty.
    FAC_RC_GATE_MIN=1 lets a call this small be judged (default: 65536 entries)."""
    builder = B().fuzzy(L().edits(2))
    pats, text = _wordy(0x9a7e, 120)
    rng = Rng(0x9a7f)
    other = " ".join(word(rng, "qrstuvw0123", 3, 9) for _ in range(900))[:5003]
    knobs(monkeypatch, "4", "5,6")
    monkeypatch.setenv("FAC_RC_GATE_MIN", "1")
    engine = builder.build(pats)
    sa, so = engine.stage(text.encode()), engine.stage(other.encode())
    wa, wo = oracle(builder, pats, text, 0.6), oracle(builder, pats, other, 0.6)
    _, _, i = call(monkeypatch, capfd, sa, 0.6, wa)
    assert i.reset == "fresh"
    _, _, i = call(monkeypatch, capfd, so, 0.6, wo)
    assert i.reset == "none" and 10 * i.carried < i.carried + i.built, i.line
    _, _, i = call(monkeypatch, capfd, sa, 0.6, wa)
    assert i.reset == "gated" and i.carried == 0 and i.pool_words == 0, i.line
    _, _, i = call(monkeypatch, capfd, sa, 0.6, wa)
    assert i.reset == "fresh" and i.carried == 0, i.line
    _, _, i = call(monkeypatch, capfd, sa, 0.6, wa)
    assert i.reset == "none" and i.built == 0 and i.carried > 0, i.line
