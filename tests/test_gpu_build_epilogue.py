"""The prefix-cache build epilogue (rc_build_kernel): final keys (empty queue) are
snapshotted without a sweep of the dedup table, open keys sweep it once and their writing passes read
only the entries they store. Every case compares all fields of the records with the CPU oracle, with the
cache off (FAC_NO_RC) and with the earlier epilogue (FAC_RC_FULL_SWEEP=1: three sweeps for every key),
which must write the same snapshots: equal records and equal states_popped / states_cached /
lane_windows. The FAC_RC_DEBUG line's final / open key counts show that a case builds the keys it is
meant for."""
import re

import pytest

from fuzzy_aho_corasick import FuzzyAhoCorasickBuilder as B, FuzzyLimits as L
from oracle_harness import OracleEngine

pytestmark = pytest.mark.gpu

RC_KNOBS = ("FAC_RC_MIN", "FAC_RC_MIN2", "FAC_RC_STRIDE2", "FAC_RC_T2", "FAC_RC_K", "FAC_RC_K2", "FAC_RC_LEVELS")


class Rng:  # the xorshift of the other differential tests
    def __init__(self, s):
        self.s = s

    def next(self):
        x = self.s
        x ^= (x << 13) & 0xFFFFFFFFFFFFFFFF
        x ^= x >> 7
        x ^= (x << 17) & 0xFFFFFFFFFFFFFFFF
        self.s = x
        return x


def word(rng, alphabet, lo, hi):
    return "".join(alphabet[rng.next() % len(alphabet)] for _ in range(lo + rng.next() % (hi - lo + 1)))


def check(monkeypatch, capfd, builder, pats, hay, thr, k, levels):
    """Records of the single-sweep epilogue == oracle == cache off == full-sweep epilogue, and the
    three pop statistics of the two epilogues are equal. Returns (records, keys final, keys open,
    keys refused for nv > rc_vmax) of the single-sweep run."""
    for name in RC_KNOBS + ("FAC_NO_RC", "FAC_RC_FULL_SWEEP", "FAC_RC_DEBUG"):
        monkeypatch.delenv(name, raising=False)
    staged = builder.build(pats).stage(hay.encode("utf-8"))
    for name, v in (("FAC_RC_MIN", "1"), ("FAC_RC_MIN2", "1"), ("FAC_RC_STRIDE2", "1"), ("FAC_RC_T2", "1"),
                    ("FAC_RC_K", k), ("FAC_RC_LEVELS", levels)):
        monkeypatch.setenv(name, v)
    monkeypatch.setenv("FAC_RC_DEBUG", "1")
    capfd.readouterr()
    new, st_new = staged.search_windows(thr)
    err = capfd.readouterr().err
    monkeypatch.delenv("FAC_RC_DEBUG")
    monkeypatch.setenv("FAC_RC_FULL_SWEEP", "1")
    old, st_old = staged.search_windows(thr)
    monkeypatch.delenv("FAC_RC_FULL_SWEEP")
    monkeypatch.setenv("FAC_NO_RC", "1")
    off, _ = staged.search_windows(thr)
    monkeypatch.delenv("FAC_NO_RC")
    want = sorted(OracleEngine(builder, pats).raw_rows(hay, thr))
    assert sorted(new) == want
    assert sorted(off) == want
    assert sorted(old) == want
    for f in ("states_popped", "states_cached", "lane_windows"):
        assert getattr(st_new, f) == getattr(st_old, f), f
    line = [ln for ln in err.splitlines() if ln.startswith("FAC_RC windows=")]
    assert line, err[-2000:]
    counts = re.findall(r"final=(\d+) open=(\d+)", line[-1])
    vmax = re.findall(r"FAC_RC uncached keys: .* vmax (\d+)", err)
    print(f"k={k} levels={levels} records={len(want)} final/open per level={counts} vmax-refused={vmax} "
          f"popped={st_new.states_popped} cached={st_new.states_cached} lane={st_new.lane_windows}")
    return want, sum(int(f) for f, _ in counts), sum(int(o) for _, o in counts), sum(int(v) for v in vmax)


@pytest.mark.parametrize("edits", [1, 2])
def test_every_key_final_no_records(edits, monkeypatch, capfd):
    """A haystack over characters no pattern contains: every window dies inside its key, so every key
    built is final and holds no record. (The one-character pattern keeps the 2-gram window skip of a
    one-edit engine off, which would leave no window to build a key from.)"""
    rng = Rng(0xf17a1 + edits)
    pats = [word(rng, "abcdefgh", 6, 10) for _ in range(40)] + ["q"]
    hay = "".join("XYZW0123"[rng.next() % 8] for _ in range(4099))
    rows, fin, opn, _ = check(monkeypatch, capfd, B().fuzzy(L().edits(edits)), pats, hay, 0.8, "4", "5,6")
    assert rows == [] and fin > 0 and opn == 0


def test_final_keys_with_records(monkeypatch, capfd):
    """Patterns of 2-3 characters under 4- and 5-character keys: matches end inside the key, so final
    snapshots carry a best list (and no queue or dedup entries)."""
    rng = Rng(0xbe57)
    pats = sorted({word(rng, "abc", 2, 3) for _ in range(40)})
    assert len(pats) >= 20
    hay = "".join(pats[rng.next() % len(pats)] if rng.next() % 3 == 0 else "xyz "[rng.next() % 4] * (1 + rng.next() % 5)
                  for _ in range(1500))[:6001]
    rows, fin, opn, _ = check(monkeypatch, capfd, B().fuzzy(L().edits(1)), pats, hay, 0.6, "4", "5")
    assert len(rows) > 0 and fin > 0


def _wordy(seed, npat):
    rng = Rng(seed)
    stems = [word(rng, "abcdefghijklmnop", 3, 4) for _ in range(12)]
    pats = sorted({stems[rng.next() % 12] + word(rng, "abcdefghijklmnop", 2, 6) for _ in range(npat)})
    text = " ".join(pats[rng.next() % len(pats)][: 3 + rng.next() % 8] + "xyz"[rng.next() % 3] for _ in range(500))
    return pats, text[:5003]


@pytest.mark.parametrize("levels,k", [("2,4", "2"), ("4,5,6", "3")])
@pytest.mark.parametrize("width", [4, 8])
def test_beamed_engine_check_entries(width, levels, k, monkeypatch, capfd):
    """A small beam at two edits fires before the snapshot (jbeam > 0), so open snapshots put their
    check entries (j + 1 <= jcheck) first; the dedup-free resume paths (lane kernel, live pass) honour
    them."""
    pats, text = _wordy(0xbea3 + width, 120)
    rows, fin, opn, _ = check(monkeypatch, capfd, B().fuzzy(L().edits(2)).beam_width(width), pats, text, 0.6, k, levels)
    assert len(rows) > 0 and opn > 0


def test_unbeamed_two_edit_engine(monkeypatch, capfd):
    """No beam: jcheck == 0 for every key, the check pass is empty wave-wide and skipped."""
    pats, text = _wordy(0x2ed17, 120)
    rows, fin, opn, _ = check(monkeypatch, capfd, B().fuzzy(L().edits(2)), pats, text, 0.6, "4", "5,6")
    assert len(rows) > 0 and opn > 0 and fin > 0


def test_dense_trie_large_snapshots(monkeypatch, capfd):
    """Many patterns sharing 2-3 character prefixes over a 3-letter alphabet: open keys keep many live
    dedup entries (a large nv). No key of it is refused for nv > rc_vmax (the FAC_RC_DEBUG line of
    uncached keys by reason reports 0): that branch shows only at full size (C3: 138 keys per step)."""
    rng = Rng(0xde75e)
    pats = sorted({word(rng, "abc", 5, 8) for _ in range(200)})
    hay = "".join("abc"[rng.next() % 3] for _ in range(2053))
    rows, fin, opn, _ = check(monkeypatch, capfd, B().fuzzy(L().edits(2)), pats, hay, 0.7, "4", "5,6")
    assert len(rows) > 0 and opn > 0


def test_mixed_open_and_final_keys(monkeypatch, capfd):
    """Planted near-matches between filler that matches nothing: one level's build pass holds open and
    final keys side by side in a wave's chunk."""
    rng = Rng(0x313ed)
    pats = [word(rng, "abcdefgh", 5, 9) for _ in range(60)]
    parts = []
    for _ in range(400):
        w = list(pats[rng.next() % len(pats)])
        if rng.next() % 2:
            w[rng.next() % len(w)] = "abcdefgh"[rng.next() % 8]
        parts.append("".join(w))
        parts.append("".join("XYZW "[rng.next() % 5] for _ in range(1 + rng.next() % 9)))
    hay = "".join(parts)[:5501]
    rows, fin, opn, _ = check(monkeypatch, capfd, B().fuzzy(L().edits(2)), pats, hay, 0.7, "4", "5,6")
    assert len(rows) > 0 and fin > 0 and opn > 0
