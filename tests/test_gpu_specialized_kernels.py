"""The plain-engine instances of the window kernels (CfPlain, DESIGN.md §5 *Specialised instances*):
rc_build_kernel_plain (rings 256 and 512), bfs_window_kernel_live_plain and bfs_window_kernel_plain (<512, 256>) are compiled
with the flag-like launch constants of the plain engine folded in; every other engine, variant or knob
takes the generic instances of the same source -- so do the lane kernel and the unbeamed engines'
<0, 512> variant, whose plain instances were measured and dropped. Tiny haystacks with the
prefix cache forced on run the builds, the lookups, the lane kernel, the dedup-free pass and the exact
re-run of spilled windows.

Every case reads the launcher's FAC_INSTANCE lines (FAC_RC_DEBUG=launch: the host's lines without the
device counters, which would make the run a diagnostics run) to see that the instance it is meant for
really ran, and compares the records with the CPU oracle and with the same search under
FAC_NO_SPECIALIZE=1, whose states_popped / states_cached / lane_windows must be equal too. With
FAC_NO_SPECIALIZE=1 exported the whole file runs on the generic instances."""
import os
import re

import pytest

from fuzzy_aho_corasick import FuzzyAhoCorasickBuilder as B, FuzzyLimits as L, Pattern, Similarity
from oracle_harness import OracleEngine
from test_gpu_build_epilogue import RC_KNOBS, Rng, _wordy, word

pytestmark = pytest.mark.gpu

FORCED_GENERIC = os.environ.get("FAC_NO_SPECIALIZE") == "1"
BUILD, LIVE, DEDUP, ND, LANE = ("rc_build_kernel<256>", "bfs_window_kernel_live<256>", "bfs_window_kernel<512,256>",
                                "bfs_window_kernel_nd<512>", "lane_window_kernel<12,8>")
BUILD512 = "rc_build_kernel<512>"  # the builds of unbeamed engines (a ring as large as their main pass's)
HOT = {BUILD, BUILD512, LIVE, DEDUP}  # the launches that have a plain instance
DIAG_KNOBS = ("FAC_NO_RC", "FAC_RC_FULL_SWEEP", "FAC_RC_DEBUG", "FAC_DUP_CUT", "FAC_BEAM_CANONICAL", "FAC_LIVE_NQMAX")


def instances(err):
    """kernel -> set of instances its launches used, from the FAC_INSTANCE lines"""
    seen = {}
    for kernel, inst in re.findall(r"^FAC_INSTANCE kernel=(\S+) instance=(\S+)$", err, re.M):
        seen.setdefault(kernel, set()).add(inst)
    return seen


def check(monkeypatch, capfd, builder, pats, hay, thr, k, levels, plain, must_launch, env=None, parts=1):
    """Records == oracle == FAC_NO_SPECIALIZE=1 run, equal pop statistics, and the launches of the
    kernels in `plain` (True: all of HOT, False: none) used the plain instance, every other launch the
    generic one; must_launch: kernels the case is meant to run. parts > 1: the union over
    set_key_partition(parts, r). Returns (records, stats, kernel -> instances)."""
    plain = HOT if plain is True else (plain or set())
    for name in RC_KNOBS + DIAG_KNOBS:
        monkeypatch.delenv(name, raising=False)
    eng = builder.build(pats)
    data = hay.encode("utf-8")
    for name, v in (("FAC_RC_MIN", "1"), ("FAC_RC_MIN2", "1"), ("FAC_RC_STRIDE2", "1"), ("FAC_RC_T2", "1"),
                    ("FAC_RC_K", k), ("FAC_RC_LEVELS", levels)) + tuple((env or {}).items()):
        monkeypatch.setenv(name, v)

    def run():
        got, stats = [], []
        for r in range(parts):
            staged = eng.stage(data)
            if parts > 1:
                staged.set_key_partition(parts, r)
            rows, st = staged.search_windows(thr)
            got += rows
            stats.append((st.states_popped, st.states_cached, st.lane_windows))
        return sorted(got), stats

    monkeypatch.setenv("FAC_RC_DEBUG", "launch")
    capfd.readouterr()
    new, st_new = run()
    seen = instances(capfd.readouterr().err)
    with monkeypatch.context() as m:
        m.setenv("FAC_NO_SPECIALIZE", "1")
        old, st_old = run()
        seen_old = instances(capfd.readouterr().err)
    want = sorted(OracleEngine(builder, pats).raw_rows(hay, thr))
    print(f"k={k} levels={levels} records={len(want)} (popped, cached, lane)={st_new} launches={seen}")
    assert new == want
    assert old == want
    assert st_new == st_old
    assert all(v == {"generic"} for v in seen_old.values()), seen_old
    assert set(must_launch) <= set(seen), (must_launch, seen)
    for kernel, used in seen.items():
        assert used == ({"plain"} if kernel in plain and not FORCED_GENERIC else {"generic"}), (kernel, used)
    assert seen
    return want, st_new, seen


@pytest.mark.parametrize("width", [4, 8, 64])
@pytest.mark.parametrize("edits", [1, 2])
def test_beamed_plain_engine(edits, width, monkeypatch, capfd):
    """Beamed engines at one and two edits: builds, lane kernel and dedup-free pass on the plain
    instances; a small beam at two edits triggers inside windows, which spill into <512, 256>."""
    pats, text = _wordy(0xbea3 + width, 120)
    must = [BUILD, LANE, LIVE] + ([DEDUP] if edits == 2 and width <= 8 else [])
    rows, _, _ = check(monkeypatch, capfd, B().fuzzy(L().edits(edits)).beam_width(width), pats, text, 0.6, "2", "2,4",
                       True, must)
    assert len(rows) > 0


@pytest.mark.parametrize("edits", [1, 2])
def test_unbeamed_plain_engine(edits, monkeypatch, capfd):
    """No beam: the builds take the plain rc_build_kernel<512> (a ring as large as the main pass's); the
    main pass is the dedup-free <0, 512> variant, which has no plain instance."""
    pats, text = _wordy(0x2ed17, 120)
    rows, _, _ = check(monkeypatch, capfd, B().fuzzy(L().edits(edits)), pats, text, 0.6, "4", "5,6", True,
                       [BUILD512, LANE, ND])
    assert len(rows) > 0


@pytest.mark.parametrize("width", [0, 8])
def test_case_insensitive_unicode_haystack(width, monkeypatch, capfd):
    """A non-ASCII haystack (text32) searched case-insensitively: case folding and the text's encoding
    stay run-time in the plain instances."""
    rng = Rng(0x0c1 + width)
    alphabet = "abcdeéñωмΣ"
    stems = [word(rng, alphabet, 3, 4) for _ in range(10)]
    pats = sorted({stems[rng.next() % 10] + word(rng, alphabet, 2, 5) for _ in range(80)})
    parts = []
    for _ in range(450):
        w = pats[rng.next() % len(pats)][: 3 + rng.next() % 7]
        parts.append(w.upper() if rng.next() % 3 == 0 else w)
        parts.append(" xÉ"[rng.next() % 3])
    hay = "".join(parts)[:4801]
    assert not hay.isascii()
    b = B().fuzzy(L().edits(2)).case_insensitive(True)
    if width:
        b = b.beam_width(width)
    must = [LANE, LIVE, BUILD] if width else [LANE, ND, BUILD512]
    rows, _, _ = check(monkeypatch, capfd, b, pats, hay, 0.6, "2", "2,4", True, must)
    assert len(rows) > 0


def test_every_key_final(monkeypatch, capfd):
    """A haystack over characters no pattern contains: every window dies inside its key, so the plain
    build settles nothing but final keys (the key-end tests are compile-time true in it)."""
    rng = Rng(0xf17a1 + 2)
    pats = [word(rng, "abcdefgh", 6, 10) for _ in range(40)] + ["q"]
    hay = "".join("XYZW0123"[rng.next() % 8] for _ in range(4099))
    rows, _, _ = check(monkeypatch, capfd, B().fuzzy(L().edits(2)).beam_width(8), pats, hay, 0.8, "4", "5,6", True,
                       [BUILD])
    assert rows == []


def test_mixed_open_and_final_keys(monkeypatch, capfd):
    """Planted near-matches between filler that matches nothing: open and final keys side by side in a
    wave's chunk of the plain build."""
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
    rows, _, _ = check(monkeypatch, capfd, B().fuzzy(L().edits(2)).beam_width(8), pats, hay, 0.7, "4", "5,6", True,
                       [BUILD, LIVE])
    assert len(rows) > 0


# ---- engines and knobs that must stay on the generic instances

def test_generic_pattern_limits(monkeypatch, capfd):
    """Per-pattern limits: the limits path (mef == 255) is not the plain engine's edit model."""
    pats, text = _wordy(0x11317, 80)
    lim = [Pattern(p).fuzzy(L().edits(1 + i % 2)) for i, p in enumerate(pats)]
    rows, _, _ = check(monkeypatch, capfd, B().beam_width(8), lim, text, 0.6, "2", "2,4", False, [BUILD, LIVE])
    assert len(rows) > 0


def test_generic_non_ascii_similarity_pair(monkeypatch, capfd):
    """A similarity pair beyond ASCII (n_sim > 0): the binary search behind the ASCII table stays."""
    rng = Rng(0x51a1)
    alphabet = "abcdeéè"
    pats = sorted({word(rng, alphabet, 4, 8) for _ in range(80)})
    hay = " ".join(pats[rng.next() % len(pats)].replace("é", "è") if rng.next() % 2 else word(rng, alphabet, 2, 6)
                   for _ in range(600))[:4507]
    sim = Similarity.from_map({("é", "è"): 0.8, ("a", "e"): 0.5})
    rows, _, _ = check(monkeypatch, capfd, B().fuzzy(L().edits(2)).similarity(sim).beam_width(8), pats, hay, 0.6, "2",
                       "2,4", False, [BUILD, LIVE])
    assert len(rows) > 0


def test_generic_auto_beam(monkeypatch, capfd):
    """An auto-beam engine. Its counting pass (unbeamed, exact dedup, every window's queue length into
    win_counts) must stay on generic kernels: its builds are rc_build_kernel<512>, which has a plain
    twin, so this is the case that holds plain_params()'s !win_counts clause. The windows behind the
    switch are an ordinary beamed pass of a plain engine and take the plain instances."""
    pats, text = _wordy(0xab40, 100)
    rows, _, seen = check(monkeypatch, capfd, B().fuzzy(L().edits(2)).auto_beam(40, 8), pats, text, 0.6, "4", "5",
                          HOT - {BUILD512}, ["bfs_window_kernel<512,512>", BUILD512])
    assert len(rows) > 0


def test_generic_key_partition(monkeypatch, capfd):
    """set_key_partition(2, r): each part on the generic instances, the union equal to the whole."""
    pats, text = _wordy(0x4e9, 120)
    rows, _, _ = check(monkeypatch, capfd, B().fuzzy(L().edits(2)).beam_width(8), pats, text, 0.6, "2", "2,4", False,
                       [BUILD, LIVE], parts=2)
    assert len(rows) > 0


def test_generic_dup_cut(monkeypatch, capfd):
    """FAC_DUP_CUT=1 is a diagnostics knob: the run takes the generic instances, which hold its code."""
    pats, text = _wordy(0xbea3 + 4, 120)
    rows, _, _ = check(monkeypatch, capfd, B().fuzzy(L().edits(2)).beam_width(4), pats, text, 0.6, "2", "2,4", False,
                       [BUILD, LIVE], env={"FAC_DUP_CUT": "1"})
    assert len(rows) > 0
