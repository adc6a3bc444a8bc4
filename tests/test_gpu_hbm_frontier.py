"""The HBM rungs of the frontier ladder (DESIGN.md §5 "HBM rungs"): searches whose beam, fan-out or
frontier no LDS rung holds run with the ring and the dedup table in global memory and return the
CPU oracle's rows (spans, pattern ids, similarity bits, edit counts). The oracle's row counts are
asserted so an empty result cannot pass; the oracle rows of a case are computed once and shared.

FAC_RC_DEBUG prints one `FAC_HBM rung=<vcap>,<qcap> windows=<n> slots=<n>` line per HBM launch;
FAC_HBM_CAP0 picks the first HBM rung tried and FAC_HBM_FRONTIER_MB the scratch budget."""
import functools
import re

import pytest

from fuzzy_aho_corasick import FuzzyAhoCorasickBuilder as B, FuzzyLimits as L, SearchOptions as O, workloads
from fuzzy_aho_corasick.structs import DeviceError
from oracle_harness import OracleEngine
from test_gpu_parity import Rng, rows

pytestmark = pytest.mark.gpu

PATS = ["a" * 12, "ab" * 6, "b" * 12, "ba" * 6]
HAY = "ab" * 20 + "a" * 20 + "b" * 20
HAY_SHORT = "ab" * 6 + "a" * 14 + "b" * 14
CJK = [chr(0x4E00 + i) + "東京" for i in range(5000)]
H2 = "".join(chr(0x4E00 + (i * 37) % 5000) + ("東京" if i % 3 else "東亰") + "。" for i in range(60))
RUNGS = [(1 << 14, 1 << 14), (1 << 17, 1 << 17), (1 << 20, 1 << 20)]
# slots of the oracle's diagnostics histogram (orc_deg_hist): per-window maxima over a search
ORC_MAX_PENDING = 73  # oracle.cpp, the beam check: max(queue.size() - q_idx)
ORC_MAX_KEYS = 74     # oracle.cpp, the end of a window: max(visited.size())


def deep(edits, beam=0):
    b = B().fuzzy(L().edits(edits))
    return b.beam_width(beam) if beam else b


@functools.lru_cache(maxsize=None)
def deep_want(edits, beam=0, hay=HAY):
    return sorted(OracleEngine(deep(edits, beam), PATS).raw_rows(hay, 0.3))


@functools.lru_cache(maxsize=None)
def cjk_case(beamed):
    b = B().fuzzy(L().edits(1))
    pats = CJK
    if beamed:
        b, pats = b.beam_width(16), CJK[:2100]
    return b, pats, sorted(OracleEngine(b, pats).raw_rows(H2, 0.6))


def gpu_rows(builder, pats, hay, thr):
    got, st = builder.build(pats).stage(hay.encode("utf-8")).search_windows(thr)
    return sorted(got), st


def hbm_lines(err):
    """(vcap, qcap, windows, slots) of every FAC_HBM line."""
    return [tuple(int(x) for x in m) for m in re.findall(r"FAC_HBM rung=(\d+),(\d+) windows=(\d+) slots=(\d+)", err)]


def test_wide_beam_that_never_triggers():
    """1. beam_width 3000 needs a ring of more than 6000 states: no LDS rung; 2 x 3000 pending states
    are never reached at edits 6, so the rows are the unbeamed ones."""
    want = deep_want(6, 3000)
    assert len(want) == 1847 and want == deep_want(6)
    got, _ = gpu_rows(deep(6, 3000), PATS, HAY, 0.3)
    assert got == want


@pytest.mark.parametrize("hay,beam,n,n_unbeamed", [
    (HAY, 2100, 2471, 2686), (HAY, 2500, 2617, 2686), (HAY, 3000, 2686, 2686),
    (HAY_SHORT, 2100, 1127, 1146), (HAY_SHORT, 2500, 1133, 1146), (HAY_SHORT, 3000, 1146, 1146)])
def test_wide_beam_that_triggers(hay, beam, n, n_unbeamed):
    """2. edits 8: the selection runs over more than 4096 pending states of a global ring (the beams
    that change the rows are the ones that triggered)."""
    want = deep_want(8, beam, hay)
    assert len(want) == n and len(deep_want(8, 0, hay)) == n_unbeamed
    got, _ = gpu_rows(deep(8, beam), PATS, hay, 0.3)
    assert got == want


def test_wide_root_unbeamed():
    """3. 5000 distinct first graphemes: the root alone pushes 10003 states."""
    b, pats, want = cjk_case(False)
    assert len(want) == 100
    got, _ = gpu_rows(b, pats, H2, 0.6)
    assert got == want


def test_wide_root_beamed():
    """4. 2100 first graphemes behind a beam of 16 (the root's 4203 pushes must fit the ring), staged
    and as a batch of three documents, each searched as a text of its own."""
    b, pats, want = cjk_case(True)
    assert len(want) == 95
    got, _ = gpu_rows(b, pats, H2, 0.6)
    assert got == want
    docs = [H2[:80], H2[80:160], H2[160:]]
    eng, orc = b.build(pats), OracleEngine(b, pats)
    per_doc = eng.search_batch(docs, O().threshold(0.6))
    total = 0
    for doc, ms in zip(docs, per_doc):
        alone = rows(orc.search(doc, O().threshold(0.6)))
        assert rows(ms) == alone, doc
        total += len(alone)
    assert total > 0


@pytest.mark.parametrize("kind", ["beam1000", "auto_beam_count_pass"])
def test_deep_frontier_with_exact_dedup(kind):
    """5. 5706 distinct keys in one window pass the 3584-entry fill limit of the largest LDS table, and
    a search that needs exact dedup (a beam; the auto-beam count pass) may not drop the table."""
    b = deep(6, 1000) if kind == "beam1000" else deep(6).auto_beam(2 ** 64 - 1, 8)
    want = sorted(OracleEngine(b, PATS).raw_rows(HAY, 0.3))
    assert len(want) == 1847
    got, _ = gpu_rows(b, PATS, HAY, 0.3)
    assert got == want


def test_spilled_windows_resume_from_the_prefix_cache(monkeypatch, capfd):
    """A wide beam with a small fan-out starts on the dedup-free first pass, as before the HBM rungs;
    with the prefix cache forced on, the windows it spills keep their snapshot and resume from it on
    the HBM rung (the fenced snapshot load of run_window)."""
    want = deep_want(8, 2100)
    for k, v in {"FAC_RC_MIN": "1", "FAC_RC_K": "4", "FAC_RC_K2": "0", "FAC_RC_DEBUG": "1"}.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    got, st = gpu_rows(deep(8, 2100), PATS, HAY, 0.3)
    err = capfd.readouterr().err
    assert got == want and len(want) == 2471
    assert hbm_lines(err) and st.states_cached > 0, err[-1500:]


def test_mappings():
    """6. The mapping flavour of the HBM kernels."""
    b = B().mapping("ß", "ss").fuzzy(L().edits(1)).beam_width(3000)
    pats, hay = ["strasse", "gross"], "die straße ist groß, die strase ist gros"
    want = sorted(OracleEngine(b, pats).raw_rows(hay, 0.7))
    assert len(want) == 4
    got, _ = gpu_rows(b, pats, hay, 0.7)
    assert got == want


@pytest.mark.parametrize("edits,n", [(6, 1847), (7, 2233), (8, 2686)])
def test_unbeamed_deep_frontier(edits, n):
    """7. Unbeamed windows past the 8192-state dedup-free ring (the commit before the HBM rungs: edits 6
    stayed within it, edits 7 and 8 ended in FAC_E_CAPACITY)."""
    want = deep_want(edits)
    assert len(want) == n
    got, _ = gpu_rows(deep(edits), PATS, HAY, 0.3)
    assert got == want


@functools.lru_cache(maxsize=None)
def larger_case(beamed):
    """Windows the smallest HBM rung cannot hold, by the oracle's own per-window maxima (pending states,
    distinct dedup keys): beamed, edits 10 with beam 2100 on PATS; unbeamed, edits 10 on 16-letter
    patterns. Returns (builder, patterns, oracle rows, max pending, max keys)."""
    import ctypes

    import oracle_harness
    oracle_harness._lib.orc_deg_hist.restype = ctypes.POINTER(ctypes.c_uint64)
    hist = oracle_harness._lib.orc_deg_hist()
    hist[ORC_MAX_PENDING] = hist[ORC_MAX_KEYS] = 0
    b, pats = (deep(10, 2100), PATS) if beamed else (deep(10), ["a" * 16, "ab" * 8, "b" * 16, "ba" * 8])
    want = sorted(OracleEngine(b, pats).raw_rows(HAY, 0.3))
    # (the layout is checked: a window's keys are never fewer than its largest pending count here)
    assert 0 < hist[ORC_MAX_PENDING] < hist[ORC_MAX_KEYS]
    return b, pats, want, int(hist[ORC_MAX_PENDING]), int(hist[ORC_MAX_KEYS])


@pytest.mark.parametrize("beam", [0, 2100])
def test_escalation_between_hbm_rungs(monkeypatch, capfd, beam):
    """8. edits 8 reaches the HBM rungs (unbeamed from the LDS rungs, beam 2100 from its first pass) and
    the smallest rung holds it: the oracle's worst window has 6754 pending states and, beamed, 12983
    distinct keys against the rung's 16384-state ring and 14336-entry fill limit. So the escalation from
    one HBM rung to the next is shown on a larger case, and FAC_HBM_CAP0 moves the first rung tried."""
    b, pats, want_big, max_pending, max_keys = larger_case(beam != 0)
    # before the GPU is touched: the smallest rung must overflow -- an exact-dedup table past its fill
    # limit; an unbeamed ring (never shorter than the oracle's fully deduplicated queue, §3) past its size
    assert max_keys > RUNGS[0][0] - RUNGS[0][0] // 8 if beam else max_pending > RUNGS[0][1]
    assert len(want_big) == (2908 if beam else 3140)
    monkeypatch.setenv("FAC_RC_DEBUG", "1")
    capfd.readouterr()
    got, st = gpu_rows(b, pats, HAY, 0.3)
    lines = hbm_lines(capfd.readouterr().err)
    assert got == want_big
    assert len({ln[:2] for ln in lines}) >= 2, lines
    assert [ln[:2] for ln in lines] == sorted(ln[:2] for ln in lines) and lines[0][:2] == RUNGS[0], lines
    assert all(x[2] >= y[2] for x, y in zip(lines, lines[1:])), lines  # only the spilled windows move on
    assert st.retries >= len(lines) - 1
    want = deep_want(8, beam)
    capfd.readouterr()
    got, _ = gpu_rows(deep(8, beam), PATS, HAY, 0.3)
    lines = hbm_lines(capfd.readouterr().err)
    assert got == want and lines and {ln[:2] for ln in lines} == {RUNGS[0]}, lines
    monkeypatch.setenv("FAC_HBM_CAP0", "131072")
    capfd.readouterr()
    got, _ = gpu_rows(deep(8, beam), PATS, HAY, 0.3)
    lines = hbm_lines(capfd.readouterr().err)
    assert got == want
    assert lines and lines[0][:2] == RUNGS[1] and all(ln[:2] != RUNGS[0] for ln in lines), lines
    monkeypatch.setenv("FAC_HBM_CAP0", "20000")  # not a rung size: the smallest rung that holds as many
    capfd.readouterr()
    got, _ = gpu_rows(deep(8, beam), PATS, HAY, 0.3)
    lines = hbm_lines(capfd.readouterr().err)
    assert got == want and lines and lines[0][:2] == RUNGS[1], lines


def test_budget(monkeypatch, capfd):
    """9. FAC_HBM_FRONTIER_MB bounds the scratch: 1 MiB holds two unbeamed slots of the smallest rung
    (512 KiB each) and the rows stay the same; a budget below one slot of the needed rung is
    FAC_E_CAPACITY, decided on the host before any launch, never a partial result."""
    b, pats, want = cjk_case(False)
    monkeypatch.setenv("FAC_RC_DEBUG", "1")
    capfd.readouterr()
    gpu_rows(b, pats, H2, 0.6)
    free = hbm_lines(capfd.readouterr().err)
    assert free and all(ln[:2] == RUNGS[0] and ln[3] > 2 for ln in free), free
    monkeypatch.setenv("FAC_HBM_FRONTIER_MB", "1")
    capfd.readouterr()
    got, _ = gpu_rows(b, pats, H2, 0.6)
    lines = hbm_lines(capfd.readouterr().err)
    assert got == want
    assert lines and all(ln[:2] == RUNGS[0] and 1 <= ln[3] <= 2 for ln in lines), lines
    monkeypatch.setenv("FAC_HBM_CAP0", "131072")  # one slot of that rung is 4 MiB
    with pytest.raises(DeviceError) as ei:
        gpu_rows(b, pats, H2, 0.6)
    assert ei.value.code == 105
    assert "HBM frontier budget is 1 MiB" in str(ei.value) and "131072 states" in str(ei.value), str(ei.value)
    monkeypatch.delenv("FAC_HBM_CAP0")
    bb, bpats, _ = cjk_case(True)  # beamed: the selection's scratch doubles the slot, past 1 MiB
    with pytest.raises(DeviceError) as ei:
        gpu_rows(bb, bpats, H2, 0.6)
    assert ei.value.code == 105 and "16384 states" in str(ei.value), str(ei.value)


@pytest.mark.parametrize("limit,lens,bw", [
    # core's 16 partition rounds; lengths around the 4096-state LDS limit of the mask words, around
    # 32768 (median3_rec 4 levels deep: 81 leaf triples) and 262144 (5 levels: 243)
    (16, [4097, 6000, 32767, 32768, 40000, 100001, 262143, 262144, 300000], 2000),
    (16, [8193, 70000, 131072, 1 << 20], 4096),
    # median_of_medians after one round, or at once (one lane, sequential: short arrays)
    (1, [4097, 5000, 6001], 1000), (0, [4097, 4500], 1000)])
def test_beam_select_on_a_global_ring(limit, lens, bw):
    """The beam cut alone over a ring in global memory, as the HBM rungs run it, at pending counts no
    search in this file reaches: the bw survivors and their order are the oracle's
    select_nth_unstable_by (test_device_beam_select_matches_oracle does the same for the LDS rings)."""
    import numpy as np
    import oracle_harness as OH
    from fuzzy_aho_corasick import _native
    from test_rust_select import _BEAM_COSTS, _orc_select_batch, _selection_violations

    rng = np.random.default_rng(4242 + limit + len(lens))
    offs = np.zeros(len(lens) + 1, np.uint64)
    offs[1:] = np.cumsum(lens)
    n = int(offs[-1])
    terms = rng.integers(1, 9, size=n)  # penalties of 1..8 edits: many ties, many distinct values
    k = rng.integers(0, len(_BEAM_COSTS), size=(n, 8))
    keys = np.where(np.arange(8)[None, :] < terms[:, None], _BEAM_COSTS[k], np.float32(0)).sum(axis=1, dtype=np.float32)
    keys[int(offs[1]):int(offs[2])] = _BEAM_COSTS[k[int(offs[1]):int(offs[2]), 0]]  # one array of six values
    index = np.full(len(lens), bw - 1, np.uint64)
    OH.set_modes(sel_limit=limit)
    try:
        want, bad = _orc_select_batch(keys, offs, index)
    finally:
        OH.set_modes(sel_limit=16)
    assert bad == 0 and _selection_violations(keys, offs, index, want) == 0
    perm = np.zeros(len(lens) * bw, np.uint32)
    rc = _native.lib.fac_diag_beam_select(keys.ctypes.data, offs.ctypes.data, len(lens), bw, 2, limit, perm.ctypes.data)
    assert rc == 0, _native.last_error()
    exp = np.concatenate([want[int(offs[a]):int(offs[a]) + bw] for a in range(len(lens))])
    diff = np.nonzero(perm != exp)[0]
    assert len(diff) == 0, f"arrays {sorted(set((diff // bw).tolist()))} of lengths {lens} differ"


# fac_stats of the commit before the HBM rungs, from a run of that commit on an MI355X:
# (retries, kernel_launches)
# (profiles/hbm_frontier/probe_stats.py -> stats_parent.json)
PARENT_STATS = {"unbeamed": (0, 1), "beamed": (1, 2), "c3": (3, 4), "wide_beam": (0, 1)}


def test_engines_that_fit_the_lds_rungs_are_unmoved(monkeypatch, capfd):
    """10. test_every_frontier_variant's two engines and test_frontier_spill_beamed's C3 slice never
    reach an HBM rung and launch exactly what they launched before. So does an engine whose beam no
    table rung holds (3000) but whose windows stay small: before the HBM rungs its dedup-free first
    pass finished them all, and it still does."""
    rng = Rng(0xabcdef)
    words = ["needle", "haystack", "fuzzy", "automaton", "école", "Москва"]
    text = " ".join(words[rng.next() % 6][: 3 + rng.next() % 6] + "xyzé"[rng.next() % 4] for _ in range(600))
    w = workloads.config("c3", 24 << 10, 3)
    cases = [("unbeamed", B().fuzzy(L().edits(2)), words, text, 0.6),
             ("beamed", B().fuzzy(L().edits(2)).beam_width(8).case_insensitive(True), words, text, 0.6),
             ("wide_beam", B().fuzzy(L().edits(1)).beam_width(3000), words, text, 0.6),
             ("c3", workloads.builder_for(w), w.patterns, w.haystack.decode("utf-8"), w.threshold)]
    monkeypatch.setenv("FAC_RC_DEBUG", "1")
    for name, b, pats, hay, thr in cases:
        want = sorted(OracleEngine(b, pats).raw_rows(hay, thr))
        capfd.readouterr()
        got, st = gpu_rows(b, pats, hay, thr)
        err = capfd.readouterr().err
        assert got == want and len(want) > 0, name
        assert "FAC_HBM" not in err, (name, hbm_lines(err))
        assert (st.retries, st.kernel_launches) == PARENT_STATS[name], name
