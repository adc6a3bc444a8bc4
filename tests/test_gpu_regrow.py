"""The whole-pass re-runs of the search launcher (launch_pass, DESIGN.md §5 "Whole-pass re-runs") at
small shapes. A pass is run again when a wave's per-window best list (ERR_EMIT), the spill list
(ERR_SPILL) or the record buffer overflowed; the diagnostics knobs FAC_ECAP0, FAC_SPILL_CAP0 and
FAC_OUT_CAP0 shrink the three first sizes so a few thousand windows reach each branch. Every case
compares the forced run bit-exactly with the CPU oracle (spans, pattern ids, similarity bits, edit
counts) and with the same staged object without the knob, asserts from the oracle's own output --
before the GPU is touched -- that the input must overflow the shrunken buffer, and checks that
fac_stats.retries counts the re-runs."""
import functools
import re
from collections import Counter

import pytest

from fuzzy_aho_corasick import (FuzzyAhoCorasickBuilder as B, FuzzyLimits as L, Order, Overlap, ReplacementTable,
                                SearchOptions as O, StagedBatch, batch_offsets)
from oracle_harness import OracleEngine
from test_gpu_parity import (ASCII_FILLER, ASCII_VOCAB, ASTRAL_FILLER, ASTRAL_VOCAB, UNI_FILLER, UNI_VOCAB, Rng,
                             _staged_vs_oracle, random_case, rows)

pytestmark = pytest.mark.gpu

OUT, ECAP, SPILL = "FAC_OUT_CAP0", "FAC_ECAP0", "FAC_SPILL_CAP0"
WORDS = ["needle", "haystack", "fuzzy", "automaton"]
CACHE = {
    "off": {"FAC_NO_RC": "1"},
    "k4": {"FAC_RC_MIN": "1", "FAC_RC_K": "4", "FAC_RC_K2": "0"},
    "k2+k4": {"FAC_RC_MIN": "1", "FAC_RC_K": "2", "FAC_RC_K2": "4", "FAC_RC_MIN2": "1", "FAC_RC_STRIDE2": "1",
              "FAC_RC_T2": "1"},
}
# the start level's dense bitmaps kept and their window list taken at any share of finished windows
DENSE = {"FAC_RC_MIN": "1", "FAC_RC_MIN2": "1", "FAC_RC_DENSE_OFF": "0", "FAC_RC_DENSE_LIST": "0"}
C2_BYTES = (16 << 10) + 500
# with the dense list: the spill list from the smallest ring
DENSE_EXTRA = {"FAC_SPILL_CAP0": {"FAC_VARIANT": "0,128"}}


def ecap_steps(keys, cap0):
    """x8 growth steps of a best list of cap0 entries until it holds `keys` entries."""
    steps = 0
    while cap0 < keys:
        cap0 *= 8
        steps += 1
    return steps


def max_keys(want):
    """The largest number of records of one window: a window's records share their start, so these are
    its distinct (end, pattern) keys, the entries of its best list."""
    return max(Counter(r[0] for r in want).values())


@functools.lru_cache(maxsize=None)
def long_case(beamed):
    """test_long_haystack_windows's haystack cut to 2500 words (18 K windows, under 4096 records: the
    default record buffer holds them), edits 1, unbeamed or beam 8."""
    rng = Rng(77)
    text = " ".join(WORDS[rng.next() % 4][: 3 + rng.next() % 6] + "xyz"[rng.next() % 3] for _ in range(2500))
    b = B().fuzzy(L().edits(1))
    if beamed:
        b = b.beam_width(8)
    return b, WORDS, text, 0.7, sorted(OracleEngine(b, WORDS).raw_rows(text, 0.7))


@functools.lru_cache(maxsize=None)
def spill_case(beamed):
    """test_frontier_spill_unbeamed / _beamed: runs of one letter against one-letter patterns."""
    rng = Rng(5)
    hay = "".join("aaaaaaaaaaaaaaaa" if rng.next() % 3 else "ab" for _ in range(40))
    pats = ["aaaaaaaaaa", "aaaab", "baaaaaaaa"]
    b = B().fuzzy(L().edits(3))
    if beamed:
        b = b.beam_width(64)
    return b, pats, hay, 0.5, sorted(OracleEngine(b, pats).raw_rows(hay, 0.5))


@functools.lru_cache(maxsize=None)
def deep_case():
    """test_frontier_beyond_2048_states, unbeamed: windows that climb the whole variant ladder."""
    pats = ["a" * 12, "ab" * 6, "b" * 12, "ba" * 6]
    hay = "ab" * 20 + "a" * 20 + "b" * 20
    b = B().fuzzy(L().edits(5))
    return b, pats, hay, 0.3, sorted(OracleEngine(b, pats).raw_rows(hay, 0.3))


@functools.lru_cache(maxsize=None)
def c2_case():
    """A C2-shaped slice (1 K ASCII patterns, edits 1) of C2_BYTES bytes with 100 bytes of spill_case's
    letter runs in its middle and its three patterns added with a limit of 3 edits of their own, at
    threshold 0.6: the C2 words keep the start level's dense bitmaps and their window list (with 2
    edits for every pattern no 5-char key is final, and no window is left out), the runs' windows pop
    over 512 states and hold up to 18 keys, more than a lane's own best list (8). Also returns the
    runs' window range."""
    from fuzzy_aho_corasick import Pattern, workloads
    w = workloads.config("c2", C2_BYTES, 7)
    b = workloads.builder_for(w)
    text, runs = w.haystack.decode("utf-8"), spill_case(False)[2][:100]
    cut = text.index(" ", len(text) // 2)
    hay = text[:cut] + " " + runs + text[cut:]
    pats = list(w.patterns) + [Pattern(p).fuzzy(L().edits(3)) for p in spill_case(False)[1]]
    return b, pats, hay, 0.6, sorted(OracleEngine(b, pats).raw_rows(hay, 0.6)), (cut + 1, cut + 1 + len(runs))


def window_pops(b, pats, hay, thr, upto=None, begin=0):
    """States the oracle pops in each of the windows [begin, upto) of an ASCII haystack (window = byte)."""
    orc = OracleEngine(b, pats)
    pops = []
    for w in range(begin, len(hay) if upto is None else upto):
        orc.raw_rows(hay, thr, windows=(w, w + 1))
        pops.append(orc.states_popped)
    return pops


def windows_popping_over(b, pats, hay, thr, limit):
    """Windows whose search pops more than `limit` states in the oracle. An unbeamed window pops every
    state it ever holds pending, so only these can overflow a ring of `limit` states."""
    return sum(p > limit for p in window_pops(b, pats, hay, thr))


def search(staged, thr, monkeypatch, env):
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        got, st = staged.search_windows(thr)
    return sorted(got), st


def forced_vs_base(staged, thr, monkeypatch, env, knobs, want):
    """Records of the run with `knobs` == the same staged object's without == the oracle's."""
    base, st0 = search(staged, thr, monkeypatch, env)
    assert base == want
    got, st = search(staged, thr, monkeypatch, dict(env, **{k: str(v) for k, v in knobs.items()}))
    assert got == base
    return st0, st


@pytest.mark.parametrize("case", ["out=1", "out=n", "out=n-1", "ecap=1", "ecap=2"])
@pytest.mark.parametrize("beamed", [False, True], ids=["unbeamed", "beam8"])
def test_record_buffer_and_best_list_cache_off(beamed, case, monkeypatch):
    """The record buffer and the best lists alone, every window searched from the root. A record
    buffer of exactly the oracle's record count is no overflow (retries as unforced); one record less
    is, in the pass that holds every record. The beamed engine runs its exact variant here
    (FAC_NO_BEAM_BAIL), so its first pass holds every record too."""
    b, pats, text, thr, want = long_case(beamed)
    n, kmax = len(want), max_keys(want)
    assert 100 < n < 4096 and kmax > 2  # the default buffers (4096 records, 1024 entries) never overflow
    env = dict(CACHE["off"], FAC_NO_BEAM_BAIL="1")
    staged = b.build(pats).stage(text.encode())
    if case.startswith("out"):
        cap = {"out=1": 1, "out=n": n, "out=n-1": n - 1}[case]
        st0, st = forced_vs_base(staged, thr, monkeypatch, env, {OUT: cap}, want)
        assert st0.retries == 0  # one pass: it emits all n records
        assert st.retries == (0 if cap == n else 1)  # the buffer grows to the count at once
    else:
        cap = int(case[-1])
        st0, st = forced_vs_base(staged, thr, monkeypatch, env, {ECAP: cap}, want)
        assert st.retries >= st0.retries + ecap_steps(kmax, cap) >= 1


@pytest.mark.parametrize("knob", [OUT, ECAP])
def test_beamed_dedup_free_first_pass_reruns(knob, monkeypatch):
    """The default beamed path (dedup-free first pass, spilled windows re-run on the dedup variants)
    with one-entry buffers: a re-run of the first pass spills the same windows again. A window spills
    there once it holds more than 2 x 8 states pending, so the windows that pop no more than 16 states
    in all without a beam (oracle, first 2000 windows; unbeamed, every pending state is popped) finish
    in the first pass: their records overflow it."""
    b, pats, text, thr, want = long_case(True)
    pops = window_pops(long_case(False)[0], pats, text, thr, upto=2000)
    light = [r for r in want if r[0] < len(pops) and pops[r[0]] <= 16]
    assert len(light) > 1 and max_keys(light) > 1
    staged = b.build(pats).stage(text.encode())
    st0, st = forced_vs_base(staged, thr, monkeypatch, CACHE["off"], {knob: 1}, want)
    assert st.retries >= st0.retries + (1 if knob == OUT else ecap_steps(max_keys(light), 1))


@pytest.mark.parametrize("beamed", [False, True], ids=["unbeamed", "beam64"])
def test_spill_list_regrow_cache_off(beamed, monkeypatch):
    """A one-entry spill list under inputs that spill many windows: the first pass is run again with
    a list of the spilled count, then the ladder goes on as unforced (one retry more)."""
    b, pats, hay, thr, want = spill_case(beamed)
    assert len(want) > 0
    if not beamed:  # the unbeamed first variant's ring holds 512 states
        assert windows_popping_over(b, pats, hay, thr, 512) >= 2
    staged = b.build(pats).stage(hay.encode())
    st0, st = forced_vs_base(staged, thr, monkeypatch, CACHE["off"], {SPILL: 1}, want)
    assert st0.retries > 0 and st.retries >= st0.retries + 1


@pytest.mark.parametrize("knob", [SPILL, OUT, ECAP])
def test_rerun_with_escalations(knob, monkeypatch):
    """Windows that climb the ladder from its smallest variant (FAC_VARIANT=0,128; oracle: up to 3038
    distinct states), so several passes run from a spill list (the d_list / d_spill swap) and the later
    ones hold most records: with one-entry buffers the re-runs happen in list-driven passes as well.
    The spill list itself can only regrow in the first pass -- a later pass runs at most the windows
    the list already held -- and the swapped buffers must survive that regrow."""
    b, pats, hay, thr, want = deep_case()
    kmax = max_keys(want)
    assert len(want) > 1 and kmax > 1
    assert windows_popping_over(b, pats, hay, thr, 2048) >= 2  # still spilling two escalations on
    env = dict(CACHE["off"], FAC_VARIANT="0,128")
    staged = b.build(pats).stage(hay.encode())
    st0, st = forced_vs_base(staged, thr, monkeypatch, env, {knob: 1}, want)
    assert st0.retries >= 2
    assert st.retries >= st0.retries + (ecap_steps(kmax, 1) if knob == ECAP else 1)


@pytest.mark.parametrize("lane", [True, False], ids=["lane", "no-lane"])
@pytest.mark.parametrize("levels", ["k4", "k2+k4"])
def test_each_branch_prefix_cache_on(levels, lane, monkeypatch):
    """Each branch with the prefix cache forced on (one and two levels), the lane kernel on and off: a
    re-run repeats the lookups, the lane kernel and the flushes of finished windows. With FAC_ECAP0=1
    the cache builds overflow too and refuse those keys (they stay uncached). The lane kernel keeps
    best lists of 8 entries of its own, so with it on only windows of more keys must reach a wave's
    list: long_case (3 keys a window) with the lane kernel on is a records-only check for FAC_ECAP0,
    spill_case (19 keys) forces the re-runs either way."""
    env = dict(CACHE[levels])
    if not lane:
        env["FAC_NO_LANE"] = "1"
    for beamed in (False, True):
        b, pats, text, thr, want = long_case(beamed)
        kmax = max_keys(want)
        assert len(want) > 1 and kmax > 1
        staged = b.build(pats).stage(text.encode())
        st0, st = forced_vs_base(staged, thr, monkeypatch, env, {OUT: 1}, want)
        assert st.retries >= 1 and st0.states_cached > 0
        st0, st = forced_vs_base(staged, thr, monkeypatch, env, {ECAP: 1}, want)
        if not lane:
            assert st.retries >= st0.retries + ecap_steps(kmax, 1)
        b, pats, hay, thr, want = spill_case(beamed)
        assert len(want) > 0
        staged = b.build(pats).stage(hay.encode())
        st0, st = forced_vs_base(staged, thr, monkeypatch, env, {SPILL: 1}, want)
        assert st0.retries > 0 and st.retries >= st0.retries + 1
        kmax = max_keys(want)
        assert kmax > 8  # more keys than a lane's list holds: a wave's list must grow to them
        st0, st = forced_vs_base(staged, thr, monkeypatch, env, {ECAP: 1}, want)
        assert st.retries >= st0.retries + ecap_steps(kmax, 1)


def _dense_run(staged, thr, monkeypatch, capfd, env):
    """Sorted rows, stats and the `unlisted` count of every lookup of the run (FAC_RC_DEBUG)."""
    capfd.readouterr()
    got, st = search(staged, thr, monkeypatch, dict(env, FAC_RC_DEBUG="1"))
    err = capfd.readouterr().err
    return got, st, [int(u) for u in re.findall(r"dense-final \d+ unlisted (\d+)", err)]


@pytest.mark.parametrize("knob", [OUT, ECAP, SPILL])
def test_dense_window_list_survives_a_rerun(knob, monkeypatch, capfd):
    """The lookups' dense window list (dl_*_kernel), taken at any share of finished windows, under
    each forced re-run: a re-run builds the list again from every window, not from the previous list.
    The input is c2_case: a C2-shaped slice of 16 KiB + 500 bytes (on the plain slice the list forms
    from 8 KiB on, 30 windows left out there, and at 4 KiB no cache is built; this size spans five
    list blocks with a partial last one) with letter runs of heavier windows. The list must have
    formed (unlisted > 0 in the FAC_RC_DEBUG line of every lookup), the forced run looks up at least
    twice, and every lookup leaves the same windows out (each counted once). Records == the oracle
    == the bitmaps off == the list off. A window of 18 keys fits neither a lane's own list (8) nor
    a snapshot of the cache built with one-entry lists, so a wave's list must grow to it (two x8
    steps). The spill-list case starts on the (0, 128) ring, which the runs' windows (over 128 states
    popped in the oracle) overflow."""
    b, pats, hay, thr, want, (r0, r1) = c2_case()
    kmax = max_keys(want)
    assert 1 < len(want) < 4096 and kmax > 8  # the default record buffer holds them: no unforced regrow
    reruns = ecap_steps(kmax, 1) if knob == ECAP else 1
    env = dict(DENSE, **DENSE_EXTRA.get(knob, {}))
    if knob == SPILL:
        assert sum(p > 128 for p in window_pops(b, pats, hay, thr, upto=r1, begin=r0)) >= 2
    staged = b.build(pats).stage(hay.encode())
    base, st0, un0 = _dense_run(staged, thr, monkeypatch, capfd, env)
    assert base == want
    assert un0 and un0[0] > 0, un0
    got, st, un = _dense_run(staged, thr, monkeypatch, capfd, dict(env, **{knob: "1"}))
    assert got == want
    assert len(un) >= 2 and set(un) == {un0[0]}, (un0, un)
    assert st.retries >= st0.retries + reruns >= 1
    if knob == SPILL:
        assert st0.retries > 0
    for off in ("FAC_RC_NO_DENSE", "FAC_RC_NO_DENSE_LIST"):
        assert search(staged, thr, monkeypatch, dict(env, **{off: "1", knob: "1"}))[0] == want


@pytest.mark.parametrize("cache", ["off", "k4", "dense"])
def test_key_parts(cache, monkeypatch, capfd):
    """Key parts (set_key_partition) under each forced re-run: the part's own window list is the
    pass's source list and must be the same in the re-run -- walked directly (cache off), by the
    lookups (cache on), or as the source of the dense list, where both lists meet (c2_case, the spill
    list from the (0, 128) ring as in the dense-list test: every knob forces a re-run in some part). The parts' union == the oracle and each part's records ==
    that part's without the knob. With the dense list on, the list must have formed in the parts'
    forced runs too, leaving the same windows out in every lookup of a run. With the cache and the
    lane kernel on, long_case's windows (3 keys) fit a lane's own list: records only for FAC_ECAP0."""
    inputs = [c2_case()[:5]] if cache == "dense" else [long_case(False), spill_case(False)]
    env = DENSE if cache == "dense" else CACHE[cache]
    for b, pats, hay, thr, want in inputs:
        assert len(want) > 1
        spills = hay != long_case(False)[2]
        eng = b.build(pats)
        for parts in (2, 3):
            union, forced, unlisted = [], Counter(), 0
            for part in range(parts):
                staged = eng.stage(hay.encode()).set_key_partition(parts, part)
                base, st0 = search(staged, thr, monkeypatch, env)
                union += base
                for knob in (OUT, ECAP, SPILL):
                    kenv, st1 = env, st0
                    if cache == "dense" and knob in DENSE_EXTRA:
                        kenv = dict(env, **DENSE_EXTRA[knob])
                        got, st1 = search(staged, thr, monkeypatch, kenv)
                        assert got == base, (parts, part, knob)
                    got, st = search(staged, thr, monkeypatch, dict(kenv, **{knob: "1"}))
                    assert got == base, (parts, part, knob)
                    if knob == OUT and len(base) > 1 and st1.retries == 0:  # one pass holds them all
                        assert st.retries >= 1
                    if knob == ECAP and base and (cache != "k4" or max_keys(base) > 8):
                        assert st.retries >= st1.retries + ecap_steps(max_keys(base), 1)
                    forced[knob] += st.retries > st1.retries
                    if cache == "dense":
                        _, _, un = _dense_run(staged, thr, monkeypatch, capfd, dict(kenv, **{knob: "1"}))
                        assert len(set(un)) == 1, (knob, un)
                        unlisted += un[0]
            assert sorted(union) == want, parts
            assert forced[OUT] > 0, forced
            assert cache != "dense" or unlisted > 0
            if cache != "k4" or max_keys(want) > 8:  # (a lane's own list finishes windows of <= 8 keys)
                assert forced[ECAP] > 0, forced
            if spills:
                assert forced[SPILL] > 0, forced


def _doc_rows(recs, doc_off, d):
    return sorted((int(r["start"]), int(r["end"]), int(r["pattern_index"]), float(r["similarity"]), int(r["insertions"]),
                   int(r["deletions"]), int(r["substitutions"]), int(r["swaps"]), int(r["edits"]))
                  for r in recs[int(doc_off[d]):int(doc_off[d + 1])])


@functools.lru_cache(maxsize=None)
def batch_case():
    """200 short ASCII documents (0-12 words of the long haystack's kind, every tenth empty)."""
    rng = Rng(0xBA7C4)
    docs = []
    for d in range(200):
        k = 0 if d % 10 == 3 else 1 + rng.next() % 12
        docs.append(" ".join(WORDS[rng.next() % 4][: 3 + rng.next() % 6] + "xyz"[rng.next() % 3] for _ in range(k)))
    b = B().fuzzy(L().edits(1))
    orc = OracleEngine(b, WORDS)
    plain = [sorted(orc.raw_rows(d, 0.7)) for d in docs]
    filtered = [sorted(orc.raw_rows(d, 0.7, prefilter=True)) for d in docs]
    return b, docs, 0.7, plain, filtered


@pytest.mark.parametrize("knob", [OUT, ECAP])
def test_batch_search_records(knob, monkeypatch):
    """StagedBatch.search_records: the loop driven by device-side segments, empty documents among
    them; per document == the oracle on that document alone."""
    from fuzzy_aho_corasick import _native
    b, docs, thr, plain, _ = batch_case()
    kmax = max(max_keys(p) for p in plain if p)
    assert sum(map(len, plain)) > 1 and kmax > 1 and any(not p for p in plain)
    sb = StagedBatch(b.build(WORDS), *batch_offsets([d.encode() for d in docs]))
    monkeypatch.setenv("FAC_NO_RC", "1")
    base, base_off = sb.search_records(O().threshold(thr))
    monkeypatch.setenv(knob, "1")
    st = _native.fac_stats()
    recs, doc_off = sb.search_records(O().threshold(thr), stats=st)
    assert list(doc_off) == list(base_off)
    assert [_doc_rows(recs, doc_off, d) for d in range(len(docs))] == plain \
        == [_doc_rows(base, base_off, d) for d in range(len(docs))]
    assert st.retries >= (1 if knob == OUT else ecap_steps(kmax, 1))


def test_batch_prefiltered_records(monkeypatch):
    """search_records(prefilter=True): the loop over the pre-filter's merged windows of every document."""
    from fuzzy_aho_corasick import _native
    b, docs, thr, _, filtered = batch_case()
    assert sum(map(len, filtered)) > 1
    sb = StagedBatch(b.build(WORDS), *batch_offsets([d.encode() for d in docs]))
    base, base_off = sb.search_records(O().threshold(thr), prefilter=True)
    monkeypatch.setenv(OUT, "1")
    st = _native.fac_stats()
    recs, doc_off = sb.search_records(O().threshold(thr), stats=st, prefilter=True)
    assert list(doc_off) == list(base_off)
    assert [_doc_rows(recs, doc_off, d) for d in range(len(docs))] == filtered \
        == [_doc_rows(base, base_off, d) for d in range(len(docs))]
    assert st.retries >= 1


def test_staged_prefiltered_records(monkeypatch):
    """search_prefiltered_records on one staged haystack: a window list from the pre-filter."""
    b, pats, text, thr, _ = long_case(False)
    want = sorted(OracleEngine(b, pats).raw_rows(text, thr, prefilter=True))
    assert len(want) > 1
    staged = b.build(pats).stage(text.encode())
    base, _ = staged.search_prefiltered_records(thr)
    monkeypatch.setenv(OUT, "1")
    recs, st = staged.search_prefiltered_records(thr)
    assert _doc_rows(recs, [0, len(recs)], 0) == _doc_rows(base, [0, len(base)], 0) == want
    assert st.retries >= 1


def test_ranked_batch_after_a_rerun(monkeypatch):
    """The ranking and splice kernels behind a re-run pass: ranked records per document == the oracle's
    FuzzyMatches::apply, and replace_batch's bytes == the unforced call's."""
    from fuzzy_aho_corasick import _native
    from test_gpu_batch import canon, oracle_doc, sim_bits
    b, docs, thr, plain, _ = batch_case()
    assert sum(map(len, plain)) > 1
    eng, orc = b.build(WORDS), OracleEngine(b, WORDS)
    sb = StagedBatch(eng, *batch_offsets([d.encode() for d in docs]))
    opts = O().threshold(thr)
    opts.order_, opts.overlap_ = Order.Default, Overlap.NonOverlapping
    want = [oracle_doc(orc, d, thr, opts.order_, opts.overlap_) for d in docs]
    table = ReplacementTable(eng, ["<N>", "<H>", None, ""])
    out0, off0 = sb.replace_bytes(table, opts)
    recs0, doc_off0 = sb.search_records(opts)
    monkeypatch.setenv(OUT, "1")
    st, st2 = _native.fac_stats(), _native.fac_stats()
    recs, doc_off = sb.search_records(opts, stats=st)
    assert list(doc_off) == list(doc_off0)
    for d in range(len(docs)):
        got = [r[:3] + (sim_bits(r[3]),) + r[4:] for r in _doc_rows(recs, doc_off, d)]
        assert _doc_rows(recs0, doc_off0, d) == _doc_rows(recs, doc_off, d), d
        assert canon(got, opts.order_, opts.overlap_) == canon(want[d], opts.order_, opts.overlap_), (d, docs[d])
    out, off = sb.replace_bytes(table, opts, stats=st2)
    assert out == out0 and list(off) == list(off0) and out != b"".join(d.encode() for d in docs)
    assert st.retries >= 1 and st2.retries >= 1


def test_auto_beam_count_pass_rerun(monkeypatch):
    """test_auto_beam_matches_oracle's budget 40, width 8 with a one-record buffer: the counting pass
    writes every window's queue length again in its re-run, and the switch window -- so the records --
    must not move. The counting pass searches every window unbeamed, so it emits what the engine
    without auto_beam finds: more than one record there forces the re-run."""
    monkeypatch.setenv("FAC_RC_MIN", "1")
    monkeypatch.setenv("FAC_RC_K", "4")
    rng = Rng(0xab ^ 40)
    cases = []
    for _ in range(40):
        b0, pats, hay, thr = random_case(rng, ASCII_VOCAB + UNI_VOCAB, ASCII_FILLER + UNI_FILLER, allow_beam=False)
        n0 = len(OracleEngine(b0, pats).raw_rows(hay, thr))  # (before auto_beam: the builder changes in place)
        b = b0.auto_beam(40, 8)
        cases.append((b, pats, hay, thr, n0, rows(OracleEngine(b, pats).search(hay, O().threshold(thr)))))
    assert sum(n0 > 1 for *_, n0, _ in cases) >= 10
    monkeypatch.setenv(OUT, "1")
    for b, pats, hay, thr, n0, want in cases:
        eng = b.build(pats)
        assert rows(eng.search(hay, O().threshold(thr))) == want, (pats, hay, thr)
        st, _ = _staged_vs_oracle(b, pats, hay, thr)
        assert st.retries >= (1 if n0 > 1 else 0), (pats, hay, thr)


@pytest.mark.parametrize("root_cache", ["off", "k2+k4"])
@pytest.mark.parametrize("seed,vocab,filler", [
    (0x1234_5678_9abc_def1, ASCII_VOCAB, ASCII_FILLER),
    (0xdead_beef_0bad_f00d, UNI_VOCAB, UNI_FILLER),
    (0x0a57_2a1c_0de5_51de, ASTRAL_VOCAB, ASTRAL_FILLER),
], ids=["ascii", "unicode", "astral"])
def test_differential_all_three_forced(seed, vocab, filler, root_cache, monkeypatch):
    """60 random cases per vocabulary with the three first sizes at 1 together: every search with more
    than one record re-runs, most of them several times and for more than one reason."""
    rng = Rng(seed ^ 0x3e9)
    cases = [random_case(rng, vocab, filler) for _ in range(60)]
    must = [len(OracleEngine(b, pats).raw_rows(hay, thr)) > 1 for b, pats, hay, thr in cases]
    assert sum(must) >= 10
    for k, v in dict(CACHE[root_cache], **{OUT: "1", ECAP: "1", SPILL: "1"}).items():
        monkeypatch.setenv(k, v)
    for (b, pats, hay, thr), forced in zip(cases, must):
        st, _ = _staged_vs_oracle(b, pats, hay, thr)
        assert st.retries >= (1 if forced else 0), (pats, hay, thr)
