"""Term counts on the device (fac_count_batch, count_kernels.hip). Part 1 runs the reduce alone
(fac_diag_count_terms) on synthetic documents at every tier and tier edge; part 2 goes through the
search: the expected value is the CPU oracle's applied rows of each document alone (ARef of
test_gpu_anchors.py), grouped by the pure-Python reference of test_counts_host.py. Every comparison
is exact, best_similarity by bits."""
import ctypes
import random

import numpy as np
import pytest

from fuzzy_aho_corasick import (Anchor, Boundary, DeviceError, FuzzyAhoCorasickBuilder as B, FuzzyLimits as L,
                                FuzzyReplacer, Order, Overlap, TERM_DTYPE, UnsupportedConfiguration, _native)
import batch_mapping_cases as map_cases
import batch_unicode_cases as uni_cases
from test_counts_host import SIMS, bits_of, make_recs, ref_terms, term_rows
from test_gpu_anchors import ARef, PATS, Sides, ascii_builder, ascii_docs
from test_gpu_boundaries import COMBOS, TWO, device_batch, options, staged

pytestmark = pytest.mark.gpu

LANE, GROUP, HIST = _native.COUNT_LANE_MAX, _native.COUNT_GROUP_MAX, _native.COUNT_HIST_KEYS
THR = 0.5
KEYS = [0, 0, 1, 2, 0]


# ---------------------------------------------------------------- 1. the reduce alone

def diag(docs, keys, n_patterns, n_keys, lane_max=0, group_max=0, totals=True):
    """fac_diag_count_terms on documents given as lists of (pattern_index, similarity bits):
    (the terms of every document as term_rows, the totals or None)."""
    rows = [r for d in docs for r in d]
    recs = make_recs(rows)
    off = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
    karr = np.asarray(keys, dtype=np.uint32) if keys is not None else None
    nk = n_keys if keys is not None else n_patterns
    tot = np.full((max(nk, 1), 2), 0xABAB, dtype=np.uint64) if totals else None
    toff = np.full(len(docs) + 1, 0xABAB, dtype=np.uint64)
    ptr, n = ctypes.POINTER(_native.fac_term)(), ctypes.c_uint64()
    rc = _native.lib.fac_diag_count_terms(recs.ctypes.data if rows else None, len(rows), off.ctypes.data, len(docs),
                                          karr.ctypes.data if karr is not None else None, n_patterns, n_keys, lane_max,
                                          group_max, ctypes.byref(ptr), ctypes.byref(n), toff.ctypes.data,
                                          tot.ctypes.data if totals else None)
    assert rc == 0, _native.last_error()
    terms = _native.take_terms(ptr, n.value)
    assert toff[0] == 0 and int(toff[-1]) == len(terms) and (np.diff(toff.astype(np.int64)) >= 0).all()
    return [term_rows(terms[int(toff[d]):int(toff[d + 1])]) for d in range(len(docs))], (tot[:nk] if totals else None)


def ref_totals(per_doc, n_keys):
    tot = np.zeros((n_keys, 2), dtype=np.uint64)
    for terms in per_doc:
        for k, c, _, _ in terms:
            tot[k, 0] += c
            tot[k, 1] += 1
    return tot


def check_diag(docs, keys, n_patterns, n_keys, **kw):
    got, tot = diag(docs, keys, n_patterns, n_keys, **kw)
    want = [ref_terms(d, keys) for d in docs]
    for d, (g, w) in enumerate(zip(got, want)):
        assert g == w, (d, len(docs[d]), kw)
    assert (tot == ref_totals(want, n_keys if keys is not None else n_patterns)).all()
    return want


def key_shapes(m, top):
    """The pattern indices of a document of m records, one list per shape; top: the greatest index."""
    q = m // 4
    return [[7] * m, list(range(m)), list(range(m - 1, -1, -1)), [i // 2 for i in range(m)],
            [i if i < q else m if i < m - q else m + 1 + i for i in range(m)],  # one run straddling the middle
            [top if i % 2 else 0 for i in range(m)]]


def synthetic(sizes, top, seed):
    """One document per size and shape, similarities drawn from 4 values, an empty document before
    every third one, and as the first and the last document."""
    rng = random.Random(seed)
    docs = [[]]
    for m in sizes:
        for k, shape in enumerate(key_shapes(m, top)):
            if k % 3 == 0:
                docs.append([])
            docs.append([(p, rng.choice(SIMS)) for p in shape])
    return docs + [[]]


def tier_counts(docs, lane_max, group_max):
    sizes = [len(d) for d in docs if d]
    return (sum(m <= lane_max for m in sizes), sum(lane_max < m <= group_max for m in sizes),
            sum(m > group_max for m in sizes))


@pytest.fixture(scope="module")
def default_docs():
    n_pat = 2 * GROUP + 8  # every shape's indices are below it
    docs = synthetic([0, 1, 2, LANE - 1, LANE, LANE + 1, 63, 64, 65, GROUP - 1, GROUP, GROUP + 1], n_pat - 1, 0xC0DE)
    assert min(tier_counts(docs, LANE, GROUP)) >= 2
    assert sum(len(d) in (63, 64) for d in docs) >= 2 and sum(len(d) in (65, GROUP) for d in docs) >= 2  # both group paths
    assert not docs[0] and not docs[-1] and max(p for d in docs for p, _ in d) == n_pat - 1
    return docs, n_pat


def test_every_tier_default_ceilings(default_docs):
    docs, n_pat = default_docs
    want = check_diag(docs, None, n_pat, n_pat)
    assert any(t[0] == n_pat - 1 for w in want for t in w)  # key n_keys - 1 is present
    assert any(len(w) == GROUP + 1 for w in want) and any(len(w) == 1 and w[0][1] == GROUP + 1 for w in want)
    check_diag(docs, None, n_pat, 0)  # n_keys 0 with keys NULL


def test_every_tier_folded_keys(default_docs):
    docs, n_pat = default_docs
    keys = [(p * 7) % 11 if p % 5 else 11 for p in range(n_pat)]
    want = check_diag(docs, keys, n_pat, 12)
    assert any(t[0] == 11 for w in want for t in w)
    # ties inside a group: some term's best similarity is reached by several patterns
    assert any(sum(1 for p, b in d if keys[p] == t[0] and b == t[2]) > 1 for d, w in zip(docs, want) for t in w)


def test_every_tier_smallest_ceilings():
    """lane_max 2 and group_max 4 on documents of 1..9 records: all three tiers in one call."""
    docs = synthetic(range(1, 10), 19, 0xBEEF)
    assert min(tier_counts(docs, 2, 4)) >= 2
    check_diag(docs, None, 20, 20, lane_max=2, group_max=4)
    check_diag(docs, [p % 3 for p in range(20)], 20, 3, lane_max=2, group_max=4)
    check_diag(docs, None, 20, 20, lane_max=1, group_max=1)  # one-record documents by lanes, all else sorted
    check_diag(docs, None, 20, 20)


@pytest.mark.parametrize("n_keys", [5, HIST, HIST + 1])
def test_totals_both_modes(n_keys):
    used = [0, n_keys // 2, n_keys - 1]
    rng = random.Random(n_keys)
    docs = [[(rng.choice(used), rng.choice(SIMS)) for _ in range(rng.choice([0, 1, 2, 3, 9, 70]))] for _ in range(300)]
    docs += [[(used[1], SIMS[0])]] * 5000  # one hot key shared by 5 000 one-record documents
    docs += [[(used[2], SIMS[1])] * 70000, []]  # a count above 2^16 in one term
    want = check_diag(docs, None, n_keys, n_keys)
    tot = ref_totals(want, n_keys)
    assert tot[used[1], 1] >= 5000 and tot[used[2], 0] > 70000 and (tot[[k for k in range(n_keys) if k not in used]] == 0).all()
    if n_keys == 5:  # the same through a key table
        check_diag(docs, [4, 3, 2, 1, 0], 5, 5)


def test_empty_inputs_and_no_totals():
    assert diag([], None, 3, 3)[0] == []
    got, tot = diag([], [0, 1, 1], 3, 2)
    assert got == [] and (tot == 0).all() and tot.shape == (2, 2)
    got, tot = diag([[], [], []], None, 3, 3)
    assert got == [[], [], []] and (tot == 0).all()
    docs = [[(1, SIMS[0]), (0, SIMS[1]), (1, SIMS[2])], [], [(2, SIMS[3])]]
    got, tot = diag(docs, None, 3, 3, totals=False)  # records present, totals NULL
    assert tot is None and got == [ref_terms(d) for d in docs]


def test_diag_argument_errors():
    recs = make_recs([(0, SIMS[0]), (2, SIMS[0])])
    off = np.array([0, 2], dtype=np.uint64)
    ptr, n = ctypes.POINTER(_native.fac_term)(), ctypes.c_uint64()
    toff = np.zeros(2, dtype=np.uint64)

    def call(n_patterns, n_keys, keys=None, lane_max=0, group_max=0, offsets=off):
        karr = np.asarray(keys, dtype=np.uint32) if keys is not None else None
        return _native.lib.fac_diag_count_terms(recs.ctypes.data, 2, offsets.ctypes.data, 1,
                                                karr.ctypes.data if karr is not None else None, n_patterns, n_keys,
                                                lane_max, group_max, ctypes.byref(ptr), ctypes.byref(n), toff.ctypes.data, None)

    assert call(3, 3) == 0
    _native.lib.fac_buffer_free(ctypes.cast(ptr, ctypes.c_void_p))
    assert call(3, 3, lane_max=LANE + 1) == _native.FAC_E_INVALID
    assert call(3, 3, group_max=GROUP + 1) == _native.FAC_E_INVALID
    assert call(2, 2) == _native.FAC_E_INVALID  # pattern_index 2 is not below n_patterns
    assert call(3, 2) == _native.FAC_E_INVALID  # keys NULL: n_keys is 0 or n_patterns
    assert call(3, 2, keys=[0, 1, 2]) == _native.FAC_E_INVALID  # a key >= n_keys
    assert call(3, 3, offsets=np.array([0, 1], dtype=np.uint64)) == _native.FAC_E_INVALID
    assert not ptr


# ---------------------------------------------------------------- 2. through the search

def expected(ref, docs, opts, sides, keys=None, prefilter=False):
    """Per document, the reference's terms of the oracle's applied rows."""
    return [ref_terms([(r[2], r[3]) for r in ref.rows(doc, opts, sides, prefilter)], keys) for doc in docs]


def split_terms(terms, doc_off):
    assert doc_off[0] == 0 and int(doc_off[-1]) == len(terms)
    return [term_rows(terms[int(doc_off[d]):int(doc_off[d + 1])]) for d in range(len(doc_off) - 1)]


def check_counts(sb, ref, docs, thr, sides, combos, keys=None, n_keys=None, n_patterns=len(PATS), prefilter=False):
    nk = n_keys if n_keys is not None else (max(keys) + 1 if keys is not None else n_patterns)
    first = None
    for order, overlap in combos:
        opts = options(thr, order, overlap)
        want = expected(ref, docs, opts, sides, keys, prefilter)
        first = want if first is None else first
        terms, doc_off, tot = sb.count_records(opts, keys, n_keys, totals=True, prefilter=prefilter)
        assert terms.dtype == TERM_DTYPE and len(doc_off) == len(docs) + 1
        for d, (g, w) in enumerate(zip(split_terms(terms, doc_off), want)):
            assert g == w, (int(sides), order, overlap, d, docs[d])
        assert tot.shape == (nk, 2) and (tot == ref_totals(want, nk)).all(), (order, overlap)
        assert sb.count_records(opts, keys, n_keys, prefilter=prefilter)[2] is None
    return first  # (the first combination's terms)


@pytest.fixture(scope="module")
def plain():
    b = ascii_builder()
    eng, ref = b.build(PATS), ARef(b, PATS)
    return eng, ref, ascii_docs(eng.max_match_graphemes())


@pytest.mark.parametrize("where", ["host", "device"])
def test_ascii_column_every_combo(plain, where):
    eng, ref, docs = plain
    sb, keep = (staged(eng, docs), None) if where == "host" else device_batch(eng, docs, pad=b"b")
    want = check_counts(sb, ref, docs, THR, Sides(0), COMBOS)
    assert any(len(w) > 1 for w in want) and any(t[1] > 1 for w in want for t in w) and any(not w for w in want)
    folded = check_counts(sb, ref, docs, THR, Sides(0), COMBOS, keys=KEYS)
    assert folded != want
    check_counts(sb, ref, docs, THR, Sides(0), TWO, keys=KEYS, n_keys=7)  # a key space larger than the keys used
    del keep


def test_masks(plain):
    eng, ref, docs = plain
    docs = docs + ["abc d", "x abc", "abc-abcd", "b b", "zabcd abc"]
    plain_terms = expected(ref, docs, options(THR), Sides(0))
    for anchors, bounds in ((Anchor.NONE, Boundary.WHOLE), (Anchor.START, Boundary.NONE), (Anchor.START, Boundary.WHOLE)):
        sb = staged(eng, docs, boundaries=bounds, anchors=anchors)
        for keys in (None, KEYS):
            want = check_counts(sb, ref, docs, THR, Sides(anchors, bounds), TWO, keys=keys)
        assert expected(ref, docs, options(THR), Sides(anchors, bounds)) != plain_terms and any(want)


def test_prefiltered(plain):
    eng, ref, docs = plain
    assert eng.with_prefilter().is_active()
    sb = staged(eng, docs)
    check_counts(sb, ref, docs, THR, Sides(0), COMBOS, prefilter=True)
    check_counts(sb, ref, docs, THR, Sides(0), TWO, keys=KEYS, prefilter=True)


def test_mixed_non_ascii_column_prefiltered():
    b = B().fuzzy(L().edits(1)).case_insensitive(True)
    pats, thr = uni_cases.SLICE_PATS, uni_cases.SLICE_THR
    eng, ref = b.build(pats), ARef(b, pats)
    docs = uni_cases.slice_docs() + ["hello world", "", "cell"]
    assert any(d.isascii() for d in docs) and not all(d.isascii() for d in docs)
    sb = staged(eng, docs, unicode_prefilter=True)
    keys = [p % 4 for p in range(len(pats))]
    for kk in (None, keys):
        want = check_counts(sb, ref, docs, thr, Sides(0), TWO, keys=kk, n_patterns=len(pats), prefilter=True)
        check_counts(sb, ref, docs, thr, Sides(0), TWO, keys=kk, n_patterns=len(pats))
    assert sum(len(w) for w in want) > len(docs) // 2


def test_mapping_engine_column():
    b = map_cases.cut_builder(B, L)
    pats, thr = map_cases.CUT_PATS, map_cases.CUT_THR
    eng, ref = b.build(pats), ARef(b, pats)
    docs = map_cases.cut_batches()["neighbours"]
    assert not all(d.isascii() for d in docs)
    sb = staged(eng, docs, unicode_mappings=True)
    want = check_counts(sb, ref, docs, thr, Sides(0), COMBOS, n_patterns=len(pats))
    check_counts(sb, ref, docs, thr, Sides(0), TWO, keys=[1, 0, 1], n_patterns=len(pats))
    assert sum(len(w) for w in want) >= 4
    with pytest.raises(UnsupportedConfiguration):  # without the opt-in: nothing runs
        staged(eng, docs).count_records(options(thr))


def test_sorted_tier_behind_a_search(plain):
    eng, ref, _ = plain
    docs = ["", "abcd" * 130, "b", "abcd" * 3]
    opts = options(THR)
    rows = [ref.rows(d, opts, Sides(0)) for d in docs]
    assert len(rows[1]) > GROUP and len(rows[2]) == 1 and not rows[0] and LANE < len(rows[3]) <= GROUP
    sb = staged(eng, docs)
    for keys in (None, KEYS):
        want = check_counts(sb, ref, docs, THR, Sides(0), [(Order.Unsorted, Overlap.Keep)], keys=keys)
    assert sum(t[1] for t in want[1]) == len(rows[1])
    check_counts(sb, ref, docs, THR, Sides(0), [(Order.Default, Overlap.NonOverlapping)])


def test_device_outputs(plain):
    import torch
    eng, ref, docs = plain
    sb = staged(eng, docs)
    opts = options(THR)
    want = expected(ref, docs, opts, Sides(0), KEYS)
    flat = [t for w in want for t in w]
    host_terms, host_off, host_tot = sb.count_records(opts, KEYS, totals=True)
    nk = max(KEYS) + 1
    out = torch.full((len(flat) * 16 + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    d_off = torch.full((len(docs) + 1,), -7, dtype=torch.int64, device="cuda")
    d_tot = torch.full((nk, 2), -7, dtype=torch.int64, device="cuda")
    filled, doc_off, tot = sb.count_records(opts, KEYS, out=out, doc_offsets_out=d_off, totals=d_tot)
    assert filled.is_cuda and filled.numel() == len(flat) * 16 and tot is d_tot
    assert term_rows(np.frombuffer(filled.cpu().numpy().tobytes(), dtype=TERM_DTYPE)) == flat
    assert (out[len(flat) * 16:] == 0xEE).all()  # nothing behind the terms
    assert list(doc_off) == list(host_off) == d_off.cpu().numpy().view(np.uint64).tolist()
    assert (d_tot.cpu().numpy().view(np.uint64) == host_tot).all() and (host_tot == ref_totals(want, nk)).all()
    assert term_rows(host_terms) == flat
    # one term too small: the count needed, and no device output touched
    small = torch.full(((len(flat) - 1) * 16,), 0xEE, dtype=torch.uint8, device="cuda")
    d_off.fill_(-7)
    d_tot.fill_(-7)
    with pytest.raises(DeviceError) as ei:
        sb.count_records(opts, KEYS, out=small, doc_offsets_out=d_off, totals=d_tot)
    assert ei.value.code == _native.FAC_E_OUTPUT_CAPACITY == 106 and ei.value.needed == len(flat)
    assert (small == 0xEE).all() and (d_off == -7).all() and (d_tot == -7).all()


@pytest.mark.parametrize("keys", [None, KEYS])
def test_term_matrix(plain, keys):
    import torch
    eng, ref, docs = plain
    sb = staged(eng, docs)
    opts = options(THR, Order.Default, Overlap.NonOverlapping)
    want = expected(ref, docs, opts, Sides(0), keys)
    nk = max(keys) + 1 if keys else len(PATS)
    dense = {v: np.zeros((len(docs), nk), dtype=np.float32) for v in ("count", "similarity")}
    for d, w in enumerate(want):
        for k, c, sim, _ in w:
            dense["count"][d, k] = c
            dense["similarity"][d, k] = np.array([sim], dtype=np.uint32).view(np.float32)[0]
    _, doc_off, _ = sb.count_records(opts, keys)
    for values in ("count", "similarity"):
        m = sb.term_matrix(opts, keys, values=values)
        assert m.is_cuda and m.layout == torch.sparse_csr and tuple(m.shape) == (len(docs), nk) and m.dtype == torch.float32
        assert m.crow_indices().cpu().tolist() == [int(x) for x in doc_off]
        assert (m.to_dense().cpu().numpy().view(np.uint32) == dense[values].view(np.uint32)).all()
    assert dense["count"].sum() > 0
    if keys:  # a key space larger than the keys used: empty columns
        wide = sb.term_matrix(opts, keys, n_keys=nk + 3)
        assert tuple(wide.shape) == (len(docs), nk + 3) and (wide.to_dense()[:, :nk].cpu().numpy() == dense["count"]).all()
    else:  # without a key table the key space is the pattern count
        with pytest.raises(DeviceError):
            sb.term_matrix(opts, keys, n_keys=nk + 3)
    with pytest.raises(ValueError):
        sb.term_matrix(opts, keys, values="mean")
    empty = staged(eng, ["", "zzz"]).term_matrix(opts, keys)
    assert tuple(empty.shape) == (2, nk) and empty.values().numel() == 0


def as_dicts(want):
    return [{k: (c, sim, p) for k, c, sim, p in w} for w in want]


def got_dicts(per_doc):
    return [{k: (t.count, bits_of(t.best_similarity), t.best_pattern) for k, t in terms.items()} for terms in per_doc]


def test_conveniences(plain):
    eng, ref, docs = plain
    opts = options(THR, Order.Default, Overlap.NonOverlapping)
    for keys in (None, KEYS):
        want = expected(ref, docs, opts, Sides(0), keys)
        got = eng.count_batch(docs, opts, keys)
        assert got_dicts(got) == as_dicts(want) and all(list(g) == sorted(g) for g in got)
        pf = eng.with_prefilter().count_batch(docs, opts, keys)
        assert got_dicts(pf) == as_dicts(expected(ref, docs, opts, Sides(0), keys, prefilter=True))
    anchored = eng.count_batch(docs, opts, KEYS, anchors=Anchor.WHOLE)
    assert got_dicts(anchored) == as_dicts(expected(ref, docs, opts, Sides(3), KEYS)) != got_dicts(got)
    reps = ["Alpha", "Alpha", "Beta", "Gamma", "Alpha"]
    forms = ["Alpha", "Beta", "Gamma"]
    assert FuzzyReplacer.term_keys(reps) == (KEYS, forms)
    by_form = FuzzyReplacer(eng, reps).count_batch(docs, opts)
    assert by_form == [{forms[k]: c for k, c, _, _ in w} for w in expected(ref, docs, opts, Sides(0), KEYS)]
    assert any(len(d) > 1 for d in by_form)


def test_prefiltered_convenience_routes_non_ascii_documents_one_by_one():
    """An engine without a filter (a pattern of 64 graphemes has none) sends the ASCII documents as one
    batch and the others through the host's term_counts."""
    b = B().fuzzy(L().edits(1)).case_insensitive(True)
    pats = uni_cases.SLICE_PATS + ["q" * 64]
    eng, ref = b.build(pats), ARef(b, pats)
    assert not eng.with_prefilter().is_active()
    docs = ["hello wörld", "hello world", "", "я cell я", "cafés"]
    opts = options(uni_cases.SLICE_THR, Order.Default, Overlap.NonOverlapping)
    keys = [p % 3 for p in range(len(pats))]
    for kk in (None, keys):
        got = eng.with_prefilter().count_batch(docs, opts, kk)
        assert got_dicts(got) == as_dicts(expected(ref, docs, opts, Sides(0), kk, prefilter=True))


def test_errors(plain):
    eng, _, docs = plain
    sb = staged(eng, docs)
    for bad in (dict(keys=[0, 0, 1, 2, 0], n_keys=2), dict(keys=None, n_keys=3), dict(keys=None, n_keys=6)):
        with pytest.raises(DeviceError) as ei:
            sb.count_records(options(THR), **bad)
        assert ei.value.code == _native.FAC_E_INVALID, bad
    assert sb.count_records(options(THR), None, len(PATS))[1][-1] > 0  # the pattern count is accepted
    with pytest.raises(ValueError):
        sb.count_records(options(THR), [0, 1])  # one key per pattern
    b = B().fuzzy(L().edits(1)).mapping("ß", "ss")
    with pytest.raises(UnsupportedConfiguration):
        staged(b.build(["straße"]), ["straße", "x"]).count_records(options(0.8))


def test_n_keys_zero_without_a_table_means_the_pattern_count(plain):
    """keys None with n_keys None, 0 or the pattern count: one key space, the pattern count, for the
    totals on the host, the totals in HBM and the matrix."""
    import torch
    eng, ref, docs = plain
    sb = staged(eng, docs)
    opts = options(THR)
    want = expected(ref, docs, opts, Sides(0))
    tot_want = ref_totals(want, len(PATS))
    assert tot_want[:, 0].sum() > 0
    for n_keys in (None, 0, len(PATS)):
        terms, doc_off, tot = sb.count_records(opts, None, n_keys, totals=True)
        assert split_terms(terms, doc_off) == want
        assert tot.shape == (len(PATS), 2) and (tot == tot_want).all(), n_keys
        d_tot = torch.full((len(PATS) + 2, 2), -7, dtype=torch.int64, device="cuda")
        assert sb.count_records(opts, None, n_keys, totals=d_tot)[2] is d_tot
        got = d_tot.cpu().numpy()
        assert (got[:len(PATS)].view(np.uint64) == tot_want).all() and (got[len(PATS):] == -7).all(), n_keys
        with pytest.raises(ValueError):  # a tensor smaller than the pattern count is refused, nothing runs
            sb.count_records(opts, None, n_keys, totals=torch.zeros((len(PATS) - 1, 2), dtype=torch.int64, device="cuda"))
        m = sb.term_matrix(opts, None, n_keys)
        assert tuple(m.shape) == (len(docs), len(PATS)) and int(m.col_indices().max()) < len(PATS)
        assert m.to_dense().sum().item() == float(tot_want[:, 0].sum())
    assert got_dicts(eng.count_batch(docs, opts, None, 0)) == as_dicts(want)
    assert got_dicts(eng.with_prefilter().count_batch(docs, opts, None, 0)) == as_dicts(
        expected(ref, docs, opts, Sides(0), None, prefilter=True))
    for call in (eng.count_batch, eng.with_prefilter().count_batch):
        with pytest.raises(DeviceError) as ei:
            call(docs, opts, None, len(PATS) + 1)
        assert ei.value.code == _native.FAC_E_INVALID
