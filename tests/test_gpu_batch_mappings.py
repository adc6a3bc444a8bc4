"""Batches that hold non-ASCII documents, searched by engines with multi-character mappings
(fac_batch_allow_unicode_mappings): every batch call on an opted-in batch gives, per document, what
the CPU oracle gives for that document alone -- bit for bit, similarity included -- and what the
device's own single-document call gives. The documents are batch_mapping_cases.py's; the oracle-only
test_batch_mappings_host.py shows that they hold the records that make the comparison mean something."""
import pytest
import torch

import batch_mapping_cases as cases
from fuzzy_aho_corasick import (FuzzyAhoCorasickBuilder as B, FuzzyLimits as L, Order, Overlap, ReplacementTable,
                                SearchOptions as O, StagedBatch, UnsupportedConfiguration, _native, batch_offsets)
from oracle_harness import OracleEngine
from test_gpu_batch import canon, check_batch, full_rows, set_knobs, sim_bits

pytestmark = pytest.mark.gpu

REFUSAL = "batches with non-ASCII documents do not support multi-character mappings"
MODES = (_native.FAC_RENDER_STRIP_PREFIX, _native.FAC_RENDER_STRIP_SUFFIX, _native.FAC_RENDER_SEGMENT_TEXT)
REPS = ["<street>", None, "<big>"]


def opted_in(eng, docs):
    return StagedBatch(eng, *batch_offsets([d.encode("utf-8") for d in docs]), unicode_mappings=True)


def rec_rows(recs):
    return [(int(r["start"]), int(r["end"]), int(r["pattern_index"]), sim_bits(float(r["similarity"])),
             int(r["insertions"]), int(r["deletions"]), int(r["substitutions"]), int(r["swaps"]), int(r["edits"]))
            for r in recs]


def seg_rows(segs):
    return [(s.matched().start, s.matched().end, s.matched().pattern_index) if s.matched() is not None
            else (s.unmatched().start, s.unmatched().end, _native.FAC_UNMATCHED) for s in segs]


def check_every_call(eng, orc, docs, thr, sb):
    """search, replace, extract, segment and the three render modes, plain and pre-filtered (the plain
    call again: an engine with mappings has no filter), per document against the oracle on that
    document alone and against the device's single-document call."""
    check_batch(eng, orc, docs, thr, sb=sb)
    opts = O().threshold(thr)
    order, overlap = opts.order_, opts.overlap_
    enc = [d.encode("utf-8") for d in docs]
    table = ReplacementTable(eng, REPS)
    callback = lambda m: REPS[m.pattern_index]  # noqa: E731
    one = [eng.search(d, opts) for d in docs]
    want = [orc.search(d, opts) for d in docs]
    compared = 0
    for pf in (False, True):
        recs, doc_off = sb.search_records(opts, prefilter=pf)
        got = [rec_rows(recs[int(doc_off[d]):int(doc_off[d + 1])]) for d in range(len(docs))]
        rep, rep_off = sb.replace_bytes(table, opts, prefilter=pf)
        _, ex_doc, ex_text, ex_item = sb.extract(None, opts, prefilter=pf)
        srecs, soff = sb.segment_records(opts, prefilter=pf)
        rendered = {m: sb.render_bytes(m, opts, prefilter=pf) for m in MODES}
        for d, doc in enumerate(docs):
            assert canon(got[d], order, overlap) == canon(full_rows(one[d]), order, overlap), (pf, d, doc)
            assert canon(got[d], order, overlap) == canon(full_rows(want[d]), order, overlap), (pf, d, doc)
            items = [ex_text[int(ex_item[i]):int(ex_item[i + 1])].decode("utf-8")
                     for i in range(int(ex_doc[d]), int(ex_doc[d + 1]))]
            assert items == [enc[d][r[0]:r[1]].decode("utf-8") for r in got[d]], (pf, d, doc)
            assert sorted(items) == sorted(want[d].matched_strings()) == sorted(one[d].matched_strings())
            ms = orc._segmented(doc, opts)
            if len({m.start for m in ms}) != len(list(ms)):
                continue  # kept records of equal start: the crate leaves their order open (matches.rs:111)
            compared += 1
            out = rep[int(rep_off[d]):int(rep_off[d + 1])].decode("utf-8")
            assert out == orc.replace(doc, opts, callback) == eng.replace(doc, opts, callback), (pf, d, doc)
            mine = [(int(r["start"]), int(r["end"]), int(r["pattern_index"])) for r in srecs[int(soff[d]):int(soff[d + 1])]]
            assert mine == seg_rows(ms.segment_iter()) == seg_rows(eng.segment_iter(doc, opts)), (pf, d, doc)
            for mode, host, dev in ((MODES[0], orc.strip_prefix, eng.strip_prefix), (MODES[1], orc.strip_suffix, eng.strip_suffix),
                                    (MODES[2], orc.segment_text, eng.segment_text)):
                buf, off = rendered[mode]
                assert buf[int(off[d]):int(off[d + 1])].decode("utf-8") == host(doc, opts) == dev(doc, opts), (pf, mode, d, doc)
    assert compared >= len(docs)  # (of 2 x len(docs))
    return got


@pytest.fixture(scope="module")
def cut_engines():
    b = cases.cut_builder(B, L)
    return b.build(cases.CUT_PATS), OracleEngine(b, cases.CUT_PATS)


def whole(rows, p):
    """The pattern p matched whole: similarity 1 (a mapping costs nothing and counts as a substitution)."""
    return any(r[2] == p and r[3] == sim_bits(1.0) for r in rows)


@pytest.mark.parametrize("name", sorted(cases.cut_batches()))
def test_cuts(cut_engines, name):
    eng, orc = cut_engines
    docs = cases.cut_batches()[name]
    got = check_every_call(eng, orc, docs, cases.CUT_THR, opted_in(eng, docs))
    hits = [[p for p in range(3) if whole(rows, p)] for rows in got]
    if name == "split_ss":  # a side split by a document boundary matches in neither document
        assert hits == [[] for _ in docs]
    if name == "ends_at_last":  # a side that ends exactly at the document's last grapheme matches
        assert hits == [[2], [], [2], [1], [], [2], [0], [2]]
    if name == "one_short":  # one grapheme short of the end: no match
        assert hits == [[] for _ in docs]
    if name == "neighbours":
        assert hits == [[0], [0], [0], [0], [2], [], [], [1]]
    if name == "tile_256":
        assert hits == [[0], [], [0], [0], []]
    if name == "tile_257":
        assert hits == [[0], [], [], [1]]


def test_list_methods_take_the_keyword(cut_engines):
    eng, orc = cut_engines
    docs = cases.cut_batches()["neighbours"]
    opts = O().threshold(cases.CUT_THR)
    opts.order_, opts.overlap_ = Order.Default, Overlap.NonOverlapping  # (no kept records of equal start here)
    kw = dict(unicode_mappings=True)
    assert [full_rows(m) for m in eng.search_batch(docs, opts, **kw)] == [full_rows(eng.search(d, opts)) for d in docs]
    assert sum(len(m) for m in eng.search_batch(docs, opts, **kw)) >= 6
    callback = lambda m: REPS[m.pattern_index]  # noqa: E731
    assert eng.replace_batch(docs, opts, REPS, **kw) == [orc.replace(d, opts, callback) for d in docs]
    assert eng.matched_strings_batch(docs, opts, **kw) == eng.extract_batch(docs, opts, **kw) \
        == [eng.search(d, opts).matched_strings() for d in docs]
    assert eng.strip_prefix_batch(docs, opts, **kw) == [orc.strip_prefix(d, opts) for d in docs]
    assert eng.strip_suffix_batch(docs, opts, **kw) == [orc.strip_suffix(d, opts) for d in docs]
    assert eng.segment_text_batch(docs, opts, **kw) == [orc.segment_text(d, opts) for d in docs]
    assert eng.split_batch(docs, opts, **kw) == [list(orc.split(d, opts)) for d in docs]
    assert [[s.as_str() for s in segs] for segs in eng.segment_batch(docs, opts, **kw)] \
        == [[s.as_str() for s in eng.segment_iter(d, opts)] for d in docs]
    # the pre-filtered conveniences need no keyword: they send all texts as one opted-in batch
    pf = eng.with_prefilter()
    assert not pf.is_active() and pf._batch_parts([d.encode("utf-8") for d in docs]) == list(range(len(docs)))
    assert [full_rows(m) for m in pf.search_batch(docs, opts)] == [full_rows(eng.search(d, opts)) for d in docs]
    assert pf.replace_batch(docs, opts, REPS) == eng.replace_batch(docs, opts, REPS, **kw)
    assert pf.matched_strings_batch(docs, opts) == eng.matched_strings_batch(docs, opts, **kw)
    assert pf.segment_text_batch(docs, opts) == eng.segment_text_batch(docs, opts, **kw)
    assert pf.split_batch(docs, opts) == eng.split_batch(docs, opts, **kw)


def test_opt_out_refuses_as_before(cut_engines):
    eng, _ = cut_engines
    docs = cases.cut_batches()["neighbours"]
    enc = [d.encode("utf-8") for d in docs]
    opts = O().threshold(cases.CUT_THR)
    table = ReplacementTable(eng, REPS)

    def calls(sb):
        for pf in (False, True):
            yield lambda: sb.search_records(opts, prefilter=pf)
            yield lambda: sb.replace_bytes(table, opts, prefilter=pf)
            yield lambda: sb.extract(None, opts, prefilter=pf)
            yield lambda: sb.segment_records(opts, prefilter=pf)
            for mode in MODES:
                yield lambda: sb.render_bytes(mode, opts, prefilter=pf)

    def refused(sb):
        n = 0
        for call in calls(sb):
            with pytest.raises(UnsupportedConfiguration) as ei:
                call()
            assert REFUSAL in str(ei.value)
            n += 1
        return n

    sb = StagedBatch(eng, *batch_offsets(enc))
    assert refused(sb) == 14
    assert sb.allow_unicode_mappings() is sb
    assert sum(1 for call in calls(sb) if call() is not None) == 14
    sb.allow_unicode_mappings(False)
    assert refused(sb) == 14
    sb.allow_unicode_prefilter()  # the other opt-in is independent
    assert refused(sb) == 14
    for fn in (eng.search_batch, eng.matched_strings_batch, eng.strip_prefix_batch, eng.segment_batch):
        with pytest.raises(UnsupportedConfiguration) as ei:
            fn(docs, opts)
        assert REFUSAL in str(ei.value)
    # an all-ASCII batch never needed the opt-in
    asc = [d for d in docs if d.isascii()]
    assert len(StagedBatch(eng, *batch_offsets([d.encode() for d in asc])).search_records(opts)[0]) > 0


def device_batch(eng, docs, reuse=None, **kw):
    data, offs = batch_offsets([d.encode("utf-8") for d in docs])
    d_data = torch.frombuffer(bytearray(data or b"\0"), dtype=torch.uint8).cuda()
    d_off = torch.tensor(offs, dtype=torch.int64).cuda()
    sb = StagedBatch.from_device(eng, d_data.data_ptr(), d_off.data_ptr(), len(docs), len(data), reuse=reuse, **kw)
    sb.data, sb._keep = data, (d_data, d_off)  # (borrowed device memory: alive as long as the batch)
    return sb


def test_the_flag_survives_a_restage_in_place(cut_engines):
    eng, orc = cut_engines
    batches = cases.cut_batches()
    sb = device_batch(eng, batches["neighbours"], unicode_mappings=True)
    combos = [(Order.Unsorted, Overlap.Keep), (Order.Default, Overlap.NonOverlapping)]
    check_batch(eng, orc, batches["neighbours"], cases.CUT_THR, combos=combos, sb=sb)
    for name in ("tile_257", "one_short", "ends_at_last", "tile_256", "split_ss"):  # longer, shorter, ...
        again = device_batch(eng, batches[name], reuse=sb)  # no keyword: the batch keeps its opt-in
        assert again is sb
        check_batch(eng, orc, batches[name], cases.CUT_THR, combos=combos, sb=sb)
    device_batch(eng, ["plain", "ascii"], reuse=sb)
    check_batch(eng, orc, ["plain", "ascii"], cases.CUT_THR, combos=combos, sb=sb)
    device_batch(eng, batches["neighbours"], reuse=sb)
    sb.allow_unicode_mappings(False)
    with pytest.raises(UnsupportedConfiguration) as ei:
        sb.search_records(O().threshold(cases.CUT_THR))
    assert REFUSAL in str(ei.value)


@pytest.mark.parametrize("seed,vocab", cases.DIFF_SEEDS)
def test_differential(seed, vocab):
    """Random mixed batches of random engines with one to three mapping rules, every Order x Overlap,
    == the oracle on each document alone."""
    rng = cases.Rng(seed)
    total = uni = 0
    for _ in range(cases.N_BATCHES):
        b, pats, docs, thr = cases.mapping_batch(rng, vocab)
        eng, orc = b.build(pats), OracleEngine(b, pats)
        sb = check_batch(eng, orc, docs, thr, sb=opted_in(eng, docs))
        total += len(sb.search_records(O().threshold(thr))[0])
        uni += sum(not d.isascii() for d in docs)
    assert total > 0 and uni > 0


@pytest.mark.parametrize("cache", ["off", "k4"])
def test_differential_restaged_on_the_device(cache, monkeypatch):
    """One from_device batch, opted in once and restaged in place for every set of documents."""
    set_knobs(monkeypatch, cache, False)
    rng = cases.Rng(0x5EED_B004)
    b, pats, docs, thr = cases.mapping_batch(rng, cases.DIFF_SEEDS[2][1])
    eng, orc = b.build(pats), OracleEngine(b, pats)
    sb = device_batch(eng, docs, unicode_mappings=True)
    combos = [(Order.Unsorted, Overlap.Keep), (Order.Default, Overlap.NonOverlapping), (Order.Default, Overlap.Keep)]
    uni = 0
    for _ in range(12):
        check_batch(eng, orc, docs, thr, combos=combos, sb=sb)
        uni += sum(not d.isascii() for d in docs)
        docs = cases.mapping_batch(rng, cases.DIFF_SEEDS[2][1])[2]
        assert device_batch(eng, docs, reuse=sb) is sb
    assert uni > 0


@pytest.mark.parametrize("budget,width", [(5, 4), (40, 8)])
def test_auto_beam_takes_the_per_segment_loop(budget, width):
    """An auto-beam engine with mappings: the batch's descriptors are read back and every document runs
    the per-segment loop, its running total restarting at each document."""
    rng = cases.Rng(0x5EED_B005 ^ budget)
    crossed = uni = 0
    for _ in range(15):
        b, pats, docs, thr = cases.mapping_batch(rng, cases.DIFF_SEEDS[2][1], allow_beam=False)
        b = b.auto_beam(budget, width)
        eng, orc = b.build(pats), OracleEngine(b, pats)
        check_batch(eng, orc, docs, thr, combos=[(Order.Unsorted, Overlap.Keep), (Order.Default, Overlap.NonOverlapping)],
                    sb=opted_in(eng, docs))
        plain = OracleEngine(b.auto_beam(2 ** 64 - 1, width), pats)
        crossed += sum(sorted(plain.raw_rows(d, thr)) != sorted(orc.raw_rows(d, thr)) for d in docs if not d.isascii())
        uni += sum(not d.isascii() for d in docs)
        b.auto_beam(budget, width)
    assert crossed > 0 and uni > 0  # the beam did switch on inside some non-ASCII documents
