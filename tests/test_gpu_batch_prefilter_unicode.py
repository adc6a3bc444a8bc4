"""Pre-filtered batches that hold non-ASCII documents (fac_batch_allow_unicode_prefilter): per
document exactly engine.with_prefilter().search(doc, opts) of the crate, whatever its neighbours
are. Every expected value comes from the CPU oracle applied to each document alone --
OracleEngine.prefilter_windows(doc, thr), raw_rows(doc, thr, prefilter=True) and apply_rows -- never
from the plain batch or from the device. test_batch_prefilter_unicode_host.py checks on the oracle
alone that the documents used here hold the cases the comparisons are about."""
import re

import numpy as np
import pytest

import batch_unicode_cases as cases
import test_gpu_batch_prefilter as tpf
import test_gpu_segment_batch as tsb
import test_gpu_template_extract as tte
from fuzzy_aho_corasick import (DeviceError, FuzzyAhoCorasickBuilder as B, FuzzyLimits as L, Order, Overlap,
                                ReplacementTable, SearchOptions as O, StagedBatch, UnsupportedConfiguration, Wrap, _native,
                                batch_offsets)
from oracle_harness import OracleEngine, graphemes
from test_gpu_batch import set_knobs
from test_gpu_replace_batch import options

pytestmark = pytest.mark.gpu

COMBOS = [(o, v) for o in Order for v in Overlap]  # what check_prefiltered uses by default
DEFAULT = [(Order.Default, Overlap.NonOverlapping)]


def builder():
    return B().fuzzy(L().edits(1)).case_insensitive(True)


def staged(eng, docs, opt_in=True):
    return StagedBatch(eng, *batch_offsets([d.encode("utf-8") for d in docs]), unicode_prefilter=opt_in)


def diag(capfd):
    """(full-scan words, q-gram patterns, patterns, documents, unicode) of the last FAC_BATCH_PF line."""
    err = capfd.readouterr().err
    m = re.findall(r"FAC_BATCH_PF docs=(\d+) .*full-scan words=(\d+) qgram patterns=(\d+)/(\d+) .*unicode=(\d)", err)
    assert m, err
    docs, words, qpat, npat, uni = (int(x) for x in m[-1])
    return words, qpat, npat, docs, uni


def check_records(eng, orc, docs, thr, combos=None, sb=None):
    """check_prefiltered on an opted-in batch. stats.windows is compared here: the start windows
    searched are the merged windows' lengths, a window of a non-ASCII document counted in bytes where
    its slice is all ASCII (it is searched byte-wise) and in graphemes where it is not."""
    sb = sb or staged(eng, docs)
    tpf.check_prefiltered(eng, orc, docs, thr, combos=combos, sb=sb, count_windows=False)
    want = 0
    for d, s, e in cases.oracle_windows(orc, docs, thr):
        raw = cases.window_bytes(docs[d], s, e)
        want += len(raw) if raw.isascii() else e - s
    st = _native.fac_stats()
    sb.search_records(O().threshold(thr), prefilter=True, stats=st)
    assert st.windows == want, (st.windows, want)
    return sb


# ---------------------------------------------------------------- 1. default off

def test_default_off():
    import torch
    eng = builder().build(cases.ENGINES["packed"][0])
    thr = cases.ENGINES["packed"][1]
    table = ReplacementTable(eng, ["<%d>" % i for i in range(len(eng.patterns_))])
    opts = O().threshold(thr).sorted().non_overlapping()
    sb = staged(eng, ["hello world", "wörld hello", "cell"], opt_in=False)
    buf = torch.full((64 * 32,), 0xAB, dtype=torch.uint8, device="cuda")
    calls = [lambda: sb.search_records(opts, prefilter=True, out=buf),
             lambda: sb.replace_bytes(table, opts, prefilter=True, out=buf),
             lambda: sb.extract(table, opts, records_out=buf, text_out=buf[:256], prefilter=True),
             lambda: sb.segment_records(opts, prefilter=True, out=buf),
             lambda: sb.render_bytes(_native.FAC_RENDER_SEGMENT_TEXT, opts, prefilter=True, out=buf),
             lambda: sb.prefilter_windows(thr)]

    def refused():
        for call in calls:
            with pytest.raises(UnsupportedConfiguration):
                call()
        assert bool((buf == 0xAB).all())  # nothing written

    refused()
    assert sb.allow_unicode_prefilter() is sb
    for call in calls:
        call()
    assert len(sb.search_records(opts, prefilter=True)[0]) >= 4 and sb.prefilter_windows(thr)
    buf.fill_(0xAB)
    sb.allow_unicode_prefilter(False)
    refused()


# ---------------------------------------------------------------- 2. windows per document

@pytest.mark.parametrize("shift", [-1, 0, 1])
@pytest.mark.parametrize("which", ["packed", "qgram", "mixed"])
def test_windows_per_document(which, shift, monkeypatch, capfd):
    monkeypatch.setenv("FAC_RC_DEBUG", "1")
    pats, thr = cases.ENGINES[which]
    eng, orc = builder().build(pats), OracleEngine(builder(), pats)
    docs = cases.boundary_docs(pats, shift, 0xB0D5 + shift)
    sb = staged(eng, docs)
    got = sb.prefilter_windows(thr)
    words, qpat, npat, ndocs, uni = diag(capfd)
    assert (npat, ndocs, uni) == (len(pats), len(docs), 1)
    if which == "qgram":
        assert words == 0 and qpat == npat
    elif which == "packed":
        assert words > 0 and qpat == 0
    else:
        assert words > 0 and qpat == cases.N_QGRAM
    assert got == cases.oracle_windows(orc, docs, thr)
    for batch in cases.small_batches(pats):
        assert staged(eng, batch).prefilter_windows(thr) == cases.oracle_windows(orc, batch, thr), batch


@pytest.mark.parametrize("which", ["packed", "qgram", "mixed"])
def test_records_on_the_boundary_batch(which):
    pats, thr = cases.ENGINES[which]
    eng, orc = builder().build(pats), OracleEngine(builder(), pats)
    docs = cases.boundary_docs(pats, 0, 0xB0D5)
    sb = check_records(eng, orc, docs, thr, combos=DEFAULT + [(Order.Unsorted, Overlap.Keep)])
    assert len(sb.search_records(O().threshold(thr), prefilter=True)[0]) > 40
    for batch in cases.small_batches(pats):
        check_records(eng, orc, batch, thr, combos=DEFAULT)


# ---------------------------------------------------------------- 3. slices

def test_slices():
    eng, orc = builder().build(cases.SLICE_PATS), OracleEngine(builder(), cases.SLICE_PATS)
    docs = cases.slice_docs()
    sb = staged(eng, docs)
    assert sb.prefilter_windows(cases.SLICE_THR) == cases.oracle_windows(orc, docs, cases.SLICE_THR)
    check_records(eng, orc, docs, cases.SLICE_THR, sb=sb)
    # between ASCII neighbours too: the same documents, every other one followed by an ASCII one
    mixed = [x for d in docs for x in (d, "zz hello zz")]
    check_records(eng, orc, mixed, cases.SLICE_THR, combos=DEFAULT)


# ---------------------------------------------------------------- 4. all five result calls

ALL_DOCS = ["hello wörld", "", "zq0 helo zq0 wrld hello", "москва cell abcdefg", "zz", "ж" * 70 + "HELLO\r\nWORLD",
            "cafés in 東京都庁", "  wörld москва  ", "é", "Москва, hello; cafés!", "q" * 300 + "HELLO", "東京都庁"]


def test_all_result_calls():
    import torch
    pats, thr = cases.ENGINES["packed"]
    eng, orc = builder().build(pats), OracleEngine(builder(), pats)
    docs = ALL_DOCS
    sb = check_records(eng, orc, docs, thr)  # search: every order x overlap, bit-exact
    assert not sb.search_records(O().threshold(thr), prefilter=True)[0]["pad"].tobytes().strip(b"\0")
    n = len(pats)
    plain = [["", "X", "«é»", "😀", "0123456789abcdefghij"][i % 5] for i in range(n)]
    keep = [None if i % 2 else plain[i] for i in range(n)]
    templ = [Wrap("<b>", "</b>") if i % 3 == 0 else (None if i % 3 == 1 else "R%d" % i) for i in range(n)]
    opts = options(thr)
    for reps in (plain, keep):  # replace == the splice of the oracle's kept rows
        _, compared, ties = tpf.check_replace(eng, orc, docs, reps, opts, sb=sb)
        assert compared + ties == len(docs) and ties <= 2
    ttab = ReplacementTable(eng, templ)
    recs, doc_off = sb.search_records(opts, prefilter=True)  # (pinned to the oracle above)
    out, off = sb.replace_bytes(ttab, opts, prefilter=True)
    for d, doc in enumerate(docs):
        raw, want, last = doc.encode("utf-8"), b"", 0
        for r in tte.rows_of(recs[int(doc_off[d]):int(doc_off[d + 1])]):
            if r[0] >= last:
                want += raw[last:r[0]] + tte.item_of(raw, r, templ)
                last = r[1]
        assert out[int(off[d]):int(off[d + 1])] == want + raw[last:], (d, doc)
    for order, overlap in COMBOS:  # extract, with and without a table: items pinned to the pinned records
        o = options(thr, order, overlap)
        a = tte.check_extract(eng, docs, o, None, sb=sb, prefilter=True, references=False)
        b = tte.check_extract(eng, docs, o, templ, sb=sb, table=ttab, prefilter=True, references=False)
        assert sum(len(x) for x in a) == sum(len(x) for x in b) >= 12
    for order, overlap in COMBOS:  # segments and the three render modes
        tsb.check(eng, docs, options(thr, order, overlap), sb=sb, prefilter=True)
    # device output buffers, and FAC_E_OUTPUT_CAPACITY with nothing written
    o = options(thr)
    want, want_off = sb.search_records(o, prefilter=True)
    small = torch.full(((len(want) - 1) * 32,), 0xAB, dtype=torch.uint8, device="cuda")
    with pytest.raises(DeviceError) as ei:
        sb.search_records(o, prefilter=True, out=small)
    assert ei.value.code == _native.FAC_E_OUTPUT_CAPACITY and ei.value.needed == len(want) and bool((small == 0xAB).all())
    exact = torch.empty(len(want) * 32, dtype=torch.uint8, device="cuda")
    dev_off = torch.full((len(docs) + 1,), -1, dtype=torch.int64, device="cuda")
    got, got_off = sb.search_records(o, prefilter=True, out=exact, doc_offsets_out=dev_off)
    assert got.cpu().numpy().tobytes() == want.tobytes() and list(got_off) == list(want_off)
    assert dev_off.cpu().tolist() == [int(x) for x in want_off]
    host, host_off = sb.replace_bytes(ttab, o, prefilter=True)
    short = torch.full((len(host) - 1,), 0xAB, dtype=torch.uint8, device="cuda")
    with pytest.raises(DeviceError) as ei:
        sb.replace_bytes(ttab, o, prefilter=True, out=short)
    assert ei.value.code == _native.FAC_E_OUTPUT_CAPACITY and ei.value.needed == len(host) and bool((short == 0xAB).all())
    buf = torch.full((len(host) + 16,), 0xCD, dtype=torch.uint8, device="cuda")
    g, g_off = sb.replace_bytes(ttab, o, prefilter=True, out=buf[:len(host)])
    assert g.cpu().numpy().tobytes() == host and list(g_off) == list(host_off) and bool((buf[len(host):] == 0xCD).all())
    for mode in tsb.MODES:
        h, h_off = sb.render_bytes(mode, o, prefilter=True)
        buf = torch.full((len(h) + 16,), 0xCD, dtype=torch.uint8, device="cuda")
        g, g_off = sb.render_bytes(mode, o, prefilter=True, out=buf[:len(h)])
        assert g.cpu().numpy().tobytes() == h and list(g_off) == list(h_off) and bool((buf[len(h):] == 0xCD).all())
    segs, seg_off = sb.segment_records(o, prefilter=True)
    sbuf = torch.empty(len(segs) * 32, dtype=torch.uint8, device="cuda")
    g, g_off = sb.segment_records(o, prefilter=True, out=sbuf)
    assert g.cpu().numpy().tobytes() == segs.tobytes() and list(g_off) == list(seg_off)


# ---------------------------------------------------------------- 5. random differential

@pytest.mark.parametrize("cache", ["off", "k4"])
@pytest.mark.parametrize("seed", cases.DIFF_SEEDS)
def test_differential(seed, cache, monkeypatch):
    set_knobs(monkeypatch, cache, False)
    eng, orc = builder().build(cases.DIFF_PATS), OracleEngine(builder(), cases.DIFF_PATS)
    docs = cases.random_docs(seed)
    sb = check_records(eng, orc, docs, cases.DIFF_THR)
    assert sb.prefilter_windows(cases.DIFF_THR) == cases.oracle_windows(orc, docs, cases.DIFF_THR)
    reps = [["", "X", "«é»", "😀", "0123456789abcdefghij", None][(seed + i) % 6] for i in range(len(cases.DIFF_PATS))]
    for overlap in (Overlap.NonOverlapping, Overlap.NonOverlappingUnique):
        _, compared, ties = tpf.check_replace(eng, orc, docs, reps, options(cases.DIFF_THR, overlap=overlap), sb=sb)
        assert compared + ties == len(docs) and 4 * ties <= len(docs)


# ---------------------------------------------------------------- 6. auto-beam

AB_DOC = "xx hello ÿÿÿÿÿÿÿÿÿÿÿÿÿÿÿÿ hellp zzzzzzzzzzzzzzzz hallo ÿÿÿÿÿÿÿÿÿÿÿÿÿÿÿÿ hello"


@pytest.mark.parametrize("budget", [20, 40])
def test_auto_beam_restarts_per_merged_window(budget):
    b = B().fuzzy(L().edits(1)).auto_beam(budget, 2)
    eng, orc = b.build(["hello"]), OracleEngine(b, ["hello"])
    assert orc.prefilter_windows(AB_DOC, 0.8) == [(0, 10), (22, 32), (46, 55), (68, 77)]
    want_pf, want_plain = orc.raw_rows(AB_DOC, 0.8, prefilter=True), orc.raw_rows(AB_DOC, 0.8)
    assert len(want_pf) != len(want_plain)  # the running total restarts per merged window
    docs = [AB_DOC, tpf.AB_DOC, "", AB_DOC, "é"]
    sb = staged(eng, docs)
    tpf.check_prefiltered(eng, orc, docs, 0.8, sb=sb, count_windows=False)
    _, doc_off = sb.search_records(O().threshold(0.8), prefilter=True)
    assert int(doc_off[1]) == len(want_pf)


# ---------------------------------------------------------------- 7. fallbacks

def test_fallbacks():
    long_pat = "abcdefghijklmnopqrstuvwxyz0123"
    docs = ["strasse hello", "straße héllo", "", "no match here", "hello strase", long_pat + " hallo"]
    b = B()
    eng, orc = b.build([long_pat, "hello"]), OracleEngine(b, [long_pat, "hello"])
    assert orc.prefilter_windows("hello", 0.6) is None  # k_for above 24
    sb = staged(eng, docs)
    assert sb.prefilter_windows(0.6) is None
    for order, overlap in ((Order.Unsorted, Overlap.Keep), (Order.Default, Overlap.NonOverlapping)):
        opts = options(0.6, order, overlap)
        a, a_off = sb.search_records(opts, prefilter=True)
        p, p_off = sb.search_records(opts)
        assert len(a) >= 3 and list(a_off) == list(p_off)
        assert sorted(r.tobytes() for r in a) == sorted(r.tobytes() for r in p)
    tpf.check_prefiltered(eng, orc, docs, 0.6, combos=DEFAULT, sb=sb)
    bm = B().fuzzy(L().edits(1)).mapping("ss", "ß")
    em = bm.build(["strasse", "hello"])
    msb = staged(em, docs)
    with pytest.raises(UnsupportedConfiguration) as ei:  # fac_search_batch's own refusal
        msb.search_records(O().threshold(0.7), prefilter=True)
    assert "mappings" in str(ei.value)
    with pytest.raises(UnsupportedConfiguration):
        msb.search_records(O().threshold(0.7))


# ---------------------------------------------------------------- 8. restage in place

def test_restaging_in_place_keeps_the_opt_in(monkeypatch, capfd):
    import torch
    monkeypatch.setenv("FAC_RC_DEBUG", "1")
    pats, thr = cases.ENGINES["packed"]
    eng, orc = builder().build(pats), OracleEngine(builder(), pats)
    first = ["hello", "hello world", "", "zzcell"]
    second = ["wörldwörld", "", "hellom", "ж", "москва hello", "abcdefg hussein8"]  # other cuts, other coordinates
    keep, sb = [], None
    for which in (0, 1, 0):
        docs = (first, second)[which]
        data, off = batch_offsets([d.encode("utf-8") for d in docs])
        t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
        o = torch.from_numpy(np.asarray(off, dtype=np.uint64).view(np.int64).copy()).cuda()
        keep.append((t, o))
        sb = StagedBatch.from_device(eng, t.data_ptr(), o.data_ptr(), len(off) - 1, len(data), reuse=sb,
                                     unicode_prefilter=sb is None)
        assert sb.prefilter_windows(thr) == cases.oracle_windows(orc, docs, thr)
        assert diag(capfd)[4] == which  # the all-ASCII batch takes the byte path again
        check_records(eng, orc, docs, thr, combos=DEFAULT, sb=sb)


# ---------------------------------------------------------------- 9. a table that does not fit LDS

def test_symbol_table_out_of_lds():
    marks = [chr(c) for c in range(0x0300, 0x0300 + 60)]
    big = lambda ch, i: ch + "".join(marks[(7 * i + j) % 60] for j in range(58))  # noqa: E731
    pats = ["h" + big("e", i) + "llo" + chr(ord("a") + i % 26) + str(i // 26) for i in range(40)]
    pool = {g.lower() for p in pats for g in graphemes(p)}
    assert sum(len(g) for g in pool) > 2048 and all(len(graphemes(p)) == 7 for p in pats)
    b = builder()
    eng, orc = b.build(pats), OracleEngine(b, pats)
    g3 = graphemes(pats[3])
    docs = ["zz" + pats[0] + "zz", "é" + pats[1].upper(), "hello", "ж" * 9 + "".join(g3[:2] + ["z"] + g3[3:]) + "ж", "",
            pats[39] + "→" + pats[2], "zz " + big("e", 5) + " " + big("e", 77) + " zz"]
    thr = 0.75
    sb = staged(eng, docs)
    assert sb.prefilter_windows(thr) == cases.oracle_windows(orc, docs, thr)
    check_records(eng, orc, docs, thr, combos=DEFAULT, sb=sb)
    assert len(sb.search_records(O().threshold(thr), prefilter=True)[0]) >= 5


# ---------------------------------------------------------------- 10. Python conveniences

def test_conveniences_stage_one_batch(monkeypatch, capfd):
    monkeypatch.setenv("FAC_RC_DEBUG", "1")
    b = builder()
    pats = ["hello", "wörld", "cell", "москва"]
    eng = b.build(pats)
    pf = eng.with_prefilter()
    assert pf.is_active()
    texts = ["hello wörld", "HELLO cell", "", "wôrld", "say helo to the cell", "é", "zz", "  Москва, hello  "]
    opts = O().threshold(0.7).sorted().non_overlapping()
    seg = [pf._segmented(t, opts) for t in texts]
    reps = ["HI", None, "", "M"]

    def one_batch(call):
        capfd.readouterr()
        out = call()
        lines = re.findall(r"FAC_BATCH_PF docs=(\d+) ", capfd.readouterr().err)
        assert lines == [str(len(texts))], lines  # one batch holding all the texts
        return out

    got = one_batch(lambda: pf.search_batch(texts, opts))
    assert [tpf.full_rows(g) for g in got] == [tpf.full_rows(pf.search(t, opts)) for t in texts]
    assert sum(len(g) for g in got) > 6
    assert one_batch(lambda: pf.replace_batch(texts, opts, reps)) == [m.replace(lambda x: reps[x.pattern_index]) for m in seg]
    assert one_batch(lambda: pf.extract_batch(texts, opts)) == [m.matched_strings() for m in seg]
    assert one_batch(lambda: pf.strip_prefix_batch(texts, opts)) == [m.strip_prefix() for m in seg]
    assert one_batch(lambda: pf.strip_suffix_batch(texts, opts)) == [m.strip_suffix() for m in seg]
    assert one_batch(lambda: pf.segment_text_batch(texts, opts)) == [m.segment_text() for m in seg]
    assert one_batch(lambda: pf.split_batch(texts, opts)) == [list(m.split()) for m in seg]
    segs = one_batch(lambda: pf.segment_batch(texts, opts))
    want = [list(m.segment_iter()) for m in seg]
    assert [[(x.matched() is not None, x.as_str()) for x in d] for d in segs] == \
        [[(x.matched() is not None, x.as_str()) for x in d] for d in want]
    assert [[x.matched() for x in d if x.matched() is not None] for d in segs] == \
        [[x.matched() for x in d if x.matched() is not None] for d in want]
