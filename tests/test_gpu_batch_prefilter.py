"""Pre-filtered batches (fac_search_batch_prefiltered, fac_replace_batch_prefiltered,
fac_batch_prefilter_windows): per document exactly engine.with_prefilter().search(doc, opts) of the
crate. Every expected value comes from the CPU oracle applied to each document alone:
OracleEngine.prefilter_windows(doc, thr), raw_rows(doc, thr, prefilter=True) and apply_rows -- never
from the plain batch, whose result differs for auto-beam engines (test 3)."""
import re

import numpy as np
import pytest

import test_gpu_batch as tgb
from fuzzy_aho_corasick import (DeviceError, FuzzyAhoCorasickBuilder as B, FuzzyLimits as L, Order, Overlap,
                                ReplacementTable, SearchOptions as O, StagedBatch, UnsupportedConfiguration, _native,
                                batch_offsets)
from oracle_harness import OracleEngine
from test_gpu_batch import ASCII_FILLER, ASCII_VOCAB, Rng, canon, random_batch, set_knobs, sim_bits
from test_gpu_replace_batch import REPS, normalised, options, splice

pytestmark = pytest.mark.gpu

# patterns of 4-8 characters, edits(1): with swaps allowed one edit is up to two unit edits
# (k_from_limits, prefilter.rs:388-405), so k = 2 and every piece has m / (k + 1) < 3 symbols: the packed
# full scan takes them all
PACKED_PATS = ["hello", "world", "cell", "abcdefg", "saddam", "hussein8"]
PACKED_THR = 0.75
# patterns of 10-16 characters, edits(1), threshold 0.85: pieces of 3-5 symbols, every pattern on the q-gram path
QGRAM_PATS = ["vestibulum", "consectetur", "adipiscing elit", "lorem ipsum dolo", "pellentesque"]
QGRAM_THR = 0.85
# both paths in one engine, one coverage bitmap
MIXED_PATS = PACKED_PATS + QGRAM_PATS
MIXED_THR = 0.8
ENGINES = {"packed": (PACKED_PATS, PACKED_THR), "qgram": (QGRAM_PATS, QGRAM_THR), "mixed": (MIXED_PATS, MIXED_THR)}
FILL = "zq0 "  # no symbol of any pattern


def packed_builder():
    return B().fuzzy(L().edits(1)).case_insensitive(True)


def fill(rng, n):
    return "".join(FILL[rng.next() % len(FILL)] for _ in range(n))


def near(rng, p):
    """p, or p with one substitution by a filler symbol (still within one edit)."""
    if rng.next() % 2:
        return p
    i = rng.next() % len(p)
    return p[:i] + "z" + p[i + 1:]


def boundary_docs(pats, shift, seed):
    """Document boundaries at global bytes 32, 64, 4096 and 4096 + 87 (+ shift): the coverage words,
    the scan's 64-symbol loads, its 4096-symbol segments and their 87-symbol warm-up. At every cut one
    pattern occurrence ends exactly at the cut and another starts exactly after it. Then the edge
    documents: a pattern cut in two by a boundary, a near-match missing its first symbol at a document
    start (its coverage would reach m + k back), documents shorter than every pattern, 0-3 byte
    documents, empty documents between two matching ones, and one document of 20 KiB."""
    rng = Rng(seed)
    cuts = [0, 32 + shift, 64 + shift, 4096 + shift, 4096 + 87 + shift]
    docs = []
    for a, b in zip(cuts, cuts[1:]):
        head = near(rng, pats[rng.next() % len(pats)]) if a else ""
        tail = near(rng, pats[rng.next() % len(pats)])
        body = b - a - len(head) - len(tail)
        assert body >= 0, (a, b, head, tail)
        docs.append(head + fill(rng, body) + tail)
    docs.append(near(rng, pats[0]) + fill(rng, 9))  # an occurrence right after the last cut
    p = pats[1]
    docs += [fill(rng, 5) + p[:len(p) // 2], p[len(p) // 2:] + fill(rng, 7)]  # cut in two
    docs += [p[1:] + fill(rng, 30), "z" + p[2:] + fill(rng, 3), p[:-1], fill(rng, 2) + p]  # clamped at the start
    docs += ["", "h", "he", "hel", p[:3], ""]
    docs += [pats[0], "", "", "", pats[0], ""]  # touching occurrences around empty documents
    long = []
    while sum(map(len, long)) < 20 * 1024:
        long.append(near(rng, pats[rng.next() % len(pats)]) if rng.next() % 5 == 0 else fill(rng, 1 + rng.next() % 90))
    docs.append("".join(long))
    docs += [pats[-1], pats[-1]]
    assert all(d.isascii() for d in docs)
    off = batch_offsets([d.encode() for d in docs])[1]
    assert off[1:5] == cuts[1:] and len(docs[-3]) >= 20 * 1024
    return docs


def oracle_windows(orc, docs, thr):
    """(document, start, end) of the oracle's merged windows, ends clamped to the document."""
    out = []
    for d, doc in enumerate(docs):
        ws = orc.prefilter_windows(doc, thr)
        assert ws is not None
        out += [(d, s, min(e, len(doc))) for s, e in ws]
    return out


def diag_line(capfd):
    err = capfd.readouterr().err
    m = re.findall(r"FAC_BATCH_PF .*full-scan words=(\d+) qgram patterns=(\d+)/(\d+)", err)
    assert m, err
    return tuple(int(x) for x in m[-1])


def staged(eng, docs):
    return StagedBatch(eng, *batch_offsets([d.encode("utf-8") for d in docs]))


# ---------------------------------------------------------------- 1. windows per document

@pytest.mark.parametrize("shift", [-1, 0, 1])
@pytest.mark.parametrize("which", ["packed", "qgram", "mixed"])
def test_windows_per_document(which, shift, monkeypatch, capfd):
    monkeypatch.setenv("FAC_RC_DEBUG", "1")
    pats, thr = ENGINES[which]
    b = packed_builder()
    eng, orc = b.build(pats), OracleEngine(b, pats)
    docs = boundary_docs(pats, shift, 0xB0D5 + shift)
    want = oracle_windows(orc, docs, thr)
    sb = staged(eng, docs)
    got = sb.prefilter_windows(thr)
    words, qpat, npat = diag_line(capfd)
    assert npat == len(pats)
    if which == "qgram":
        assert words == 0 and qpat == npat
    elif which == "packed":
        assert words > 0 and qpat == 0
    else:
        assert words > 0 and qpat == len(QGRAM_PATS)
    assert got == want
    # the two occurrences at every cut are two windows, and most documents have one
    ends = {(d, e) for d, _, e in want}
    starts = {(d, s) for d, s, _ in want}
    for d in range(4):
        assert (d, len(docs[d])) in ends and (d + 1, 0) in starts, d
    assert sum(len(orc.prefilter_windows(docs[d], thr)) == 0 for d in range(len(docs))) >= 6


def test_no_candidate_at_all():
    b = packed_builder()
    for pats, thr in ((PACKED_PATS, PACKED_THR), (QGRAM_PATS, QGRAM_THR)):
        eng = b.build(pats)
        rng = Rng(0x2e20)
        docs = [fill(rng, rng.next() % 200) for _ in range(70)] + ["", fill(rng, 5000)]
        sb = staged(eng, docs)
        assert sb.prefilter_windows(thr) == []
        st = _native.fac_stats()
        recs, doc_off = sb.search_records(O().threshold(thr), prefilter=True, stats=st)
        assert len(recs) == 0 and list(doc_off) == [0] * (len(docs) + 1) and st.windows == 0


# ---------------------------------------------------------------- 2. records

def got_rows(recs, doc_off, d):
    return [(int(r["start"]), int(r["end"]), int(r["pattern_index"]), sim_bits(float(r["similarity"])),
             int(r["insertions"]), int(r["deletions"]), int(r["substitutions"]), int(r["swaps"]), int(r["edits"]))
            for r in recs[int(doc_off[d]):int(doc_off[d + 1])]]


def check_prefiltered(eng, orc, docs, thr, combos=None, sb=None, count_windows=True):
    """search_records(prefilter=True) == FuzzyMatches::apply of the oracle's Prefiltered::raw, per
    document; stats.windows == the oracle's merged-window lengths (the filter ran), or every start
    window where the reference falls back (count_windows=False for auto-beam engines, whose second,
    beamed pass over the windows after the switch counts again)."""
    sb = sb or staged(eng, docs)
    raw = [orc.raw_rows(doc, thr, prefilter=True) for doc in docs]  # (sorted by (start, end, pattern): Prefiltered::raw)
    wins = [orc.prefilter_windows(doc, thr) for doc in docs]
    if docs and wins[0] is None:
        want_windows = sum(len(d) for d in docs)
        assert all(w is None for w in wins)
    else:
        want_windows = sum(min(e, len(doc)) - s for doc, ws in zip(docs, wins) for s, e in ws)
    for order, overlap in (combos or [(o, v) for o in Order for v in Overlap]):
        opts = options(thr, order, overlap)
        st = _native.fac_stats()
        recs, doc_off = sb.search_records(opts, prefilter=True, stats=st)
        assert len(doc_off) == len(docs) + 1 and doc_off[0] == 0 and doc_off[-1] == len(recs)
        assert not count_windows or st.windows == want_windows, (st.windows, want_windows)
        for d, doc in enumerate(docs):
            rows = orc.apply_rows(raw[d], order, overlap)
            want = [(r[0], r[1], r[2], sim_bits(r[3])) + tuple(r[4:]) for r in rows]
            got = got_rows(recs, doc_off, d)
            assert canon(got, order, overlap) == canon(want, order, overlap), (order, overlap, d, doc)
            if overlap != Overlap.Keep:
                assert [r[0] for r in got] == sorted(r[0] for r in got)
    return sb


@pytest.mark.parametrize("which", ["packed", "qgram", "mixed"])
def test_records_on_the_boundary_batch(which):
    pats, thr = ENGINES[which]
    b = packed_builder()
    eng, orc = b.build(pats), OracleEngine(b, pats)
    docs = boundary_docs(pats, 0, 0xB0D5)
    sb = check_prefiltered(eng, orc, docs, thr)
    assert len(sb.search_records(O().threshold(thr), prefilter=True)[0]) > 20


def random_ascii_batch(rng):
    """random_batch's draws (the engine's included) with every document from the ASCII filler."""
    saved = tgb.FILLERS
    tgb.FILLERS = [ASCII_FILLER] * 3
    try:
        return random_batch(rng, ASCII_VOCAB)
    finally:
        tgb.FILLERS = saved


PF_SEEDS = [0x1234_5678_9abc_def1, 0x0a57_2a1c_0de5_51de]
N_BATCHES = 100


@pytest.mark.parametrize("cache", ["off", "k4"])
@pytest.mark.parametrize("seed", PF_SEEDS)
def test_differential(seed, cache, monkeypatch):
    set_knobs(monkeypatch, cache, False)
    rng = Rng(seed)
    total = filtered = 0
    for _ in range(N_BATCHES):
        b, pats, docs, thr = random_ascii_batch(rng)
        eng, orc = b.build(pats), OracleEngine(b, pats)
        sb = check_prefiltered(eng, orc, docs, thr)
        total += len(sb.search_records(O().threshold(thr), prefilter=True)[0])
        filtered += orc.prefilter_windows(docs[0], thr) is not None
    assert total > 0 and filtered > N_BATCHES // 2


# ---------------------------------------------------------------- 3. auto-beam

AB_DOC = "xx hello yyyyyyyyyyyyyyyy hellp zzzzzzzzzzzzzzzz hallo wwwwwwwwwwwwwwww hello"


@pytest.mark.parametrize("budget", [20, 40])
def test_auto_beam_restarts_per_merged_window(budget):
    """A merged window is its own search_raw call: the running total of search.rs:1096-1103 restarts
    there, so the pre-filtered result (8 records) is not the plain one (7)."""
    b = B().fuzzy(L().edits(1)).auto_beam(budget, 2)
    eng, orc = b.build(["hello"]), OracleEngine(b, ["hello"])
    assert orc.prefilter_windows(AB_DOC, 0.8) == [(0, 10), (22, 32), (46, 55), (68, 77)]
    want_pf, want_plain = orc.raw_rows(AB_DOC, 0.8, prefilter=True), orc.raw_rows(AB_DOC, 0.8)
    assert (len(want_pf), len(want_plain)) == (8, 7)
    docs = [AB_DOC, AB_DOC, "", AB_DOC]
    sb = check_prefiltered(eng, orc, docs, 0.8, count_windows=False)
    recs, doc_off = sb.search_records(O().threshold(0.8), prefilter=True)
    assert list(doc_off) == [0, 8, 16, 16, 24]
    plain, plain_off = sb.search_records(O().threshold(0.8))
    assert list(plain_off) == [0, 7, 14, 14, 21]
    key = lambda rows: sorted((r[0], r[1], r[2], sim_bits(r[3])) + tuple(r[4:]) for r in rows)  # noqa: E731
    assert sorted(got_rows(plain, plain_off, 0)) == key(want_plain)
    assert sorted(got_rows(recs, doc_off, 3)) == key(want_pf)


# ---------------------------------------------------------------- 4. fallback

def test_fallback_is_the_plain_batch():
    """No filter (an engine with a mapping), or k_for above 24 for some pattern (no edit limit, so a
    30-symbol pattern's budget at threshold 0.6 comes from the penalties alone): the call is the plain
    batch call, prefilter_windows returns None, and a batch that mixes is_ascii is accepted."""
    long_pat = "abcdefghijklmnopqrstuvwxyz0123"
    docs = ["strasse hello", "straße", "", "no match here", "hello strase", long_pat + " hallo"]
    assert not docs[1].isascii()
    bm = B().fuzzy(L().edits(1)).mapping("ss", "ß")
    for b, pats, thr, batch in ((bm, ["strasse", "hello"], 0.7, docs[:1] + docs[2:]), (B(), [long_pat, "hello"], 0.6, docs)):
        eng, orc = b.build(pats), OracleEngine(b, pats)
        assert orc.prefilter_windows("hello", thr) is None
        sb = staged(eng, batch)
        assert sb.prefilter_windows(thr) is None
        for order, overlap in ((Order.Unsorted, Overlap.Keep), (Order.Default, Overlap.NonOverlapping)):
            opts = options(thr, order, overlap)
            a, a_off = sb.search_records(opts, prefilter=True)
            p, p_off = sb.search_records(opts)
            assert len(a) >= 3 and list(a_off) == list(p_off)
            assert sorted(a.tobytes()[i:i + 32] for i in range(0, 32 * len(a), 32)) == \
                sorted(p.tobytes()[i:i + 32] for i in range(0, 32 * len(p), 32))
            if order != Order.Unsorted:
                assert a.tobytes() == p.tobytes()


# ---------------------------------------------------------------- 5. limits and errors

def test_limits_and_errors():
    import torch
    b = packed_builder()
    eng, orc = b.build(PACKED_PATS), OracleEngine(b, PACKED_PATS)
    table = ReplacementTable(eng, ["<%d>" % i for i in range(len(PACKED_PATS))])
    opts = O().threshold(PACKED_THR).sorted().non_overlapping()
    mixed = staged(eng, ["hello world", "wörld hello", "cell"])
    buf = torch.full((64 * 32,), 0xAB, dtype=torch.uint8, device="cuda")
    with pytest.raises(UnsupportedConfiguration):
        mixed.search_records(opts, prefilter=True, out=buf)
    with pytest.raises(UnsupportedConfiguration):
        mixed.replace_bytes(table, opts, prefilter=True, out=buf)
    with pytest.raises(UnsupportedConfiguration):
        mixed.prefilter_windows(PACKED_THR)
    assert bool((buf == 0xAB).all())  # nothing written
    assert len(mixed.search_records(opts)[0]) > 0  # the plain call still takes the batch
    docs = ["hello world", "", "helo wrld hello", "cell abcdefg", "zz"]
    sb = check_prefiltered(eng, orc, docs, PACKED_THR, combos=[(Order.Default, Overlap.NonOverlapping)])
    want, want_off = sb.search_records(opts, prefilter=True)
    n = len(want)
    assert n > 2
    small = torch.full(((n - 1) * 32,), 0xAB, dtype=torch.uint8, device="cuda")
    with pytest.raises(DeviceError) as ei:
        sb.search_records(opts, prefilter=True, out=small)
    assert ei.value.code == _native.FAC_E_OUTPUT_CAPACITY and ei.value.needed == n
    assert bool((small == 0xAB).all())
    exact = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    dev_off = torch.full((len(docs) + 1,), -1, dtype=torch.int64, device="cuda")
    got, got_off = sb.search_records(opts, prefilter=True, out=exact, doc_offsets_out=dev_off)
    assert got.cpu().numpy().tobytes() == want.tobytes() and list(got_off) == list(want_off)
    assert dev_off.cpu().tolist() == [int(x) for x in want_off]


def test_restaging_in_place_rebuilds_the_document_starts():
    import torch
    b = packed_builder()
    eng, orc = b.build(PACKED_PATS), OracleEngine(b, PACKED_PATS)
    first = ["hello", "hello world", "", "zzcell"]
    second = ["hellohello", "", "worldz", "q", "abcdefg hussein8"]  # other cuts over bytes the first batch fused
    keep, sb = [], None
    for which in (0, 1, 0):
        docs = (first, second)[which]
        data, off = batch_offsets([d.encode() for d in docs])
        t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
        o = torch.from_numpy(np.asarray(off, dtype=np.uint64).view(np.int64).copy()).cuda()
        keep.append((t, o))
        sb = StagedBatch.from_device(eng, t.data_ptr(), o.data_ptr(), len(off) - 1, len(data), reuse=sb)
        assert sb.prefilter_windows(PACKED_THR) == oracle_windows(orc, docs, PACKED_THR)
        check_prefiltered(eng, orc, docs, PACKED_THR, combos=[(Order.Default, Overlap.NonOverlapping)], sb=sb)


# ---------------------------------------------------------------- 6. Python conveniences

def full_rows(ms):
    return [(m.start, m.end, m.pattern_index, m.sim_bits(), m.insertions, m.deletions, m.substitutions, m.swaps, m.edits,
             m.text) for m in ms]


def test_python_conveniences_take_mixed_input():
    b = B().fuzzy(L().edits(1)).case_insensitive(True)
    pats = ["hello", "wörld", "cell"]
    eng = b.build(pats)
    pf = eng.with_prefilter()
    assert pf.is_active()
    texts = ["hello wörld", "HELLO cell", "", "wôrld", "say helo to the cell", "é", "zz"]
    for opts in (O().threshold(0.7), O().threshold(0.7).sorted().non_overlapping()):
        got = pf.search_batch(texts, opts)
        want = [pf.search(t, opts) for t in texts]
        key = (lambda r: r) if opts.order_ != Order.Unsorted else sorted
        assert [key(full_rows(g)) for g in got] == [key(full_rows(w)) for w in want]
        assert sum(len(g) for g in got) > 4
    reps = ["HI", None, ""]
    opts = O().threshold(0.7)
    order, overlap = Order.Default, Overlap.NonOverlapping
    want = [eng._search_ranked(t, 0.7, order, overlap, prefilter=True).replace(lambda m: reps[m.pattern_index])
            for t in texts]
    assert pf.replace_batch(texts, opts, reps) == want
    assert pf.replace_batch(texts, opts, ReplacementTable(eng, reps)) == want
    assert want[0] == "HI wörld" and want[1] == "HI " and pf.replace_batch([], opts, reps) == []


# ---------------------------------------------------------------- 7. replace

def check_replace(eng, orc, docs, reps, opts, sb=None, table=None):
    """replace_bytes(prefilter=True) == the loop of matches.rs:170-187 over this call's own
    pre-filtered records (every document), == the same loop over the oracle's pre-filtered, applied
    rows wherever a document's kept rows have distinct starts. Returns (outputs, compared, ties)."""
    enc = [d.encode("utf-8") for d in docs]
    sb = sb or StagedBatch(eng, *batch_offsets(enc))
    table = table or ReplacementTable(eng, reps)
    out, off = sb.replace_bytes(table, opts, prefilter=True)
    assert isinstance(out, bytes) and len(off) == len(enc) + 1 and off[0] == 0 and int(off[-1]) == len(out)
    got = [out[int(off[d]):int(off[d + 1])] for d in range(len(enc))]
    n = normalised(opts)
    recs, doc_off = sb.search_records(n, prefilter=True)
    applied = compared = ties = 0
    for d, doc in enumerate(enc):
        rows = [(int(r["start"]), int(r["end"]), int(r["pattern_index"])) for r in recs[int(doc_off[d]):int(doc_off[d + 1])]]
        want, k = splice(doc, rows, reps)
        applied += k
        assert got[d] == want, (d, doc, rows, reps)
        if orc is not None:
            kept = orc.apply_rows(orc.raw_rows(docs[d], n.threshold_, prefilter=True), n.order_, n.overlap_)
            if len({r[0] for r in kept}) != len(kept):
                ties += 1
                continue
            assert got[d] == splice(doc, [r[:3] for r in kept], reps)[0], (d, doc, kept, reps)
            compared += 1
    assert sb.replaced == applied
    return got, compared, ties


@pytest.mark.parametrize("builder,pairs,thr,texts", [
    (lambda: B().case_insensitive(True),  # tests.rs:436-450
     [("PUBLIC JOINT STOCK COMPANY", "PJSC"), ("PUBLIC JOINT STOCK", "PJSC"), ("LIMITED LIABILITY COMPANY", "LLC"),
      ("LIMITED LIABILITY", "LLC")], 0.8, ["PUBLIC JOINT STOCK COMPANY GAZPROM", "limited liability company x", "GAZPROM"]),
    (lambda: B().fuzzy(L().substitutions(1)).case_insensitive(True), [("foo", "bar"), ("baz", "qux")], 0.7,  # tests.rs:513-524
     ["fo0 and BAZ!", "", "BAZ fo0"]),
    (lambda: B().fuzzy(L().edits(5)).case_insensitive(True), [("CZECHOSLOVAKIA", "SERBIA")], 0.7,  # tests.rs:526-537
     ["CHEKHOSLOVAKIA", "in CHEKHOSLOVAKIA."]),
])
def test_replacer_cases_as_one_batch(builder, pairs, thr, texts):
    pats, reps = [p for p, _ in pairs], [r for _, r in pairs]
    eng, orc = builder().build(pats), OracleEngine(builder(), pats)
    got, compared, ties = check_replace(eng, orc, texts, reps, O().threshold(thr))
    assert compared == len(texts) and ties == 0
    assert got[0] in (b"PJSC GAZPROM", b"bar and qux!", b"SERBIA")


def test_replace_alignment_sweep():
    """Gap and replacement boundaries at every output offset mod 16 (prefix documents of 0-17 bytes
    before a matching one, replacement lengths 0-17), through the pre-filtered records."""
    b = B()
    eng, orc = b.build(["hello"]), OracleEngine(b, ["hello"])
    opts = O().threshold(0.9)
    out_res = set()
    for q in range(18):
        docs = []
        for p in range(18):
            docs += ["z" * p, "ab hello cd hello"]
        got, compared, ties = check_replace(eng, orc if q == 3 else None, docs, ["R" * q], opts)
        assert q != 3 or (compared == len(docs) and ties == 0)
        out = 0
        for d, g in zip(docs, got):
            if d.startswith("ab"):
                assert g == b"ab " + b"R" * q + b" cd " + b"R" * q
                out_res |= {(out + 3) % 16, (out + 3 + q) % 16, (out + 7 + q) % 16, (out + 7 + 2 * q) % 16}
            out += len(g)
    assert out_res == set(range(16))


REPLACE_BATCHES = 40


def test_replace_random_differential():
    """The first 40 batches of each seed of test 2, a random replacement per pattern, Default x
    {NonOverlapping, NonOverlappingUnique}. At most 5 % of the document-cases may be tied."""
    compared = ties = replaced = 0
    for seed in PF_SEEDS:
        rng, rrng = Rng(seed), Rng(seed ^ 0x5e9_1ace)
        for _ in range(REPLACE_BATCHES):
            b, pats, docs, thr = random_ascii_batch(rng)
            reps = [REPS[rrng.next() % len(REPS)] for _ in pats]
            eng, orc = b.build(pats), OracleEngine(b, pats)
            sb = staged(eng, docs)
            table = ReplacementTable(eng, reps)
            for overlap in (Overlap.NonOverlapping, Overlap.NonOverlappingUnique):
                _, c, t = check_replace(eng, orc, docs, reps, options(thr, overlap=overlap), sb=sb, table=table)
                compared += c
                ties += t
                replaced += sb.replaced
    share = ties / (compared + ties)
    print(f"oracle-compared {compared}, excluded as ties {ties} ({100 * share:.2f} %), records applied {replaced}")
    assert share <= 0.05 and replaced > 0
