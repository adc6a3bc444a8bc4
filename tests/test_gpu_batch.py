"""search_batch / StagedBatch (fac_batch_*, fac_search_batch): N independent documents in one device
pass give, per document, exactly what engine.search(doc, opts) gives for that document alone. Every
expected value comes from the CPU oracle or the host segmenter applied to each document alone."""
import ctypes
import struct

import numpy as np
import pytest

from fuzzy_aho_corasick import (DeviceError, FuzzyAhoCorasickBuilder as B, FuzzyLimits as L, FuzzyPenalties,
                                HaystackTooLarge, Order, Overlap, Pattern, SearchOptions as O, StagedBatch, _native,
                                batch_offsets)
from oracle_harness import OracleEngine

pytestmark = pytest.mark.gpu

# adjacent documents whose concatenation would fuse across the cut (UAX #29 GB3, GB9, GB12/13, GB11,
# GB9c, GB6, GB9b)
PAIRS = [("a\r", "\nb"), ("e", "\u0301x"),          # CR | LF, letter | combining acute
         ("\U0001f1e9", "\U0001f1ea\U0001f1eb"),   # regional indicators D | E F
         ("\U0001f469\u200d", "\U0001f4bb"),       # woman ZWJ | laptop
         ("\u0915\u094d", "\u0937"),               # ka virama | ssa (conjunct)
         ("\u1100", "\u1161"),                     # Hangul L | V
         ("x\u0600", "a")]                         # U+0600 ARABIC NUMBER SIGN (Prepend) | letter


def host_starts(data: bytes):
    """search_raw's graphemes of one document alone: bytes when it is ASCII (search.rs:196), else the
    host segmenter's UAX #29 clusters (fac_segment_graphemes)."""
    return list(range(len(data))) if data.isascii() else _native.grapheme_starts(data)


def check_staging(eng, docs):
    enc = [d.encode("utf-8") for d in docs]
    data, off = batch_offsets(enc)
    sb = StagedBatch(eng, data, off)
    assert int(_native.lib.fac_batch_docs(sb._h)) == len(docs)
    for d, raw in enumerate(enc):
        want = host_starts(raw)
        assert sb.doc_graphemes(d) == (len(want), raw.isascii()), (d, docs[d][:40])
        assert sb.grapheme_starts(d) == want, (d, docs[d][:40])


@pytest.fixture(scope="module")
def seg_engine():
    return B().case_insensitive(True).build(["x"])


def test_boundary_segmentation(seg_engine):
    """1. A document start is start-of-text: nothing fuses across a cut."""
    check_staging(seg_engine, [h for pair in PAIRS for h in pair])
    for pair in PAIRS:
        check_staging(seg_engine, list(pair))


def _fill(rng, nbytes):
    pieces = ["a", "\u00e9", "\u0915", "\U0001f600", " ", "\u0301", "b", "\u03c9", "\r\n", "\U0001f1eb", "\u200d"]
    out, left = [], nbytes
    while left >= 4:
        p = pieces[rng.next() % len(pieces)]
        out.append(p)
        left -= len(p.encode("utf-8"))
    return "".join(out) + "a" * left


@pytest.mark.parametrize("shift", [-1, 0, 1])
def test_tile_and_chunk_cuts(seg_engine, shift):
    """2. Document boundaries at bytes 64 / 256 / 16384 + shift and at 32768 (the segmenter's 64-byte
    thread ranges, 256-byte write steps and 16 KiB tiles), each carrying one of the pairs; one
    document longer than a tile (20 KiB), one empty document between the two halves of a pair. A
    pair needs two bytes on one side, so adjacent byte positions carry pairs in separate batches."""
    rng = Rng(0xC0751 + shift)
    cuts = [0, 64 + shift, 256 + shift, 16384 + shift, 32768, 32768 + 20 * 1024 + 700]
    docs = []
    for k in range(len(cuts) - 1):
        head = PAIRS[k][1] if k > 0 else ""
        tail = PAIRS[k + 1][0]
        body = cuts[k + 1] - cuts[k] - len(head.encode("utf-8")) - len(tail.encode("utf-8"))
        docs.append(head + _fill(rng, body) + tail)
    docs += ["", PAIRS[5][1] + " tail", "a\r", "\nb", "x\u0600", "a"]
    data, off = batch_offsets([d.encode("utf-8") for d in docs])
    assert off[1:6] == cuts[1:] and len(docs[4].encode("utf-8")) > 20 * 1024 and not data.isascii()
    check_staging(seg_engine, docs)


def test_hard_path(seg_engine):
    """3. Runs with no resync point within 1 KiB that start right after a boundary: the regional-
    indicator pairing starts at the document, not at the previous document's indicator."""
    check_staging(seg_engine, ["x\U0001f1e9", "\U0001f1ea" * 601, "\U0001f469" + "\u200d\U0001f469" * 400])


def test_utf8_is_checked_per_document(seg_engine):
    """4. A sequence split by a document boundary makes both documents invalid."""
    data = b"a\xc3" + b"\xa9b"
    with pytest.raises(DeviceError) as ei:
        StagedBatch(seg_engine, data, [0, 2, 4])
    assert ei.value.code == _native.FAC_E_INVALID and ei.value.doc == 0
    sb = StagedBatch(seg_engine, data, [0, 4])
    assert sb.doc_graphemes(0) == (3, False) and sb.grapheme_starts(0) == [0, 1, 3]
    docs = [b"ok", "é".encode(), b"", b"x\xff", b"\x80"]
    with pytest.raises(DeviceError) as ei:
        StagedBatch(seg_engine, *batch_offsets(docs))
    assert ei.value.code == _native.FAC_E_INVALID and ei.value.doc == 3


def sim_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def full_rows(ms):
    return [(m.start, m.end, m.pattern_index, m.sim_bits(), m.insertions, m.deletions, m.substitutions, m.swaps,
             m.edits) for m in ms]


def oracle_doc(orc, doc, thr, order, overlap):
    """FuzzyMatches::apply(order, overlap) of search_raw(doc) by the oracle. Unsorted with an overlap
    mode walks the records in (start, end, pattern) order, the order fac.h gives the batch walk (the
    crate walks its hash map's order there)."""
    raw = orc.raw_rows(doc, thr)
    if order == Order.Unsorted and overlap != Overlap.Keep:
        raw = sorted(raw, key=lambda r: r[:3])
    rows = orc.apply_rows(raw, order, overlap)
    return [(r[0], r[1], r[2], sim_bits(r[3])) + tuple(r[4:]) for r in rows]


def canon(rows, order, overlap):
    """The comparable form of one document's result: the sequence itself for a sorted order kept
    whole; after an overlap resolution the matches are sorted by start alone with an unstable sort
    (matches.rs:111, 148), so equal starts are put in one order; Unsorted+Keep has no order."""
    if overlap != Overlap.Keep:
        return sorted(rows, key=lambda r: (r[0],) + r[1:])
    return list(rows) if order != Order.Unsorted else sorted(rows)


def check_batch(eng, orc, docs, thr, combos=None, sb=None):
    enc = [d.encode("utf-8") for d in docs]
    if sb is None:
        sb = StagedBatch(eng, *batch_offsets(enc))
    for order, overlap in (combos or [(o, v) for o in Order for v in Overlap]):
        opts = O().threshold(thr)
        opts.order_, opts.overlap_ = order, overlap
        recs, doc_off = sb.search_records(opts)
        assert len(doc_off) == len(docs) + 1 and doc_off[0] == 0 and doc_off[-1] == len(recs)
        assert all(doc_off[i] <= doc_off[i + 1] for i in range(len(docs)))
        assert not recs["pad"].tobytes().strip(b"\0")
        for d, doc in enumerate(docs):
            got = [(int(r["start"]), int(r["end"]), int(r["pattern_index"]), sim_bits(float(r["similarity"])),
                    int(r["insertions"]), int(r["deletions"]), int(r["substitutions"]), int(r["swaps"]), int(r["edits"]))
                   for r in recs[int(doc_off[d]):int(doc_off[d + 1])]]
            want = oracle_doc(orc, doc, thr, order, overlap)
            assert canon(got, order, overlap) == canon(want, order, overlap), (order, overlap, d, doc, docs)
            if overlap != Overlap.Keep:  # start order, as the reference leaves it
                assert [r[0] for r in got] == sorted(r[0] for r in got)
    return sb


@pytest.mark.parametrize("thr", [0.0, 0.6])
def test_mixed_is_ascii(thr):
    """5. is_ascii is decided per document: "\\r\\n" is two graphemes in the ASCII documents and one in
    the Unicode one."""
    b = B().fuzzy(L().edits(1))
    pats = ["a\nb", "\r\nb"]
    docs = ["a\r\nb", "é\r\nb", "a\r\nb"]
    eng, orc = b.build(pats), OracleEngine(b, pats)
    sb = check_batch(eng, orc, docs, thr)
    assert [sb.doc_graphemes(d) for d in range(3)] == [(4, True), (3, False), (4, True)]
    per_doc = eng.search_batch(docs, O().threshold(thr))
    assert [sorted(full_rows(m)) for m in per_doc] == [sorted(full_rows(eng.search(d, O().threshold(thr)))) for d in docs]
    assert sorted(full_rows(per_doc[0])) != sorted(full_rows(per_doc[1]))


def test_no_match_across_a_cut_and_exact_attribution():
    """6. Documents are searched alone, and every record lands in its own document with
    document-relative offsets -- also the empty-span matches at a document's end, whose global byte is
    the next document's first."""
    b = B().fuzzy(L().edits(1))
    eng, orc = b.build(["hello"]), OracleEngine(b, ["hello"])
    docs = ["hel", "lo", "hello"]
    check_batch(eng, orc, docs, 0.9)
    res = eng.search_batch(docs, O().threshold(0.9))
    assert [len(r) for r in res][:2] == [0, 0] and len(res[2]) > 0
    assert all(m.start == 0 and m.end == 5 and m.text == "hello" for m in res[2] if m.edits == 0)
    eng, orc = b.build(["a"]), OracleEngine(b, ["a"])
    docs = ["a", "a", ""]
    check_batch(eng, orc, docs, 0.0)
    recs, doc_off = StagedBatch(eng, *batch_offsets([d.encode() for d in docs])).search_records(O().threshold(0.0))
    assert list(doc_off) == [0, len(recs) // 2, len(recs), len(recs)] and len(recs) > 0
    assert all(int(r["end"]) <= 1 for r in recs)
    assert any(int(r["start"]) == int(r["end"]) for r in recs)  # the empty spans are there


class Rng:  # the xorshift of the parity tests (prefilter.rs:441-452)
    def __init__(self, s):
        self.s = s

    def next(self):
        x = self.s
        x ^= (x << 13) & 0xFFFFFFFFFFFFFFFF
        x ^= x >> 7
        x ^= (x << 17) & 0xFFFFFFFFFFFFFFFF
        self.s = x
        return x


ASCII_VOCAB = ["hello", "world", "vestibulum", "abc", "lorem", "cell", "saddam", "hussein", "ab", "x"]
ASCII_FILLER = ["a", "b", "c", "d", "e", " ", "1", "o", "0", "l", "S", "H"]
UNI_VOCAB = ["café", "naïve", "Ωμέγα", "Москва", "señor", "école", "résumé"]
UNI_FILLER = ["a", "é", "ñ", "ω", "м", " ", "o", "0", "é", "Ω", "\r\n", "Σ"]
ASTRAL_VOCAB = ["a😀b", "𝒜bc", "𐍈𐌹𐍈", "x😀y😀", "hello", "b𝒜a"]
ASTRAL_FILLER = ["😀", "𝒜", "a", "b", " ", "𐍈", "c", "x", "𐌹", "y"]
FILLERS = [ASCII_FILLER, UNI_FILLER, ASTRAL_FILLER]


def random_batch(rng, vocab, allow_beam=True):
    """random_case of the parity tests (same draws for the engine), its one haystack replaced by a
    batch of 1-40 documents of 0-60 units, each drawn from the ASCII, Unicode or astral fillers
    independently (so batches mix both grapheme modes), and custom unique ids on some patterns."""
    npat = 1 + rng.next() % 4
    pats = [vocab[rng.next() % len(vocab)] for _ in range(npat)]
    edits = rng.next() % 4
    b = B().case_insensitive(rng.next() & 1 == 0)
    mode = rng.next() % 6
    if edits > 0 and mode != 5:
        b = b.fuzzy(L().edits(edits))
    if mode == 5:  # per-type / per-pattern limits
        b = b.fuzzy(L().insertions(rng.next() % 2).deletions(rng.next() % 2).substitutions(rng.next() % 2)
                    .swaps(rng.next() % 2))
        pats = [Pattern(p).fuzzy(L().edits(rng.next() % 3)) if rng.next() % 2 else p for p in pats]
    if rng.next() % 5 == 0:
        b = b.penalties(FuzzyPenalties.default().with_swap(0.6).with_insertion(0.5).with_deletion(0.8))
    if allow_beam and rng.next() % 4 == 0:
        b = b.beam_width(1 + rng.next() % 12)
    if rng.next() % 7 == 0:
        b = b.min_symbol_similarity(0.3)
    words = [w if isinstance(w, str) else w.pattern for w in pats]
    docs = []
    for _ in range(1 + rng.next() % 40):
        filler = FILLERS[rng.next() % 3]
        doc = ""
        for _ in range(rng.next() % 61):
            if rng.next() % 7 == 0:
                doc += words[rng.next() % len(words)] + " "
            else:
                doc += filler[rng.next() % len(filler)]
        docs.append(doc)
    thr = 0.6 + (rng.next() % 4) * 0.1 if rng.next() % 5 else 0.0
    if rng.next() % 2:  # custom unique ids shared between patterns (matches.rs:118-122)
        pats = [Pattern.from_(p).custom_unique_id(rng.next() % 2) if rng.next() % 2 else p for p in pats]
    return b, pats, docs, thr


def set_knobs(monkeypatch, cache, per_edge_only):
    if per_edge_only:
        monkeypatch.setenv("FAC_NO_FAST", "1")
    if cache == "off":
        monkeypatch.setenv("FAC_NO_RC", "1")
    else:
        for k, v in (("FAC_RC_MIN", "1"), ("FAC_RC_K", "4"), ("FAC_RC_K2", "0")):
            monkeypatch.setenv(k, v)


SEEDS = [(0x1234_5678_9abc_def1, ASCII_VOCAB), (0xdead_beef_0bad_f00d, UNI_VOCAB), (0x0a57_2a1c_0de5_51de, ASTRAL_VOCAB)]
N_BATCHES = 100


@pytest.mark.parametrize("cache", ["off", "k4"])
@pytest.mark.parametrize("per_edge_only", [False, True])
@pytest.mark.parametrize("seed,vocab", SEEDS)
def test_differential(seed, vocab, per_edge_only, cache, monkeypatch):
    """7. Random mixed batches, every Order x Overlap, == the oracle on each document alone; with the
    prefix cache off and forced on (4-char keys), and with the goto-table expansion off."""
    set_knobs(monkeypatch, cache, per_edge_only)
    rng = Rng(seed)
    total = 0
    for _ in range(N_BATCHES):
        b, pats, docs, thr = random_batch(rng, vocab)
        eng, orc = b.build(pats), OracleEngine(b, pats)
        sb = check_batch(eng, orc, docs, thr)
        total += len(sb.search_records(O().threshold(thr))[0])
    assert total > 0


@pytest.mark.parametrize("budget,width", [(5, 4), (40, 8), (300, 3)])
def test_auto_beam_restarts_per_document(budget, width, monkeypatch):
    """7 (auto-beam). The running total of search.rs:1096-1103 restarts at every document: budgets
    crossed inside some documents of a batch."""
    set_knobs(monkeypatch, "k4", False)
    rng = Rng(0xab ^ budget)
    crossed = 0
    for _ in range(25):
        b, pats, docs, thr = random_batch(rng, ASCII_VOCAB + UNI_VOCAB, allow_beam=False)
        b = b.auto_beam(budget, width)
        eng, orc = b.build(pats), OracleEngine(b, pats)
        check_batch(eng, orc, docs, thr, combos=[(Order.Unsorted, Overlap.Keep), (Order.Default, Overlap.NonOverlapping)])
        plain = OracleEngine(b.auto_beam(2 ** 64 - 1, width), pats)
        crossed += sum(sorted(plain.raw_rows(d, thr)) != sorted(orc.raw_rows(d, thr)) for d in docs)
        b.auto_beam(budget, width)
    assert crossed > 0  # the beam did switch on inside some documents


def test_touching_spans_across_a_cut():
    """8. Spans that touch across a document boundary never interact, and the "pattern used once"
    set of NonOverlappingUnique is per document."""
    b = B()
    pats = ["ab", "b", "a"]
    eng, orc = b.build(pats), OracleEngine(b, pats)
    check_batch(eng, orc, ["xab", "abx"], 0.9)
    check_batch(eng, orc, ["ab", "ab", "", "b", "a"], 0.9)
    eng1, orc1 = b.build(["ab"]), OracleEngine(b, ["ab"])
    docs = ["ab ab", "ab", "ab"]
    check_batch(eng1, orc1, docs, 0.9)
    opts = O().threshold(0.9).sorted()
    opts.overlap_ = Overlap.NonOverlappingUnique
    res = eng1.search_batch(docs, opts)
    assert [[(m.start, m.end) for m in r] for r in res] == [[(0, 2)], [(0, 2)], [(0, 2)]]
    opts.overlap_ = Overlap.NonOverlapping
    assert [len(r) for r in eng1.search_batch(docs, opts)] == [2, 1, 1]


def test_errors(seg_engine, monkeypatch):
    """9. Bad offsets, the per-document grapheme limit, a device buffer one record short."""
    import torch
    lib = _native.lib
    data = b"abcdefgh"
    for off in ([0, 5, 3, 8], [1, 5, 8], [0, 9, 8]):
        arr = (ctypes.c_uint64 * len(off))(*off)
        h = ctypes.c_void_p()
        ed, eg = ctypes.c_uint64(7), ctypes.c_uint64(7)
        rc = lib.fac_batch_stage(seg_engine._h, data, arr, len(off) - 1, ctypes.byref(h), ctypes.byref(ed), ctypes.byref(eg))
        assert rc == _native.FAC_E_INVALID and not h.value, off
        with pytest.raises(DeviceError) as ei:
            StagedBatch(seg_engine, data, off)
        assert ei.value.code == _native.FAC_E_INVALID
    monkeypatch.setenv("FAC_GRAPHEME_LIMIT", "100")
    with pytest.raises(HaystackTooLarge) as ei:
        StagedBatch(seg_engine, *batch_offsets(["é".encode() * 50, b"a" * 101, "é".encode() * 150]))
    assert ei.value.doc == 1 and ei.value.graphemes == 101
    with pytest.raises(HaystackTooLarge) as ei:
        StagedBatch(seg_engine, *batch_offsets([b"a" * 100, "é".encode() * 150, b"a" * 101]))
    assert ei.value.doc == 1 and ei.value.graphemes == 150
    monkeypatch.delenv("FAC_GRAPHEME_LIMIT")
    b = B().fuzzy(L().edits(1))
    eng = b.build(["hello", "world"])
    docs = [b"hello world", b"", b"helo wrld hello", "wörld".encode()]
    sb = StagedBatch(eng, *batch_offsets(docs))
    opts = O().threshold(0.6).sorted()
    want, want_off = sb.search_records(opts)
    n = len(want)
    assert n > 2
    small = torch.empty((n - 1) * 32, dtype=torch.uint8, device="cuda")
    with pytest.raises(DeviceError) as ei:
        sb.search_records(opts, out=small)
    assert ei.value.code == _native.FAC_E_OUTPUT_CAPACITY and ei.value.needed == n
    exact = torch.empty(ei.value.needed * 32, dtype=torch.uint8, device="cuda")
    dev_off = torch.full((len(docs) + 1,), -1, dtype=torch.int64, device="cuda")
    got, got_off = sb.search_records(opts, out=exact, doc_offsets_out=dev_off)
    assert got.cpu().numpy().tobytes() == want.tobytes() and list(got_off) == list(want_off)
    assert dev_off.cpu().tolist() == [int(x) for x in want_off]


@pytest.mark.parametrize("seed,vocab", SEEDS)
def test_device_staging_equals_host_staging(seed, vocab):
    """10. The batches of test 7 staged from a torch byte tensor == staged from host bytes, also when
    one batch object is restaged in place over a second batch and back."""
    import torch
    rng = Rng(seed)
    cases = [random_batch(rng, vocab) for _ in range(N_BATCHES)]
    opts = lambda thr: O().threshold(thr).sorted().non_overlapping()  # noqa: E731

    def device_tensors(docs):
        data, off = batch_offsets([d.encode("utf-8") for d in docs])
        t = torch.from_numpy(np.frombuffer(data or b"\0", dtype=np.uint8).copy()).cuda()
        o = torch.from_numpy(np.asarray(off, dtype=np.uint64).view(np.int64).copy()).cuda()
        return data, off, t, o

    for (b, pats, docs, thr), (_, _, docs2, _) in zip(cases, cases[1:] + cases[:1]):
        eng = b.build(pats)
        want = [StagedBatch(eng, *batch_offsets([d.encode("utf-8") for d in dd])).search_records(opts(thr))
                for dd in (docs, docs2)]
        keep = []
        sb = None
        for which in (0, 1, 0):
            data, off, t, o = device_tensors((docs, docs2)[which])
            keep.append((t, o))
            sb = StagedBatch.from_device(eng, t.data_ptr(), o.data_ptr(), len(off) - 1, len(data), reuse=sb)
            recs, doc_off = sb.search_records(opts(thr))
            assert recs.tobytes() == want[which][0].tobytes() and list(doc_off) == list(want[which][1])
            for d in (0, len(off) - 2):
                raw = (docs, docs2)[which][d].encode("utf-8")
                assert sb.grapheme_starts(d) == host_starts(raw)
