"""Whole-token matches on the device (fac_batch_require_boundaries, boundary_kernels.hip): every batch
call of a flagged batch gives, per document, apply(order, overlap) of the document's raw records
with the rule of DESIGN.md 6a applied first. Every expected value is the CPU oracle's search_raw of
the document alone, filtered by the reference of the rule in test_boundaries_host.py (written from
`regex` properties; it never calls fac_boundary_*), then the oracle's apply and the host's replace /
segment_iter / strip_* / segment_text. Comparisons are bit-exact, similarity bits included."""
import struct

import numpy as np
import pytest

from fuzzy_aho_corasick import (Boundary, DeviceError, FuzzyAhoCorasickBuilder as B, FuzzyLimits as L, FuzzyMatch,
                                FuzzyMatches, Order, Overlap, Pattern, ReplacementTable, SearchOptions as O, StagedBatch,
                                Wrap, _native, batch_offsets)
from oracle_harness import OracleEngine
from test_boundaries_host import Rng, ref_classes, ref_ok

pytestmark = pytest.mark.gpu

SIDES = (Boundary.NONE, Boundary.START, Boundary.END, Boundary.WHOLE)
COMBOS = [(o, v) for o in Order for v in Overlap]
TWO = [(Order.Unsorted, Overlap.Keep), (Order.Default, Overlap.NonOverlapping)]


def options(thr, order=Order.Unsorted, overlap=Overlap.Keep):
    o = O().threshold(thr)
    o.order_, o.overlap_ = order, overlap
    return o


def segmented(opts):
    """query.rs:46-64: the options replace / segment_iter / strip_* / segment_text search with."""
    return options(opts.threshold_, Order.Default if opts.order_ == Order.Unsorted else opts.order_,
                   Overlap.NonOverlapping if opts.overlap_ == Overlap.Keep else opts.overlap_)


def sim_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def rows_of(recs):
    return [(int(r["start"]), int(r["end"]), int(r["pattern_index"]), sim_bits(float(r["similarity"])),
             int(r["insertions"]), int(r["deletions"]), int(r["substitutions"]), int(r["swaps"]), int(r["edits"]))
            for r in recs]


def canon(rows, order, overlap):
    """test_gpu_batch.py canon: after an overlap resolution equal starts have no order of their own
    (matches.rs:111, 148); Unsorted + Keep has none at all."""
    if overlap != Overlap.Keep:
        return sorted(rows, key=lambda r: (r[0],) + r[1:])
    return list(rows) if order != Order.Unsorted else sorted(rows)


class Ref:
    """The host composition: oracle search_raw of one document (computed once per document), the
    test's own predicate, the oracle's apply."""

    def __init__(self, builder, pats):
        self.orc = OracleEngine(builder, pats)
        self.raw = {}

    def raw_rows(self, doc, thr, prefilter=False):
        key = (doc, thr, prefilter)
        if key not in self.raw:
            self.raw[key] = self.orc.raw_rows(doc, thr, prefilter)
        return self.raw[key]

    def applied(self, doc, opts, sides, prefilter=False):
        """Full rows in apply's order. Unsorted with an overlap mode walks (start, end, pattern)
        order, as fac.h states for batches."""
        data = doc.encode("utf-8")
        rows = [r for r in self.raw_rows(doc, opts.threshold_, prefilter) if ref_ok(data, r[0], r[1], int(sides))]
        if opts.order_ == Order.Unsorted and opts.overlap_ != Overlap.Keep:
            rows = sorted(rows, key=lambda r: r[:3])
        return self.orc.apply_rows(rows, opts.order_, opts.overlap_)

    def rows(self, doc, opts, sides, prefilter=False):
        return [(r[0], r[1], r[2], sim_bits(r[3])) + tuple(r[4:]) for r in self.applied(doc, opts, sides, prefilter)]

    def matches(self, doc, opts, sides, prefilter=False):
        data = doc.encode("utf-8")
        inner = [FuzzyMatch(ins, dele, sub, swp, ed, p, self.orc.patterns_[p], s, e, sim, data[s:e].decode("utf-8"))
                 for (s, e, p, sim, ins, dele, sub, swp, ed) in self.applied(doc, opts, sides, prefilter)]
        starts = [m.start for m in inner]
        assert opts.overlap_ == Overlap.Keep or len(set(starts)) == len(starts), doc  # no tie to break
        return FuzzyMatches(doc, inner, data)


def staged(eng, docs, **kw):
    return StagedBatch(eng, *batch_offsets([d.encode("utf-8") for d in docs]), **kw)


def check_records(sb, ref, docs, thr, sides, combos, prefilter=False):
    for order, overlap in combos:
        opts = options(thr, order, overlap)
        recs, doc_off = sb.search_records(opts, prefilter=prefilter)
        assert len(doc_off) == len(docs) + 1 and doc_off[0] == 0 and int(doc_off[-1]) == len(recs)
        assert not recs["pad"].tobytes().strip(b"\0")
        for d, doc in enumerate(docs):
            got = rows_of(recs[int(doc_off[d]):int(doc_off[d + 1])])
            want = ref.rows(doc, opts, sides, prefilter)
            assert canon(got, order, overlap) == canon(want, order, overlap), (int(sides), order, overlap, d, doc)


# ---------------------------------------------------------------- 1. neighbour decode

LETTERS = ["x", "\u00e9", "\u0915", "\U0001d49c"]          # 1, 2, 3 and 4 bytes, alphanumeric
OTHERS = [" ", "\u00a7", "\u3001", "\U0001f600"]           # 1, 2, 3 and 4 bytes, not alphanumeric
NEIGHBOURS = [""] + LETTERS + OTHERS + ["\u0301", "\u093e", "_"]
ASCII_NEIGHBOURS = ["", "x", " ", "_", "7", "-"]
PAD = 256  # letter bytes before the first and after the last document, device staging only


def device_batch(eng, docs, pad=b"z", reuse=None, **kw):
    """The documents staged from device memory, with PAD bytes of a letter before the first document
    and after the last one. Returns (batch, the tensors to keep alive)."""
    import torch
    data, off = batch_offsets([d.encode("utf-8") for d in docs])
    fill = (pad * PAD)[-PAD:] if len(pad) == 1 else pad * (PAD // len(pad))
    t = torch.from_numpy(np.frombuffer(fill + data + fill, dtype=np.uint8).copy()).cuda()
    o = torch.from_numpy(np.asarray(off, dtype=np.uint64).view(np.int64).copy()).cuda()
    sb = StagedBatch.from_device(eng, t.data_ptr() + len(fill), o.data_ptr(), len(off) - 1, len(data), reuse=reuse, **kw)
    return sb, (t, o)


def interleaved(cases, seps):
    """case, sep, case, ..., sep, case: the byte before a case's start and the byte after its end belong
    to a letter of the neighbouring document (for the batch's first and last document, which are
    cases too, to a letter of device_batch's padding). Every fifth case has an empty document before it."""
    docs = []
    for k, c in enumerate(cases):
        if k:
            docs.append(seps[k % len(seps)])
        if k % 5 == 0:
            docs.append("")
        docs.append(c)
    return docs[1:]  # (without the empty document before the first case)


@pytest.fixture(scope="module")
def ab():
    b = B().case_insensitive(True)
    return b.build(["ab"]), Ref(b, ["ab"])


@pytest.mark.parametrize("mixed", [False, True])
def test_neighbour_decode(ab, mixed):
    """L + "ab" + R for every L and R of the list (an all-ASCII batch and a mixed one), all four
    masks, Unsorted + Keep and Default + NonOverlapping. The batch is staged from device memory that
    holds letters right before its first byte and right after its last."""
    eng, ref = ab
    nb = NEIGHBOURS if mixed else ASCII_NEIGHBOURS
    cases = [l + "ab" + r for l in nb for r in nb] + ["", "AB", "abab", "ab ab", "ab_ab", "ab"]
    docs = interleaved(cases, ["z", "\u00e9"] if mixed else ["z", "Q"])
    assert all(d.isascii() for d in docs) != mixed
    sb, keep = device_batch(eng, docs, pad="\u00e9".encode("utf-8") if mixed else b"z")
    dropped = set()
    for sides in SIDES:
        sb.require_boundaries(sides)
        check_records(sb, ref, docs, 0.9, sides, TWO)
        raw = sum(len(ref.rows(doc, options(0.9), Boundary.NONE)) for doc in docs)
        dropped.add((int(sides), raw - sum(len(ref.rows(doc, options(0.9), sides)) for doc in docs) > 0))
    assert dropped == {(0, False), (1, True), (2, True), (3, True)}
    del keep


# ---------------------------------------------------------------- 2. every code point on the device

def sampled_code_points():
    """Every code point of the BMP, and beyond it both edges and one interior member of every run of
    equal class."""
    cls = ref_classes()
    cps = [c for c in range(0x10000) if not 0xD800 <= c <= 0xDFFF]
    a = 0x10000
    while a < 0x110000:
        b = a
        while b + 1 < 0x110000 and cls[b + 1] == cls[a]:
            b += 1
        cps += sorted({a, (a + b) // 2, b})
        a = b + 1
    return cps


def test_every_code_point_on_the_device(ab):
    """Three documents per code point c: "x" + c + "ab", " " + c + "ab" and "ab" + c, searched with
    START and with END. Coverage: every code point of the BMP, plus both edges and one interior member
    of every run of equal class beyond it (all 1.1 M code points would take the test past a few
    seconds, most of it building three million Python strings). Expected: the same batch's
    unflagged Unsorted + Keep records, filtered by the test's reference."""
    eng, _ = ab
    cps = sampled_code_points()
    assert len(cps) > 63488 and 0x10FFFF in cps and 0x1D49C in cps
    enc = []
    for c in cps:
        u = chr(c).encode("utf-8")
        enc += [b"x" + u + b"ab", b" " + u + b"ab", b"ab" + u]
    data, off = batch_offsets(enc)
    sb = StagedBatch(eng, data, off)
    opts = options(0.9)
    recs, doc_off = sb.search_records(opts)
    assert len(recs) > 2 * len(cps)
    doc_of = np.repeat(np.arange(len(enc)), np.diff(doc_off.astype(np.int64)))
    base = [r.tobytes() for r in recs]
    spans = [(int(d), int(s), int(e)) for d, s, e in zip(doc_of, recs["start"], recs["end"])]
    for sides in (Boundary.START, Boundary.END):
        want, want_off = [], [0] * (len(enc) + 1)
        for rec, (d, s, e) in zip(base, spans):
            if ref_ok(enc[d], s, e, int(sides)):
                want.append((d, rec))
                want_off[d + 1] += 1
        got, got_off = sb.require_boundaries(sides).search_records(opts)
        assert list(got_off) == list(np.cumsum(want_off)), int(sides)
        got_doc = np.repeat(np.arange(len(enc)), np.diff(got_off.astype(np.int64)))
        assert sorted(zip(got_doc.tolist(), (r.tobytes() for r in got))) == sorted(want), int(sides)
        assert 0 < len(want) < len(base)


# ---------------------------------------------------------------- 3. the filter runs before the overlap walk

def test_filter_before_overlap_closed_form():
    """"bc d" beats "d" in the unflagged overlap walk and is itself inside a word: a filter after the
    apply would return nothing, the filter before it returns "d"."""
    b = B()
    pats = ["bc d", "d"]
    eng, ref = b.build(pats), Ref(b, pats)
    opts = options(0.9, Order.Default, Overlap.NonOverlapping)
    assert [r[:3] for r in ref.rows("abc d", opts, Boundary.NONE)] == [(1, 5, 0)]
    assert [r[:3] for r in ref.rows("abc d", opts, Boundary.WHOLE)] == [(4, 5, 1)]
    sb = staged(eng, ["abc d"], boundaries=Boundary.WHOLE)
    recs, doc_off = sb.search_records(opts)
    assert rows_of(recs) == ref.rows("abc d", opts, Boundary.WHOLE) and list(doc_off) == [0, 1]
    assert [r[:3] for r in rows_of(recs)] == [(4, 5, 1)]
    recs, _ = sb.require_boundaries(Boundary.NONE).search_records(opts)
    assert [r[:3] for r in rows_of(recs)] == [(1, 5, 0)]


WORDS = ["art", "party", "cart", "art-house", "caf\u00e9", "cafe\u0301bar", "\u00b2art", "art_", "\u0915\u093eart",
         "start", "Art", "9art", "art\ufe0f", "\U0001d49cart", "bar", "barn", "crowbar", "bart", "the", "a", "cafe"]
SEPS = [" ", " ", ", ", "", "_", ". "]


def word_docs(rng, n, ascii_only=False):
    words = [w for w in WORDS if w.isascii()] if ascii_only else WORDS
    return ["".join(words[rng.next() % len(words)] + SEPS[rng.next() % len(SEPS)] for _ in range(1 + rng.next() % 7))
            for _ in range(n)]


def test_filter_before_overlap_fuzzy():
    """A fuzzy engine over seeded documents of words, every order x overlap, NonOverlappingUnique
    with custom unique ids included."""
    b = B().fuzzy(L().edits(1)).case_insensitive(True)
    pats = [Pattern("art").custom_unique_id(1), Pattern("bar").custom_unique_id(1), Pattern("caf\u00e9"),
            Pattern("art house"), Pattern("cart")]
    eng, ref = b.build(pats), Ref(b, pats)
    docs = word_docs(Rng(0xF11735), 36) + [""]
    sb = staged(eng, docs)
    differs = 0
    for sides in (Boundary.WHOLE, Boundary.START):
        sb.require_boundaries(sides)
        check_records(sb, ref, docs, 0.6, sides, COMBOS)
        opts = options(0.6, Order.Default, Overlap.NonOverlapping)
        for doc in docs:  # documents where filtering the unflagged result afterwards is another answer
            data = doc.encode("utf-8")
            after = [r for r in ref.rows(doc, opts, Boundary.NONE) if ref_ok(data, r[0], r[1], int(sides))]
            differs += after != ref.rows(doc, opts, sides)
    assert differs > 0


# ---------------------------------------------------------------- 4. compaction and regrow

def periodic(n):
    """n words, word i is "xab" (in-word) when i % 3 == 0, else "ab"."""
    return ["xab" if i % 3 == 0 else "ab" for i in range(n)]


def ab_row(start):
    return (start, start + 2, 0, sim_bits(1.0), 0, 0, 0, 0, 0)


@pytest.mark.parametrize("n", [63, 64, 65, 257, 70001])
def test_compaction_one_record_per_document(ab, n):
    """n raw records, one per document, a keep / drop pattern of period 3; 70 001 is more than one
    launch's first capacity (the search runs again) and more than one workgroup."""
    eng, _ = ab
    docs = periodic(n)
    sb = staged(eng, docs)
    recs, doc_off = sb.search_records(options(0.9))
    assert len(recs) == n
    sb.require_boundaries(Boundary.WHOLE)
    for order, overlap in TWO:
        recs, doc_off = sb.search_records(options(0.9, order, overlap))
        keep = [i % 3 != 0 for i in range(n)]
        assert list(doc_off) == [0] + list(np.cumsum(keep))
        assert rows_of(recs[:300]) == [ab_row(0)] * min(300, sum(keep)) and len(recs) == sum(keep)
        assert len(set(r.tobytes() for r in recs)) == 1
    recs, doc_off = sb.require_boundaries(Boundary.END).search_records(options(0.9))
    assert len(recs) == n  # "xab" ends at its document's end


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_compaction_one_document(ab, n):
    """The same n records inside one document (every record carries the same tag)."""
    eng, _ = ab
    words = periodic(n)
    doc = " ".join(words)
    starts, pos = [], 0
    for w in words:
        starts.append(pos + len(w) - 2)
        pos += len(w) + 1
    sb = staged(eng, ["", doc, ""])
    recs, _ = sb.search_records(options(0.9))
    assert sorted(rows_of(recs)) == [ab_row(s) for s in starts]
    sb.require_boundaries(Boundary.WHOLE)
    for order, overlap in TWO:
        recs, doc_off = sb.search_records(options(0.9, order, overlap))
        want = [ab_row(s) for i, s in enumerate(starts) if i % 3 != 0]
        assert canon(rows_of(recs), order, overlap) == want and list(doc_off) == [0, 0, len(want), len(want)]


def test_everything_dropped_and_nothing_found(ab):
    eng, _ = ab
    for docs in (["xab", "abx", "", "xabx"] * 40, ["zzz", "", "a b"] * 40):
        sb = staged(eng, docs, boundaries=Boundary.WHOLE)
        for order, overlap in TWO:
            recs, doc_off = sb.search_records(options(0.9, order, overlap))
            assert len(recs) == 0 and list(doc_off) == [0] * (len(docs) + 1)
        out, off = sb.replace_bytes(ReplacementTable(eng, ["#"]), options(0.9))
        assert out == "".join(docs).encode() and sb.replaced == 0
        assert list(off) == batch_offsets([d.encode() for d in docs])[1]


# ---------------------------------------------------------------- 5. every call takes the flag

CALL_PATS = ["hello", "world", "cell", "art house", "caf\u00e9"]
PLAIN = ["HELLO", None, "", "<ah>", "coffee"]
WRAPS = [Wrap("<b>", "</b>"), None, Wrap("", "#"), "AH", Wrap("\u00ab", "\u00bb")]
ASCII_DOCS = ["hello world", "Othello, hello! helloworld", "xcell cells cell", "  art house, cart houses  ", "",
              "hello_world hello-world", "world", "a hallo wrld", "cell2 2cell cell", "the art-house smart house art house"]
MIXED_DOCS = ASCII_DOCS[:6] + ["caf\u00e9 caf\u00e9s \u00e9caf\u00e9", "hello\u0301 e\u0301hello \u0301hello", "\u0915\u093ecell cell\u3001cell",
                               "\U0001d49chello \U0001f600hello\U0001f600", "caf\u00e9_ \u00b2caf\u00e9 (caf\u00e9)"]


def callback(reps):
    def cb(m):
        r = reps[m.pattern_index]
        return r.render(m.text) if isinstance(r, Wrap) else r
    return cb


def item_of(doc: bytes, row, reps):
    r = None if reps is None else reps[row[2]]
    text = doc[row[0]:row[1]].decode("utf-8")
    return (r.render(text) if isinstance(r, Wrap) else text if r is None else r).encode("utf-8")


def check_every_call(eng, ref, sb, docs, thr, sides, prefilter=False, combos=TWO):
    import torch
    enc = [d.encode("utf-8") for d in docs]
    for order, overlap in combos:
        opts = options(thr, order, overlap)
        seg = segmented(opts)
        ms = [ref.matches(doc, seg, sides, prefilter) for doc in docs]
        # replace, a plain table and a template table
        for reps in (PLAIN, WRAPS):
            out, off = sb.replace_bytes(ReplacementTable(eng, reps), opts, prefilter=prefilter)
            got = [out[int(off[d]):int(off[d + 1])] for d in range(len(docs))]
            assert got == [m.replace(callback(reps)).encode("utf-8") for m in ms], (int(sides), order, overlap, reps)
            assert sb.replaced == sum(len(m) for m in ms)
        # extract, without and with a table
        for reps in (None, WRAPS):
            table = None if reps is None else ReplacementTable(eng, reps)
            recs, doc_off, text, item_off = sb.extract(table, opts, prefilter=prefilter)
            rows = rows_of(recs)
            for d, doc in enumerate(docs):
                lo, hi = int(doc_off[d]), int(doc_off[d + 1])
                pairs = [(rows[i], text[int(item_off[i]):int(item_off[i + 1])]) for i in range(lo, hi)]
                want = [(r, item_of(enc[d], r, reps)) for r in ref.rows(doc, opts, sides, prefilter)]
                assert canon(pairs, order, overlap) == canon(want, order, overlap), (int(sides), order, overlap, d, doc)
        # segment_iter
        recs, doc_off = sb.segment_records(opts, prefilter=prefilter)
        for d, doc in enumerate(docs):
            got = [(int(r["start"]), int(r["end"]), int(r["pattern_index"]), sim_bits(float(r["similarity"])))
                   for r in recs[int(doc_off[d]):int(doc_off[d + 1])]]
            want = [(s.matched().start, s.matched().end, s.matched().pattern_index, s.matched().sim_bits())
                    if s.matched() is not None else
                    (s.unmatched().start, s.unmatched().end, _native.FAC_UNMATCHED, 0) for s in ms[d].segment_iter()]
            got = [g if g[2] != _native.FAC_UNMATCHED else g[:3] + (0,) for g in got]
            assert got == want, (int(sides), order, overlap, d, doc)
        # strip_prefix, strip_suffix, segment_text
        for mode, host in ((_native.FAC_RENDER_STRIP_PREFIX, FuzzyMatches.strip_prefix),
                           (_native.FAC_RENDER_STRIP_SUFFIX, FuzzyMatches.strip_suffix),
                           (_native.FAC_RENDER_SEGMENT_TEXT, FuzzyMatches.segment_text)):
            out, off = sb.render_bytes(mode, opts, prefilter=prefilter)
            got = [out[int(off[d]):int(off[d + 1])].decode("utf-8") for d in range(len(docs))]
            assert got == [host(m) for m in ms], (int(sides), order, overlap, mode)
        # search_records, records left in HBM
        host_recs, host_off = sb.search_records(opts, prefilter=prefilter)
        buf = torch.zeros(max(1, len(host_recs)) * _native.REC_BYTES, dtype=torch.uint8, device="cuda")
        idx = torch.zeros(len(docs) + 1, dtype=torch.int64, device="cuda")
        dev, dev_off = sb.search_records(opts, out=buf, doc_offsets_out=idx, prefilter=prefilter)
        assert list(dev_off) == list(host_off) == idx.cpu().tolist()
        dev_recs = np.frombuffer(dev.cpu().numpy().tobytes(), dtype=_native.MATCH_DTYPE)
        for d, doc in enumerate(docs):
            lo, hi = int(host_off[d]), int(host_off[d + 1])
            assert canon(rows_of(dev_recs[lo:hi]), order, overlap) == canon(ref.rows(doc, opts, sides, prefilter), order,
                                                                           overlap), (int(sides), order, overlap, d, doc)


@pytest.fixture(scope="module")
def callers():
    b = B().fuzzy(L().edits(1)).case_insensitive(True)
    return b.build(CALL_PATS), Ref(b, CALL_PATS)


@pytest.mark.parametrize("mixed", [False, True])
def test_every_call_takes_the_flag(callers, mixed):
    eng, ref = callers
    docs = MIXED_DOCS if mixed else ASCII_DOCS
    assert all(d.isascii() for d in docs) != mixed
    sb = staged(eng, docs)
    changed = False
    for sides in (Boundary.WHOLE, Boundary.END):
        sb.require_boundaries(sides)
        check_every_call(eng, ref, sb, docs, 0.7, sides)
        seg = segmented(options(0.7))
        changed |= any(ref.rows(d, seg, sides) != ref.rows(d, seg, Boundary.NONE) for d in docs)
    assert changed


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("thr", [0.7, 1.0])
def test_prefiltered_calls_take_the_flag(callers, mixed, thr):
    """The pre-filtered forms, on an all-ASCII batch and on a batch opted in with unicode_prefilter.
    At threshold 1.0 the edit budget is 0 and a merged window is exactly a match: document 0 has a
    match at the first byte of a merged window with a letter just before it in the document, so the
    neighbour must come from the document and not from the window."""
    eng, ref = callers
    assert eng.with_prefilter().is_active()
    first = ("\u00e9" if mixed else "x") + "hello hello"
    docs = [first] + (MIXED_DOCS if mixed else ASCII_DOCS)
    sb = staged(eng, docs, unicode_prefilter=mixed)
    wins = sb.prefilter_windows(thr)
    assert wins is not None
    if thr == 1.0:
        assert (0, 1, 6) in wins and (0, 7, 12) in wins  # bytes or graphemes: one symbol before "hello"
        whole = ref.rows(first, options(thr), Boundary.WHOLE, True)
        assert len(whole) == 1 and len(ref.rows(first, options(thr), Boundary.NONE, True)) == 2
    sb.require_boundaries(Boundary.WHOLE)
    check_every_call(eng, ref, sb, docs, thr, Boundary.WHOLE, prefilter=True)
    check_records(sb.require_boundaries(Boundary.START), ref, docs, thr, Boundary.START, COMBOS, prefilter=True)


def test_mapping_engine_takes_the_flag():
    b = B().fuzzy(L().edits(1)).case_insensitive(True).mapping("\u00df", "ss")
    pats = ["stra\u00dfe", "gro\u00df"]
    eng, ref = b.build(pats), Ref(b, pats)
    docs = ["Stra\u00dfe", "xstra\u00dfe stra\u00dfe", "strasse! Hauptstrasse", "gro\u00df gro\u00dfe, Gross", "", "die Stra\u00dfen stra\u00dfe_"]
    sb = staged(eng, docs, unicode_mappings=True)
    for sides in SIDES:
        check_records(sb.require_boundaries(sides), ref, docs, 0.8, sides, COMBOS)
    assert any(ref.rows(d, options(0.8), Boundary.WHOLE) != ref.rows(d, options(0.8), Boundary.NONE) for d in docs)


# ---------------------------------------------------------------- 6. flag lifetime

def test_flag_lifetime(callers):
    eng, ref = callers
    a, b2 = MIXED_DOCS, ["helloworld hello", "", "xcell cell caf\u00e9s"]
    opts = options(0.7, Order.Default, Overlap.NonOverlapping)
    sb, keep = device_batch(eng, a, boundaries=Boundary.WHOLE)
    check_records(sb, ref, a, 0.7, Boundary.WHOLE, TWO)
    sb2, keep2 = device_batch(eng, b2, reuse=sb)  # restaged in place with other documents
    assert sb2 is sb
    check_records(sb, ref, b2, 0.7, Boundary.WHOLE, TWO)
    assert any(ref.rows(d, opts, Boundary.WHOLE) != ref.rows(d, opts, Boundary.NONE) for d in b2)
    assert sb.require_boundaries(0) is sb
    check_records(sb, ref, b2, 0.7, Boundary.NONE, TWO)
    for bad in (4, -1):
        with pytest.raises(DeviceError) as ei:
            sb.require_boundaries(bad)
        assert ei.value.code == _native.FAC_E_INVALID
    check_records(sb, ref, b2, 0.7, Boundary.NONE, TWO)  # a refused mask leaves the old one
    del keep, keep2


def test_engine_search_and_conveniences(callers):
    eng, ref = callers
    for doc in MIXED_DOCS:
        for order, overlap in TWO:
            opts = options(0.7, order, overlap)
            got = eng.search(doc, opts, boundaries=Boundary.WHOLE)
            rows = [(m.start, m.end, m.pattern_index, m.sim_bits(), m.insertions, m.deletions, m.substitutions, m.swaps,
                     m.edits) for m in got]
            assert canon(rows, order, overlap) == canon(ref.rows(doc, opts, Boundary.WHOLE), order, overlap), doc
            assert [m.text for m in got] == [doc.encode("utf-8")[m.start:m.end].decode("utf-8") for m in got]
    opts = options(0.7, Order.Default, Overlap.NonOverlapping)
    ms = [ref.matches(d, opts, Boundary.WHOLE) for d in MIXED_DOCS]
    assert eng.replace_batch(MIXED_DOCS, opts, PLAIN, boundaries=Boundary.WHOLE) == [m.replace(callback(PLAIN)) for m in ms]
    assert eng.matched_strings_batch(MIXED_DOCS, opts, boundaries=Boundary.WHOLE) == [m.matched_strings() for m in ms]
    assert eng.strip_prefix_batch(MIXED_DOCS, opts, boundaries=Boundary.WHOLE) == [m.strip_prefix() for m in ms]
    assert eng.split_batch(MIXED_DOCS, opts, boundaries=Boundary.WHOLE) == [list(m.split()) for m in ms]
    pre = eng.with_prefilter()
    pms = [ref.matches(d, opts, Boundary.WHOLE, True) for d in MIXED_DOCS]
    assert pre.replace_batch(MIXED_DOCS, opts, PLAIN, boundaries=Boundary.WHOLE) == [m.replace(callback(PLAIN)) for m in pms]
    assert pre.segment_text_batch(MIXED_DOCS, opts, boundaries=Boundary.WHOLE) == [m.segment_text() for m in pms]
    got = pre.search_batch(MIXED_DOCS, opts, boundaries=Boundary.WHOLE)
    assert [[m.key() for m in g] for g in got] == [[m.key() for m in p] for p in pms]
