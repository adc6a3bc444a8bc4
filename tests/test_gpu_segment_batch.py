"""fac_segment_batch / fac_render_batch: segment_iter, split, strip_prefix, strip_suffix and
segment_text of a whole batch on the device, per document == the crate's call on that document
alone (query.rs:98-170, matches.rs:218-594).

Two expected values, as in test_gpu_replace_batch:
  E1  the loops of matches.rs:218-594 in plain Python (below) over the records
      StagedBatch.search_records returns for the same batch and the normalised options (those
      records are pinned to the oracle by test_gpu_batch). Whitespace is the explicit list of the 25
      White_Space code points, never str.strip. Defined for every document, compared byte for byte,
      always.
  E2  OracleEngine.strip_prefix / strip_suffix / split / segment_text on each document alone (one
      oracle search per document, the four host walks on it). Compared where the oracle's kept
      records have pairwise distinct starts (the others are the reference's unspecified tie,
      matches.rs:111) and the document holds none of U+001C-U+001F (the host class trims those with
      str.strip, the crate does not). The random test asserts that at most 5 % are excluded.
"""
import numpy as np
import pytest

from fuzzy_aho_corasick import (DeviceError, FuzzyAhoCorasickBuilder as B, FuzzyLimits as L, Order, Overlap, Pattern,
                                SearchOptions as O, StagedBatch, UnsupportedConfiguration, _native, batch_offsets)
from oracle_harness import OracleEngine
from test_gpu_batch import ASCII_VOCAB, ASTRAL_VOCAB, SEEDS, UNI_VOCAB, Rng, random_batch, set_knobs  # noqa: F401

pytestmark = pytest.mark.gpu

TILE = _native.SEGMENT_TILE
UNMATCHED = _native.FAC_UNMATCHED
PREFIX, SUFFIX, TEXT = (_native.FAC_RENDER_STRIP_PREFIX, _native.FAC_RENDER_STRIP_SUFFIX,
                        _native.FAC_RENDER_SEGMENT_TEXT)
MODES = (PREFIX, SUFFIX, TEXT)

# Rust's char::is_whitespace: the Unicode White_Space property
WHITE_SPACE = frozenset(chr(c) for c in [0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680] +
                        list(range(0x2000, 0x200B)) + [0x2028, 0x2029, 0x202F, 0x205F, 0x3000])
assert len(WHITE_SPACE) == 25
NO_LEADING_SPACE = (",", ".", "?", "!", ";", ":", "—", "-", "…")  # matches.rs:560-564
HOST_ONLY_SPACE = ("\x1c", "\x1d", "\x1e", "\x1f")  # str.strip trims them, char::is_whitespace does not


def normalised(opts):
    """query.rs:46-64"""
    n = O().threshold(opts.threshold_)
    n.order_ = Order.Default if opts.order_ == Order.Unsorted else opts.order_
    n.overlap_ = Overlap.NonOverlapping if opts.overlap_ == Overlap.Keep else opts.overlap_
    return n


def options(thr, order=Order.Default, overlap=Overlap.NonOverlapping):
    o = O().threshold(thr)
    o.order_, o.overlap_ = order, overlap
    return o


# ---------------------------------------------------------------- E1

def trim_start(s: str) -> str:
    i = 0
    while i < len(s) and s[i] in WHITE_SPACE:
        i += 1
    return s[i:]


def trim_end(s: str) -> str:
    i = len(s)
    while i > 0 and s[i - 1] in WHITE_SPACE:
        i -= 1
    return s[:i]


def e1_segments(doc: bytes, spans):
    """matches.rs:526-553 over (start, end) spans: [(record index or None, start, end)]"""
    segs, last = [], 0
    for i, (s, e) in enumerate(spans):
        if s >= last:
            if s > last:
                segs.append((None, last, s))
            segs.append((i, s, e))
            last = e
    if last < len(doc):
        segs.append((None, last, len(doc)))
    return segs


def e1_strip_prefix(doc: bytes, segs) -> str:
    """matches.rs:218-245"""
    out, skipping = [], True
    for i, s, e in segs:
        text = doc[s:e].decode("utf-8")
        if i is not None:
            if not skipping:
                out.append(text)
        elif skipping:
            if trim_start(text) == "":
                continue
            skipping = False
            out.append(trim_start(text))
        else:
            out.append(text)
    return "".join(out)


def e1_strip_suffix(doc: bytes, segs) -> str:
    """matches.rs:276-307"""
    keep = 0
    for k, (i, s, e) in enumerate(segs):
        if i is None and trim_end(doc[s:e].decode("utf-8")) != "":
            keep = k + 1
    out = []
    for k, (i, s, e) in enumerate(segs[:keep]):
        text = doc[s:e].decode("utf-8")
        out.append(trim_end(text) if k + 1 == keep else text)
    return "".join(out)


def e1_split(doc: bytes, segs):
    """matches.rs:344-354"""
    return [doc[s:e].decode("utf-8") for i, s, e in segs if i is None]


def e1_pieces(doc: bytes, segs):
    """matches.rs:566-594: (space before, start, end) per segment"""
    out, prev_matched, pieces = "", False, []
    for i, s, e in segs:
        text = doc[s:e].decode("utf-8")
        if i is not None:
            space = prev_matched or (out != "" and not out.endswith((" ", "\t")))
            prev_matched = True
        else:
            space = prev_matched and not text.startswith(NO_LEADING_SPACE)
            prev_matched = False
        out += (" " if space else "") + text
        pieces.append((space, s, e))
    return pieces, out


def e1_segment_text(doc: bytes, segs) -> str:
    return e1_pieces(doc, segs)[1]


E1 = {PREFIX: e1_strip_prefix, SUFFIX: e1_strip_suffix, TEXT: e1_segment_text}


def unmatched_record(s, e):
    r = np.zeros(1, dtype=_native.MATCH_DTYPE)
    r["start"], r["end"], r["pattern_index"] = s, e, UNMATCHED
    return r.tobytes()


def encode(docs):
    return [d.encode("utf-8") if isinstance(d, str) else d for d in docs]


def check(eng, docs, opts, orc=None, sb=None, prefilter=False):
    """Every mode and segment_records of the batch == E1 for every document, == E2 (with `orc`) where
    allowed. Returns ({mode: per-document bytes, "segments": per-document records, "split": ...},
    documents compared with E2, documents excluded)."""
    enc = encode(docs)
    if sb is None:
        sb = StagedBatch(eng, *batch_offsets(enc))
    recs, doc_off = sb.search_records(normalised(opts), prefilter=prefilter)
    rows = [recs[int(doc_off[d]):int(doc_off[d + 1])] for d in range(len(enc))]
    segs = [e1_segments(doc, [(int(r["start"]), int(r["end"])) for r in rows[d]]) for d, doc in enumerate(enc)]
    got = {}
    for mode in MODES:
        out, off = sb.render_bytes(mode, opts, prefilter=prefilter)
        assert isinstance(out, bytes) and len(off) == len(enc) + 1 and off[0] == 0 and int(off[-1]) == len(out)
        got[mode] = [out[int(off[d]):int(off[d + 1])] for d in range(len(enc))]
        for d, doc in enumerate(enc):
            assert got[mode][d] == E1[mode](doc, segs[d]).encode("utf-8"), (mode, d, doc, segs[d])
    srecs, soff = sb.segment_records(opts, prefilter=prefilter)
    assert len(soff) == len(enc) + 1 and soff[0] == 0 and int(soff[-1]) == len(srecs)
    got["segments"], got["split"] = [], []
    for d, doc in enumerate(enc):
        mine = srecs[int(soff[d]):int(soff[d + 1])]
        got["segments"].append(mine)
        assert len(mine) == len(segs[d]), (d, doc, segs[d])
        at = 0
        for seg, (i, s, e) in zip(mine, segs[d]):
            assert int(seg["start"]) == at == s and int(seg["end"]) == e  # the segments tile the document
            at = e
            if i is None:
                assert e > s and int(seg["pattern_index"]) == UNMATCHED and seg.tobytes() == unmatched_record(s, e)
            else:
                assert seg.tobytes() == rows[d][i].tobytes()  # field for field, similarity bits included
        assert at == len(doc)
        got["split"].append([doc[int(r["start"]):int(r["end"])].decode("utf-8") for r in mine
                             if int(r["pattern_index"]) == UNMATCHED])
        assert got["split"][d] == e1_split(doc, segs[d])
    compared = excluded = 0
    if orc is not None:
        for d, doc in enumerate(docs):
            ms = orc._segmented(doc, opts)  # what OracleEngine.strip_prefix / ... / segment_text search
            starts = [m.start for m in ms]
            if len(set(starts)) != len(starts) or any(c in doc for c in HOST_ONLY_SPACE):
                excluded += 1
                continue
            assert got[PREFIX][d] == ms.strip_prefix().encode("utf-8"), (d, doc)
            assert got[SUFFIX][d] == ms.strip_suffix().encode("utf-8"), (d, doc)
            assert got[TEXT][d] == ms.segment_text().encode("utf-8"), (d, doc)
            assert got["split"][d] == list(ms.split()), (d, doc)
            compared += 1
    return got, compared, excluded


def texts(got, mode):
    return [g.decode("utf-8") for g in got[mode]]


# ---------------------------------------------------------------- 1. the crate's own cases

def test_crate_cases_in_one_batch():
    # tests.rs:356-373
    b = B().fuzzy(L().edits(3))
    pats = ["saddam", "hussein"]
    eng, orc = b.build(pats), OracleEngine(b, pats)
    docs = ["sadamhusein", "sadamhuseinaltikriti", "", "zzzz"]
    got, compared, _ = check(eng, docs, O().threshold(0.8), orc)
    assert texts(got, TEXT) == ["sadam husein", "sadam husein altikriti", "", "zzzz"] and compared == 4
    assert eng.segment_text_batch(docs, O().threshold(0.8)) == texts(got, TEXT)
    # tests.rs:375-391
    b = B().fuzzy(L().edits(1))
    pats = ["input", "more"]
    eng, orc = b.build(pats), OracleEngine(b, pats)
    got, _, _ = check(eng, ["someinptandm0re", ""], O().threshold(0.75), orc)
    assert texts(got, TEXT) == ["some inpt and m0re", ""]
    # tests.rs:393-407
    b = B().fuzzy(L().edits(3))
    pats = ["SHANE", "DOMINIC", "CRAWFORD"]
    eng, orc = b.build(pats), OracleEngine(b, pats)
    got, _, _ = check(eng, ["SHANEDOM INICCRAWFORD", "nothing"], O().threshold(0.8), orc)
    assert texts(got, TEXT) == ["SHANE DOM INIC CRAWFORD", "nothing"]
    # tests.rs:409-423
    b = B().case_insensitive(True)
    pats = ["HASAN", "JAMAL", "HUSSEIN", "ZEINIYE"]
    eng, orc = b.build(pats), OracleEngine(b, pats)
    got, _, _ = check(eng, ["ZEINIYEHussEINHASaNJAMAL"], O().threshold(0.8), orc)
    assert texts(got, TEXT) == ["ZEINIYE HussEIN HASaN JAMAL"]
    # tests.rs:425-434
    b = B()
    pats = ["saddam", "hussein"]
    eng, orc = b.build(pats), OracleEngine(b, pats)
    got, _, _ = check(eng, ["sadam husein"], O().threshold(0.8), orc)
    assert texts(got, TEXT) == ["sadam husein"]
    # tests.rs:98-118, query.rs:113
    b = B().case_insensitive(True)
    eng, orc = b.build(["юрий"]), OracleEngine(b, ["юрий"])
    got, _, _ = check(eng, ["ЮРИЙГАГАРИН", "", "ГАГАРИН"], O().threshold(0.9), orc)
    assert texts(got, TEXT) == ["ЮРИЙ ГАГАРИН", "", "ГАГАРИН"]
    # builder.rs:12-21
    b = B().case_insensitive(True)
    eng, orc = b.build(["hello", "world"]), OracleEngine(b, ["hello", "world"])
    got, _, _ = check(eng, ["justheLLowOrLd!"], O().threshold(1.0), orc)
    assert texts(got, TEXT) == ["just heLLo wOrLd!"]


def test_crate_strip_and_split_cases_in_one_batch():
    # tests.rs:539-576
    b = B().fuzzy(L().edits(1)).case_insensitive(True)
    pats = ["LOREM", "IPSUM"]
    eng, orc = b.build(pats), OracleEngine(b, pats)
    opts = O().threshold(0.8)
    docs = ["LrEM ISuM Lorm ZZZ", "ZZZ LrEM ISuM Lorm", "ZZZLrEMISuMAAA", "", "no match"]
    got, compared, _ = check(eng, docs, opts, orc)
    assert compared == len(docs)
    assert texts(got, PREFIX)[0] == "ZZZ" and texts(got, SUFFIX)[1] == "ZZZ" and got["split"][2] == ["ZZZ", "AAA"]
    assert texts(got, PREFIX)[3:] == ["", "no match"] and texts(got, SUFFIX)[3:] == ["", "no match"]
    assert got["split"][3:] == [[], ["no match"]]
    assert eng.strip_prefix_batch(docs, opts)[0] == "ZZZ" and eng.strip_suffix_batch(docs, opts)[1] == "ZZZ"
    assert eng.split_batch(docs, opts)[2] == ["ZZZ", "AAA"]
    # query.rs:112-165
    pats = ["FOO", "BAR"]
    eng, orc = b.build(pats), OracleEngine(b, pats)
    got, _, _ = check(eng, ["xxFo0yyBAARzz", ""], opts, orc)
    assert got["split"] == [["xx", "yy", "zz"], []]


# ---------------------------------------------------------------- 2. edges of the walk

def test_segment_edges():
    b = B().fuzzy(L().edits(1)).case_insensitive(True)
    pats = ["hello", "wörld", "ab"]
    eng, orc = b.build(pats), OracleEngine(b, pats)
    docs = ["",                       # an empty document
            "zzzz qqqq",              # no match
            "hello zz",               # a match at byte 0
            "zz hello",               # a match ending at the document's end
            "helloab",                # two touching matches
            "abhelloab",
            "zz wörld zz wôrld",      # multi-byte text
            "ab",                     # the whole document one match
            "é"]
    opts = O().threshold(0.75)
    got, compared, excluded = check(eng, docs, opts, orc)
    assert compared == len(docs) and excluded == 0
    assert len(got["segments"][0]) == 0 and len(got["segments"][7]) == 1
    assert [int(r["pattern_index"]) == UNMATCHED for r in got["segments"][4]] == [False, False]
    assert texts(got, TEXT)[4:6] == ["hello ab", "ab hello ab"]
    # n_docs == 0
    got, _, _ = check(eng, [], opts, orc)
    assert got[TEXT] == [] and got["segments"] == []
    assert eng.segment_batch([], opts) == [] and eng.strip_prefix_batch([], opts) == []
    segs = eng.segment_batch(["zz hello", ""], opts)
    assert [s.as_str() for s in segs[0]] == ["zz ", "hello"] and segs[1] == []
    assert segs[0][0].unmatched().end == 3 and segs[0][1].matched().pattern.pattern == "hello"


# ---------------------------------------------------------------- 3. guard and ties

def test_guard_and_ties():
    """Pattern "a" with one edit at threshold 0 (test_gpu_replace_batch.test_guard_and_ties): empty
    matched segments, and two kept records of one start of which the guard drops the second. An empty
    matched segment pushes no bytes, so "ends with a space" must look at the accumulated result."""
    b = B().fuzzy(L().edits(1))
    eng, orc = b.build(["a"]), OracleEngine(b, ["a"])
    docs = ["a", "aa", "", "ba", "a b", "a\tb", "b a", "b\ta", " ", "bb b"]
    opts = O().threshold(0.0)
    sb = StagedBatch(eng, *batch_offsets(encode(docs)))
    recs, doc_off = sb.search_records(normalised(opts))
    rows = [[(int(r["start"]), int(r["end"])) for r in recs[int(doc_off[d]):int(doc_off[d + 1])]] for d in range(len(docs))]
    assert any(s == e for r in rows for s, e in r)  # empty spans are kept
    assert [d for d, r in enumerate(rows) if len({s for s, _ in r}) != len(r)]  # two records of one start
    got, compared, excluded = check(eng, docs, opts, orc, sb=sb)
    assert compared >= 1 and compared + excluded == len(docs)
    assert any(int(r["start"]) == int(r["end"]) and int(r["pattern_index"]) != UNMATCHED
               for segs in got["segments"] for r in segs)  # an empty matched segment
    assert got[TEXT][2] == b""


# ---------------------------------------------------------------- 4. whitespace

SPACES = ["\u0085", "\u00a0", "\u1680", "\u2003", "\u2028", "\u202f", "\u205f", "\u3000", "\t\n\x0b\x0c\r"]
NOT_SPACES = ["\x1c", "\x1d", "\x1e", "\x1f", "\u200b"]


def test_whitespace_is_rusts():
    b = B()
    eng = b.build(["hello"])
    opts = O().threshold(0.9)
    docs, want_prefix, want_suffix = [], [], []
    for w in SPACES:
        docs += ["hello" + w + "x" + w, w + "x" + w + "hello", w + "hello" + w, "hello" + w + w + "x y" + w + w + "hello"]
        want_prefix += ["x" + w, "x" + w + "hello", "", "x y" + w + w + "hello"]
        want_suffix += ["hello" + w + "x", w + "x", "", "hello" + w + w + "x y"]
    for c in NOT_SPACES:  # not whitespace: they stay
        docs += ["hello" + c + "x" + c, c + "x" + c + "hello", c + "hello" + c]
        want_prefix += [c + "x" + c, c + "x" + c + "hello", c + "hello" + c]
        want_suffix += ["hello" + c + "x" + c, c + "x" + c, c + "hello" + c]
    docs += [" \t\u3000\u2028 ",              # all whitespace
             "hel lo",                        # (no match at 0.9: whitespace in plain text)
             "  hello \u00a0 mid dle \u2003 hello  ",  # the only non-whitespace unmatched text is in the middle
             " hello hello "]
    want_prefix += ["", "hel lo", "mid dle \u2003 hello  ", ""]
    want_suffix += ["", "hel lo", "  hello \u00a0 mid dle", ""]
    got, _, _ = check(eng, docs, opts)
    assert texts(got, PREFIX) == want_prefix
    assert texts(got, SUFFIX) == want_suffix
    # whitespace only inside a matched span does not count
    b2 = B()
    eng2 = b2.build(["a b"])
    got, _, _ = check(eng2, ["a b", " a b ", "a bx", "xa b"], opts)
    assert texts(got, PREFIX) == ["", "", "x", "xa b"] and texts(got, SUFFIX) == ["", "", "a bx", "x"]


# ---------------------------------------------------------------- 5. segment_text punctuation

def test_segment_text_punctuation():
    b = B()
    eng, orc = b.build(["hello", "world"]), OracleEngine(b, ["hello", "world"])
    opts = O().threshold(0.9)
    docs, want = [], []
    for p in NO_LEADING_SPACE:
        docs.append("hello" + p + "x")
        want.append("hello" + p + "x")
    docs += ["hello\u2010x",      # U+2010 HYPHEN (E2 80 90) is not in the list: it gets the space
             "hello\u2015x", "helloéx",
             "helloworld",        # two adjacent matches
             "x hello", "x\thello", "xhello",  # a gap ending in a space, a tab, neither
             "x\u00a0hello",      # a no-break space is not U+0020
             "hello", "xx", ""]
    want += ["hello \u2010x", "hello \u2015x", "hello éx", "hello world", "x hello", "x\thello", "x hello",
             "x\u00a0 hello", "hello", "xx", ""]
    got, compared, _ = check(eng, docs, opts, orc)
    assert texts(got, TEXT) == want and compared == len(docs)


# ---------------------------------------------------------------- 6. mover shapes

def piece_residues(docs, got_text, eng, opts):
    """(output offset, source offset) of every piece's run over the batch, from E1's walk"""
    enc = encode(docs)
    sb = StagedBatch(eng, *batch_offsets(enc))
    recs, doc_off = sb.search_records(normalised(opts))
    pairs, src, out = [], 0, 0
    for d, doc in enumerate(enc):
        spans = [(int(r["start"]), int(r["end"])) for r in recs[int(doc_off[d]):int(doc_off[d + 1])]]
        at = out
        for space, s, e in e1_pieces(doc, e1_segments(doc, spans))[0]:
            at += 1 if space else 0
            pairs.append((at, src + s))
            at += e - s
        assert at - out == len(got_text[d])
        src += len(doc)
        out = at
    return pairs


def test_alignment_sweep():
    """Piece boundaries at every output offset mod 16 and every source offset mod 16: prefix documents
    of 0-17 bytes before a document with two matches, in segment_text and strip_prefix modes."""
    b = B()
    eng = b.build(["hello"])
    opts = O().threshold(0.9)
    out_res, src_res, pairs = set(), set(), set()
    strip_out, strip_src = set(), set()
    for q in range(18):
        docs = []
        for p in range(18):
            docs += ["z" * p, "y" * q + "hellocdefghijklmnopqrstuvwhello"]
        got, _, _ = check(eng, docs, opts)
        lead = "y" * q + " " if q else ""
        assert all(g == (lead + "hello cdefghijklmnopqrstuvw hello").encode() for g in got[TEXT][1::2])
        for oo, so in piece_residues(docs, got[TEXT], eng, opts):
            out_res.add(oo % 16)
            src_res.add(so % 16)
            pairs.add((oo % 16, so % 16))
        # strip_prefix: one piece per document, its source q + 6 bytes into the document
        docs = []
        for p in range(18):
            docs += ["z" * p, "hello" + " " * (q + 1) + "tail of twenty bytes hello x"]
        got, _, _ = check(eng, docs, opts)
        assert all(g == b"tail of twenty bytes hello x" for g in got[PREFIX][1::2])
        src = out = 0
        for d, g in zip(docs, got[PREFIX]):
            strip_out.add(out % 16)
            strip_src.add((src + len(d) - len(g)) % 16)
            src += len(d)
            out += len(g)
    assert out_res == set(range(16)) and src_res == set(range(16)) and len(pairs) > 128
    assert strip_out == set(range(16)) and strip_src == set(range(16))


def test_many_tiny_documents():
    """300 documents of 0-3 bytes: many documents and pieces inside one 16-byte chunk."""
    b = B()
    eng, orc = b.build(["a"]), OracleEngine(b, ["a"])
    rng = Rng(0x7157)
    docs = ["".join("ab "[rng.next() % 3] for _ in range(rng.next() % 4)) for _ in range(300)]
    assert {len(d) for d in docs} == {0, 1, 2, 3}
    _, compared, excluded = check(eng, docs, O().threshold(0.9), orc)
    assert excluded == 0 and compared == 300


@pytest.mark.parametrize("shift", [-1, 0, 1])
def test_tile_edges(shift):
    """A document boundary and an inserted space at the copy kernel's tile size - 1, + 0, + 1."""
    b = B()
    eng = b.build(["hello"])
    opts = O().threshold(0.9)
    fill = "zyxwv" * (TILE // 5 + 2)
    edge = TILE + shift
    # document boundary at output offset `edge` (all three modes: nothing to strip in document 0)
    got, _, _ = check(eng, [fill[:edge], "hello tail", "", "x"], opts)
    # (matches.rs:583-588: a space goes before " tail" as well, a space is no punctuation)
    assert texts(got, TEXT)[:2] == [fill[:edge], "hello  tail"] and got[PREFIX][1] == b"tail"
    # the inserted space at output offset `edge`, and the ones around it
    for lead in (edge, edge - 1, edge - 5, edge - 6):
        doc = fill[:lead] + "hello" + fill[:40]
        got, _, _ = check(eng, [doc, "hello"], opts)
        assert texts(got, TEXT)[0] == fill[:lead] + " hello " + fill[:40]
    # a strip's piece starts right at the tile edge of the output
    got, _, _ = check(eng, [fill[:edge], "hello " + fill[:100]], opts)
    assert got[PREFIX] == [fill[:edge].encode(), fill[:100].encode()]


def test_document_longer_than_two_tiles():
    b = B().fuzzy(L().edits(1))
    eng = b.build(["hello", "world"])
    opts = O().threshold(0.8)
    parts, n = [], 0
    rng = Rng(0x10c)
    while n < 2 * TILE + 700:
        w = ["hello", "wxrld", "helo", "world"][rng.next() % 4] if rng.next() % 3 == 0 else "q" * (1 + rng.next() % 23)
        parts.append(w + ("" if rng.next() % 2 else " "))
        n += len(parts[-1])
    doc = "".join(parts)
    doc = doc[:TILE - 2] + "hello" + doc[TILE + 3:2 * TILE - 6] + " world" + doc[2 * TILE:]
    got, _, _ = check(eng, ["hello", " hello " + doc + " hello ", "", doc[:100]], opts)
    assert len(got[TEXT][1]) > 2 * TILE and len(got[PREFIX][1]) > 2 * TILE and len(got[SUFFIX][1]) > 2 * TILE
    assert len(got[TEXT][1]) != len(doc) + 14  # some space was inserted


def test_whole_output_empty():
    b = B()
    eng, orc = b.build(["hello"]), OracleEngine(b, ["hello"])
    got, compared, _ = check(eng, ["hello", "", " hello ", "hello hello", " \t "], O().threshold(0.9), orc)
    assert compared == 5
    assert got[PREFIX] == [b""] * 5 and got[SUFFIX] == [b""] * 5
    got, _, _ = check(eng, ["", "", ""], O().threshold(0.9), orc)
    assert got[TEXT] == [b""] * 3 and all(len(s) == 0 for s in got["segments"])


# ---------------------------------------------------------------- 7. options

def test_orders_choose_the_candidate():
    b = B().fuzzy(L().edits(1))
    pats = ["hello", "hellos", "vest", "vestibulum"]
    eng, orc = b.build(pats), OracleEngine(b, pats)
    docs = ["hello!", "vestibulun", "say hello! to vestibulun"]
    res = {}
    for order in (Order.Default, Order.Greedy, Order.CoverageWeighted):
        res[order], compared, _ = check(eng, docs, options(0.7, order), orc)
        assert compared == len(docs)
    assert res[Order.Greedy]["segments"][0].tobytes() != res[Order.Default]["segments"][0].tobytes()
    assert res[Order.CoverageWeighted]["segments"][1].tobytes() != res[Order.Default]["segments"][1].tobytes()


def test_unique_is_per_document():
    b = B()
    pats = [Pattern("ab").custom_unique_id(1), Pattern("cd").custom_unique_id(1)]
    eng, orc = b.build(pats), OracleEngine(b, pats)
    docs = ["ab cd ab", "cd ab", "ab", "cd"]
    got, compared, _ = check(eng, docs, options(0.9, overlap=Overlap.NonOverlappingUnique), orc)
    assert compared == 4
    assert got[PREFIX] == [b"cd ab", b"ab", b"", b""]  # once per document, not once per batch
    assert got["split"] == [[" cd ab"], [" ab"], [], []]
    got, _, _ = check(eng, docs, options(0.9), orc)
    assert got[PREFIX] == [b""] * 4 and got["split"] == [[" ", " "], [" "], [], []]


def test_unsorted_keep_is_normalised():
    b = B().fuzzy(L().edits(1))
    pats = ["hello", "hell", "lo w", "world"]
    eng, orc = b.build(pats), OracleEngine(b, pats)
    docs = ["hello world", "helo wrld hello", "", "lo wo"]
    a, _, _ = check(eng, docs, options(0.6, Order.Unsorted, Overlap.Keep), orc)
    c, _, _ = check(eng, docs, options(0.6, Order.Default, Overlap.NonOverlapping), orc)
    for mode in MODES + ("split",):
        assert a[mode] == c[mode]
    assert [x.tobytes() for x in a["segments"]] == [x.tobytes() for x in c["segments"]]


# ---------------------------------------------------------------- 8. random differential

N_BATCHES = 40


@pytest.mark.parametrize("cache", ["off", "k4"])
def test_random_differential(cache, monkeypatch):
    """The first 40 batches of each seed of test_gpu_batch, Default x {NonOverlapping,
    NonOverlappingUnique}: E1 on every document, E2 where allowed. (The vocabularies and fillers of
    that generator hold none of U+001C-U+001F, so the exclusions are the ties of the replace test.)"""
    set_knobs(monkeypatch, cache, False)
    compared = excluded = stripped = spaces = 0
    for seed, vocab in SEEDS:
        rng = Rng(seed)
        for _ in range(N_BATCHES):
            b, pats, docs, thr = random_batch(rng, vocab)
            assert not any(c in d for d in docs for c in HOST_ONLY_SPACE)
            eng, orc = b.build(pats), OracleEngine(b, pats)
            enc = encode(docs)
            sb = StagedBatch(eng, *batch_offsets(enc))
            for overlap in (Overlap.NonOverlapping, Overlap.NonOverlappingUnique):
                got, c, x = check(eng, docs, options(thr, overlap=overlap), orc, sb=sb)
                compared += c
                excluded += x
                for d, doc in enumerate(enc):
                    stripped += 0 < len(got[PREFIX][d]) < len(doc) or 0 < len(got[SUFFIX][d]) < len(doc)
                    spaces += len(got[TEXT][d]) > len(doc)
    share = excluded / (compared + excluded)
    print(f"E2 compared {compared}, excluded {excluded} ({100 * share:.2f} %), documents stripped {stripped}, "
          f"with an inserted space {spaces}")
    assert share <= 0.05
    assert stripped > 0 and spaces > 0


# ---------------------------------------------------------------- 9. device output

def _device(docs):
    import torch
    data, off = batch_offsets(encode(docs))
    t = torch.from_numpy(np.frombuffer(data or b"\0", dtype=np.uint8).copy()).cuda()
    o = torch.from_numpy(np.asarray(off, dtype=np.uint64).view(np.int64).copy()).cuda()
    return data, off, t, o


DEV_DOCS = ["hello world", "", "  helo wrld hello  ", "wörld", "x" * 50, "helloworld"]


@pytest.mark.parametrize("mode", MODES)
def test_device_output_bytes(mode):
    import torch
    b = B().fuzzy(L().edits(1))
    eng = b.build(["hello", "world"])
    opts = O().threshold(0.6)
    want, _, _ = check(eng, DEV_DOCS, opts)
    sb = StagedBatch(eng, *batch_offsets(encode(DEV_DOCS)))
    host, host_off = sb.render_bytes(mode, opts)
    n = len(host)
    assert host == b"".join(want[mode]) and n > 16
    small = torch.full((n - 1,), 0xAB, dtype=torch.uint8, device="cuda")
    with pytest.raises(DeviceError) as ei:
        sb.render_bytes(mode, opts, out=small)
    assert ei.value.code == _native.FAC_E_OUTPUT_CAPACITY and ei.value.needed == n
    assert bool((small == 0xAB).all())  # nothing was written
    for pad in (0, 1):  # a 16-byte aligned buffer, and one that is not
        buf = torch.full((n + 32,), 0xCD, dtype=torch.uint8, device="cuda")
        exact = buf[pad:pad + n]
        dev_off = torch.full((len(DEV_DOCS) + 1,), -1, dtype=torch.int64, device="cuda")
        got, got_off = sb.render_bytes(mode, opts, out=exact, offsets_out=dev_off)
        assert got.cpu().numpy().tobytes() == host and list(got_off) == list(host_off)
        assert dev_off.cpu().tolist() == [int(x) for x in host_off]
        assert bool((buf[:pad] == 0xCD).all()) and bool((buf[pad + n:] == 0xCD).all())  # and nothing beside it


def test_device_output_segments():
    import torch
    b = B().fuzzy(L().edits(1))
    eng = b.build(["hello", "world"])
    opts = O().threshold(0.6)
    sb = StagedBatch(eng, *batch_offsets(encode(DEV_DOCS)))
    host, host_off = sb.segment_records(opts)
    n = len(host)
    assert n > 8
    small = torch.full(((n - 1) * 32,), 0xAB, dtype=torch.uint8, device="cuda")
    with pytest.raises(DeviceError) as ei:
        sb.segment_records(opts, out=small)
    assert ei.value.code == _native.FAC_E_OUTPUT_CAPACITY and ei.value.needed == n
    assert bool((small == 0xAB).all())
    for pad in (0, 1):
        buf = torch.full((n * 32 + 64,), 0xCD, dtype=torch.uint8, device="cuda")
        exact = buf[pad:pad + n * 32]
        dev_off = torch.full((len(DEV_DOCS) + 1,), -1, dtype=torch.int64, device="cuda")
        got, got_off = sb.segment_records(opts, out=exact, doc_offsets_out=dev_off)
        assert got.cpu().numpy().tobytes() == host.tobytes() and list(got_off) == list(host_off)
        assert dev_off.cpu().tolist() == [int(x) for x in host_off]
        assert bool((buf[:pad] == 0xCD).all()) and bool((buf[pad + n * 32:] == 0xCD).all())


def test_restaged_batch_gives_its_own_answer():
    b = B().fuzzy(L().edits(1))
    eng = b.build(["hello", "world"])
    opts = O().threshold(0.6)
    first = ["hello world", " zz", "wrld "]
    second = ["no", "helo " * 30, "", "worldhello", "q"]
    want = [check(eng, dd, opts)[0] for dd in (first, second)]
    keep, sb = [], None
    for which in (0, 1, 0):
        data, off, t, o = _device((first, second)[which])
        keep.append((t, o))
        sb = StagedBatch.from_device(eng, t.data_ptr(), o.data_ptr(), len(off) - 1, len(data), reuse=sb)
        for mode in MODES:
            out, offs = sb.render_bytes(mode, opts)
            assert [out[int(offs[d]):int(offs[d + 1])] for d in range(len(off) - 1)] == want[which][mode]
        segs, soff = sb.segment_records(opts)
        assert [segs[int(soff[d]):int(soff[d + 1])].tobytes() for d in range(len(off) - 1)] == \
            [s.tobytes() for s in want[which]["segments"]]


# ---------------------------------------------------------------- 10. pre-filtered forms

def test_prefiltered_forms():
    import torch
    pats = ["hello", "world", "cell", "abcdefg", "saddam", "hussein8"]
    b = B().fuzzy(L().edits(1)).case_insensitive(True)
    eng = b.build(pats)
    thr = 0.75
    opts = O().threshold(thr)
    assert eng.with_prefilter().is_active()
    docs = ["hello world", "", "  helo wrld hello  ", "cellabcdefg", "zz", "sadam husein8 zz", "q" * 70 + "hello"]
    sb = StagedBatch(eng, *batch_offsets(encode(docs)))
    assert sb.prefilter_windows(thr) is not None  # the filter runs at this threshold
    pf, _, _ = check(eng, docs, opts, sb=sb, prefilter=True)  # E1 over search_records(prefilter=True)
    plain, _, _ = check(eng, docs, opts, sb=sb)
    a, a_off = sb.search_records(normalised(opts), prefilter=True)
    p, p_off = sb.search_records(normalised(opts))
    same = 0
    for d in range(len(docs)):
        if a[int(a_off[d]):int(a_off[d + 1])].tobytes() == p[int(p_off[d]):int(p_off[d + 1])].tobytes():
            same += 1
            for mode in MODES + ("split",):
                assert pf[mode][d] == plain[mode][d]
            assert pf["segments"][d].tobytes() == plain["segments"][d].tobytes()
    assert same >= 4
    assert eng.with_prefilter().segment_text_batch(docs, opts) == texts(pf, TEXT)
    assert eng.with_prefilter().strip_prefix_batch(docs, opts) == texts(pf, PREFIX)
    assert eng.with_prefilter().strip_suffix_batch(docs, opts) == texts(pf, SUFFIX)
    assert eng.with_prefilter().split_batch(docs, opts) == pf["split"]
    # a non-ASCII document: FAC_E_UNSUPPORTED with nothing written
    mixed = StagedBatch(eng, *batch_offsets(encode(["hello world", "wörld hello", "cell"])))
    buf = torch.full((64 * 32,), 0xAB, dtype=torch.uint8, device="cuda")
    for mode in MODES:
        with pytest.raises(UnsupportedConfiguration):
            mixed.render_bytes(mode, opts, prefilter=True, out=buf)
    with pytest.raises(UnsupportedConfiguration):
        mixed.segment_records(opts, prefilter=True, out=buf)
    assert bool((buf == 0xAB).all())
    assert len(mixed.render_bytes(TEXT, opts)[0]) > 0  # the plain call still takes the batch
    # the Python conveniences send the non-ASCII text through the per-document search
    pre = eng.with_prefilter()
    both = ["helloworld", "wörldhello", "cell zz"]
    assert pre.segment_text_batch(both, opts) == [pre._segmented(t, opts).segment_text() for t in both]
    assert pre.split_batch(both, opts) == [list(pre._segmented(t, opts).split()) for t in both]
    # an engine with no active filter: exactly the unfiltered call, for any batch
    bm = B().fuzzy(L().edits(1)).mapping("ss", "ß")
    em = bm.build(["strasse", "hello"])
    assert not em.with_prefilter().is_active()
    sm = StagedBatch(em, *batch_offsets(encode(["strasse hello", "", "hello strase", "zz"])))
    mo = O().threshold(0.7)
    for mode in MODES:
        x, xo = sm.render_bytes(mode, mo, prefilter=True)
        y, yo = sm.render_bytes(mode, mo)
        assert x == y and list(xo) == list(yo)
    x, xo = sm.segment_records(mo, prefilter=True)
    y, yo = sm.segment_records(mo)
    assert x.tobytes() == y.tobytes() and list(xo) == list(yo) and len(x) >= 4


# ---------------------------------------------------------------- 11. errors

def test_errors():
    b = B()
    eng = b.build(["hello", "world"])
    sb = StagedBatch(eng, *batch_offsets([b"hello"]))
    for mode in (-1, 3, 99):
        with pytest.raises(DeviceError) as ei:
            sb.render_bytes(mode, O().threshold(0.9))
        assert ei.value.code == _native.FAC_E_INVALID
    bm = B().fuzzy(L().edits(1)).mapping("ss", "ß")
    em = bm.build(["strasse"])
    assert em.segment_text_batch(["xstrasse", "x"], O().threshold(0.9)) == ["x strasse", "x"]  # ASCII documents are fine
    with pytest.raises(UnsupportedConfiguration):  # as fac_search_batch
        em.segment_text_batch(["strasse", "straße"], O().threshold(0.9))
    with pytest.raises(UnsupportedConfiguration):
        em.segment_batch(["strasse", "straße"], O().threshold(0.9))
    import torch
    if torch.cuda.device_count() >= 2:  # a batch staged for another engine's device
        eng1 = B().device(1).build(["hello", "world"])
        sb1 = StagedBatch(eng1, *batch_offsets([b"hello"]))
        sb1.engine = eng
        with pytest.raises(DeviceError) as ei:
            sb1.render_bytes(TEXT, O().threshold(0.9))
        assert ei.value.code == _native.FAC_E_INVALID
        with pytest.raises(DeviceError) as ei:
            sb1.segment_records(O().threshold(0.9))
        assert ei.value.code == _native.FAC_E_INVALID


# ---------------------------------------------------------------- 12. the list-returning methods

def test_list_methods_equal_the_per_document_methods():
    b = B().fuzzy(L().edits(1)).case_insensitive(True)
    eng = b.build(["hello", "wörld", "lorem", "ipsum"])
    opts = O().threshold(0.75)
    batch = ["", "  Hello, wörld!  ", "LrEM ISuM Lorm ZZZ", "ZZZ lorem\tipsum", "helloworld…", "no match at all",
             "\u3000hello\u3000x\u3000", "wôrld—hello", "é", "hello"]
    assert not any(c in t for t in batch for c in HOST_ONLY_SPACE)
    assert eng.strip_prefix_batch(batch, opts) == [eng.strip_prefix(t, opts) for t in batch]
    assert eng.strip_suffix_batch(batch, opts) == [eng.strip_suffix(t, opts) for t in batch]
    assert eng.segment_text_batch(batch, opts) == [eng.segment_text(t, opts) for t in batch]
    assert eng.split_batch(batch, opts) == [list(eng.split(t, opts)) for t in batch]
    segs = eng.segment_batch(batch, opts)
    want = [list(eng.segment_iter(t, opts)) for t in batch]
    assert [[(s.matched() is not None, s.as_str()) for s in d] for d in segs] == \
        [[(s.matched() is not None, s.as_str()) for s in d] for d in want]
    assert [[s.matched() for s in d if s.matched() is not None] for d in segs] == \
        [[s.matched() for s in d if s.matched() is not None] for d in want]
