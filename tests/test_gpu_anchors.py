"""Anchored matches on the device (fac_batch_require_anchors, fac_lookup_batch, anchor_kernels.hip):
every batch call of a flagged batch gives, per document, apply(order, overlap) of the document's raw
records with the anchor rule of DESIGN.md 6a applied first, and a plain call searches only the start
windows such a record can come from. Every expected value is the CPU oracle's search_raw of the
document alone, filtered by the two-line predicate below (and test_boundaries_host's reference of the
whole-token rule where both masks are set), then the oracle's apply and the host's replace /
segment_iter / strip_* / segment_text, composed as test_gpu_boundaries.py does it. Comparisons are
bit-exact, similarity bits included."""
import hashlib
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # the child of test_past_the_cache_threshold
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import oracle_harness  # noqa: F401  (puts the package on sys.path)

from fuzzy_aho_corasick import (Anchor, Boundary, DeviceError, FuzzyAhoCorasickBuilder as B, FuzzyLimits as L,
                                FuzzyReplacer, Order, Overlap, Pattern, StagedBatch, Wrap, _native, batch_offsets)
from test_boundaries_host import ref_ok
from test_gpu_boundaries import (COMBOS, TWO, Ref, canon, check_every_call, check_records, device_batch, options, rows_of,
                                 sim_bits, staged)

pytestmark = pytest.mark.gpu

MASKS = (Anchor.NONE, Anchor.START, Anchor.END, Anchor.WHOLE)
THR = 0.5


def anchored(doc_len, start, end, sides):
    """The rule: start == 0 if START is requested, end == the document's length if END is."""
    return (not sides & 1 or start == 0) and (not sides & 2 or end == doc_len)


class Sides(int):
    """An anchor mask and a boundary mask travelling through test_gpu_boundaries' helpers as one value."""

    def __new__(cls, anchors, boundaries=0):
        obj = int.__new__(cls, int(anchors) | int(boundaries) << 2)
        obj.anchors, obj.boundaries = int(anchors), int(boundaries)
        return obj


class ARef(Ref):
    """test_gpu_boundaries.Ref with the anchor predicate (and the whole-token reference when set)."""

    def applied(self, doc, opts, sides, prefilter=False):
        data = doc.encode("utf-8")
        rows = [r for r in self.raw_rows(doc, opts.threshold_, prefilter)
                if anchored(len(data), r[0], r[1], sides.anchors)
                and (not sides.boundaries or ref_ok(data, r[0], r[1], sides.boundaries))]
        if opts.order_ == Order.Unsorted and opts.overlap_ != Overlap.Keep:
            rows = sorted(rows, key=lambda r: r[:3])
        return self.orc.apply_rows(rows, opts.order_, opts.overlap_)


# ---------------------------------------------------------------- the ASCII shapes

PATS = ["abc", "abcd", "bcd", "b", "dab"]  # five, so test_gpu_boundaries' PLAIN and WRAPS tables fit


def ascii_builder():
    return B().fuzzy(L().edits(1))


def ascii_docs(mmg):
    """The smallest documents at which an anchored search can go wrong (T = mmg + 2)."""
    t = mmg + 2
    docs = [
        "cd",                      # first document: device staging puts "b" bytes right before it
        "", "b", "x",              # empty, one grapheme (a pattern, and not)
        "abc", "abcd", "bcd",      # equal to a pattern
        "xbc", "xbcd",             # first grapheme edited
        "abx", "abcx",             # last grapheme edited ("abcx": also "abc" with one behind)
        "xabc", "zabcd",           # one extra grapheme in front
        "abcz", "abcdz",           # one extra grapheme behind
        "bc", "ab", "acd",         # a grapheme deleted at the front, at the end, inside
        "abcdzzzz",                # the pattern as a proper prefix only
        "zzzzabcd",                # ... as a proper suffix only
        "zzabcdzz",                # ... in the middle only
        "z" * (t + 5 - 4) + "abcd",            # T + 5 graphemes, the last ones a pattern
        "z" * 6 + "abxcd"[:mmg].rjust(mmg, "z"),  # a match of mmg graphemes ends the document
        "z" * (t - 3) + "abc", "z" * (t - 2) + "abc",  # the pattern's start just inside / outside the last T windows
        "ab", "c", "a", "bcd",     # neighbours "ab" | "c" and "a" | "bcd": nothing is found across an edge
        "", "a",                   # last document: device staging puts "b" bytes right after it
    ]
    return docs


@pytest.fixture(scope="module")
def plain():
    b = ascii_builder()
    eng, ref = b.build(PATS), ARef(b, PATS)
    return eng, ref, ascii_docs(eng.max_match_graphemes())


def test_the_shapes_are_what_they_claim(plain):
    eng, ref, docs = plain
    mmg = eng.max_match_graphemes()
    assert mmg == 5 and "zzzzzzabxcd" in docs
    raw = ref.rows("zzzzzzabxcd", options(THR), Sides(0))
    assert any(r[0] == 11 - mmg and r[1] == 11 for r in raw)  # its first grapheme sits mmg graphemes from the end
    for sides in MASKS[1:]:  # every mask keeps something and drops something
        kept = sum(len(ref.rows(d, options(THR), Sides(sides))) for d in docs)
        assert 0 < kept < sum(len(ref.rows(d, options(THR), Sides(0))) for d in docs)
    whole = {d: [r[2] for r in ref.rows(d, options(THR), Sides(3))] for d in docs}
    assert whole["abc"] and whole["xbc"] and whole["abx"] and whole["abcz"] and whole["bc"] and whole["ab"]
    assert not whole["xabc"]  # (the crate never starts a match with an inserted grapheme: "abc" begins at byte 1)
    assert not whole["abcdzzzz"] and not whole["zzzzabcd"] and not whole["zzabcdzz"] and not whole[""]
    assert ref.rows("zzzzabcd", options(THR), Sides(2)) and not ref.rows("zzzzabcd", options(THR), Sides(1))
    assert ref.rows("abcdzzzz", options(THR), Sides(1)) and not ref.rows("abcdzzzz", options(THR), Sides(2))


@pytest.mark.parametrize("where", ["host", "device"])
def test_search_records_every_mask(plain, where):
    """All four masks x every (order, overlap), staged from host memory and from device memory with
    letters right before the first document and right after the last."""
    eng, ref, docs = plain
    sb, keep = (staged(eng, docs), None) if where == "host" else device_batch(eng, docs, pad=b"b")
    for sides in MASKS:
        assert sb.require_anchors(sides) is sb
        check_records(sb, ref, docs, THR, Sides(sides), COMBOS)
    del keep


@pytest.mark.parametrize("prefilter", [False, True])
def test_every_call_takes_the_flag(plain, prefilter):
    """replace (plain, keep and Wrap entries), extract, segments, the three render modes and the
    records left in HBM, every mask, plain and pre-filtered."""
    eng, ref, docs = plain
    if prefilter:
        assert eng.with_prefilter().is_active()
    sb = staged(eng, docs)
    for sides in MASKS:
        sb.require_anchors(sides)
        check_every_call(eng, ref, sb, docs, THR, Sides(sides), prefilter=prefilter)
        check_records(sb, ref, docs, THR, Sides(sides), COMBOS, prefilter=prefilter)


def test_anchors_with_boundaries(plain):
    eng, ref, _ = plain
    docs = ["abc", "abc d", "x abc", "abc-abcd", "abcd abc", "abcx", " abc", "abc_", "b b", "", "zabcd abc"]
    for anchors in MASKS:
        for bounds in (Boundary.WHOLE, Boundary.START):
            sb = staged(eng, docs, boundaries=bounds, anchors=anchors)
            check_records(sb, ref, docs, THR, Sides(anchors, bounds), TWO)
    both = [ref.rows(d, options(THR), Sides(2, 3)) for d in docs]
    assert both != [ref.rows(d, options(THR), Sides(2, 0)) for d in docs]
    assert both != [ref.rows(d, options(THR), Sides(0, 3)) for d in docs]


def test_flag_lifetime(plain):
    eng, ref, docs = plain
    other = ["zzabc", "abcd", "", "bcdzz", "b"]
    sb, keep = device_batch(eng, docs, pad=b"b", anchors=Anchor.END)
    check_records(sb, ref, docs, THR, Sides(2), TWO)
    sb2, keep2 = device_batch(eng, other, pad=b"b", reuse=sb)  # restaged in place: the flag stays
    assert sb2 is sb
    check_records(sb, ref, other, THR, Sides(2), TWO)
    assert [ref.rows(d, options(THR), Sides(2)) for d in other] != [ref.rows(d, options(THR), Sides(0)) for d in other]
    sb.require_boundaries(Boundary.START)  # the two masks are independent
    check_records(sb, ref, other, THR, Sides(2, 1), TWO)
    sb.require_boundaries(0)
    check_records(sb, ref, other, THR, Sides(2), TWO)
    assert sb.require_anchors(0) is sb  # switched back: the unflagged result
    check_records(sb, ref, other, THR, Sides(0), COMBOS)
    for bad in (4, -1):
        with pytest.raises(DeviceError) as ei:
            sb.require_anchors(bad)
        assert ei.value.code == _native.FAC_E_INVALID
    check_records(sb, ref, other, THR, Sides(0), TWO)  # a refused mask leaves the old one
    del keep, keep2


# ---------------------------------------------------------------- non-ASCII documents

EDGES = ["é", "日", "\U0001d49c", "é", "\r\n"]  # 2, 3 and 4 bytes, base + mark, CR LF


def unicode_docs():
    docs = []
    for g in EDGES:
        docs += [g + "abc", "abc" + g, g + "abc" + g, g, g + "b", "b" + g]
    return docs + ["Éabc", "ABC", "日本", "x日本", "日本x", "", "abc", "éabcd\r\n"]


def test_non_ascii_documents():
    """Documents whose first or last grapheme is 2, 3 or 4 bytes long, a base with a combining mark or
    CR LF, on a case-insensitive engine: offsets are bytes of the document."""
    b = B().fuzzy(L().edits(1)).case_insensitive(True)
    pats = ["abc", "éabc", "abc日", "日本", "b", "éabc", "abc\r\n", "\U0001d49cabc\U0001d49c"]
    eng, ref = b.build(pats), ARef(b, pats)
    docs = unicode_docs()
    sb, keep = device_batch(eng, docs, pad="é".encode("utf-8"))
    for sides in MASKS:
        check_records(sb.require_anchors(sides), ref, docs, THR, Sides(sides), COMBOS)
    whole = [ref.rows(d, options(THR), Sides(3)) for d in docs]
    for g in EDGES[:3]:  # a multi-byte grapheme at either end is inside a whole-document match
        assert any(r[1] == len((g + "abc").encode()) for r in whole[docs.index(g + "abc")])
        assert any(r[1] == len(("abc" + g).encode()) for r in whole[docs.index("abc" + g)])
    del keep
    sb = staged(eng, docs, unicode_prefilter=True)  # the opted-in pre-filtered form: the filter only
    assert eng.with_prefilter().is_active()
    for sides in MASKS:
        check_records(sb.require_anchors(sides), ref, docs, THR, Sides(sides), TWO, prefilter=True)


def test_mapping_engine():
    b = B().fuzzy(L().edits(1)).case_insensitive(True).mapping("ß", "ss")
    pats = ["straße", "groß"]
    eng, ref = b.build(pats), ARef(b, pats)
    docs = ["Straße", "strasse", "xstraße", "straßen", "die straße", "groß", "gross", "GROSS!", "",
            "großstrasse"]
    sb = staged(eng, docs, unicode_mappings=True)
    for sides in MASKS:
        check_records(sb.require_anchors(sides), ref, docs, 0.8, Sides(sides), COMBOS)
    assert [r[2] for r in ref.rows("strasse", options(0.8), Sides(3))] == [0]
    assert [ref.rows(d, options(0.8), Sides(3)) for d in docs] != [ref.rows(d, options(0.8), Sides(0)) for d in docs]


# ---------------------------------------------------------------- engines

def windows_of(sb, opts):
    st = _native.fac_stats()
    sb.search_records(opts, stats=st)
    return int(st.windows)


def test_beam_engine(plain):
    _, _, docs = plain
    b = ascii_builder().beam_width(3)
    eng, ref = b.build(PATS), ARef(b, PATS)
    sb = staged(eng, docs)
    for sides in MASKS:
        check_records(sb.require_anchors(sides), ref, docs, THR, Sides(sides), COMBOS)
    assert windows_of(sb.require_anchors(3), options(THR)) == sum(1 for d in docs if d)  # restricted like any plain engine


def test_auto_beam_engine_searches_every_window(plain):
    """An auto-beam-only engine whose budget runs out inside the documents: the running total needs
    every window in order, so the call searches what the unflagged call searches and gets the filter
    only. END is the mask the restriction would break: its windows come after the switch point."""
    _, _, docs = plain
    docs = docs + ["abcdabcdabcdabcdabcdzabcd", "bcdbcdbcdbcdbcdbcdabc"]
    b = ascii_builder().auto_beam(12, 1)
    eng, ref = b.build(PATS), ARef(b, PATS)
    unbeamed = ARef(ascii_builder(), PATS)
    assert any(ref.rows(d, options(THR), Sides(2)) != unbeamed.rows(d, options(THR), Sides(2)) for d in docs)  # the switch bites
    sb = staged(eng, docs)
    full = windows_of(sb, options(THR))
    assert full >= sum(len(d) for d in docs)  # (the counting pass, then the windows after each switch point again)
    for sides in MASKS:
        check_records(sb.require_anchors(sides), ref, docs, THR, Sides(sides), COMBOS)
        assert windows_of(sb, options(THR)) == full


def test_per_pattern_limits(plain):
    _, _, docs = plain
    b = ascii_builder()
    pats = [Pattern("abc").fuzzy(L().edits(0)), Pattern("abcd").fuzzy(L().edits(2)), "bcd", Pattern("b").fuzzy(L().edits(0)),
            "dab"]
    eng, ref = b.build(pats), ARef(b, pats)
    docs = docs + ["abd", "axyd", "zzzzzzzzzzaxcdx", "abcdxx"]
    sb = staged(eng, docs)
    for sides in MASKS:
        check_records(sb.require_anchors(sides), ref, docs, THR, Sides(sides), COMBOS)


# ---------------------------------------------------------------- the restriction really happens

def test_windows_searched(plain):
    eng, _, docs = plain
    t = eng.max_match_graphemes() + 2
    opts = options(THR)
    full = windows_of(staged(eng, docs), opts)
    assert full == sum(len(d) for d in docs)
    sb = staged(eng, docs)
    nonempty = sum(1 for d in docs if d)
    assert windows_of(sb.require_anchors(0), opts) == full
    for sides in (Anchor.START, Anchor.WHOLE):
        assert 0 < windows_of(sb.require_anchors(sides), opts) <= nonempty
    assert 0 < windows_of(sb.require_anchors(Anchor.END), opts) <= sum(min(len(d), t) for d in docs) < full
    one = staged(eng, ["b"], anchors=Anchor.END)
    assert windows_of(one, opts) == 1
    assert windows_of(staged(eng, ["", ""], anchors=Anchor.WHOLE), opts) == 0


# ---------------------------------------------------------------- past the prefix cache's threshold

def cache_docs():
    """4100 distinct documents of 6 to 10 bytes that share three first characters."""
    docs = []
    for i in range(4100):
        tail = "".join(chr(97 + (i // 26 ** k) % 26) for k in (2, 1, 0))
        docs.append(["abc", "abd", "bcd"][i % 3] + tail + "abcd"[:i % 5])
    assert len(set(docs)) == 4100 and {len(d) for d in docs} == {6, 7, 8, 9, 10}
    return docs


CACHE_PATS = ["abcd", "bcd"] + cache_docs()[::300]  # some documents are entries, their neighbours near-entries


def cache_run(eng, docs, sides):
    sb = staged(eng, docs, anchors=sides)
    st = _native.fac_stats()
    recs, doc_off = sb.search_records(options(THR, Order.Default, Overlap.Keep), stats=st)
    return recs, doc_off, st


def digest(recs, doc_off):
    return hashlib.sha256(recs.tobytes() + np.asarray(doc_off, dtype=np.uint64).tobytes()).hexdigest()


def test_past_the_cache_threshold():
    """4100 one-window segments reach the prefix cache (a batch turns it on from 4096 windows).
    Expected: the same batch searched unflagged (existing, tested code), filtered by the predicate and
    ranked by the oracle's apply; and the same again in a child process with the cache off."""
    b = ascii_builder()
    eng, ref = b.build(CACHE_PATS), ARef(b, CACHE_PATS)
    docs = cache_docs()
    raw, raw_off = staged(eng, docs).search_records(options(THR))
    rows = [(int(r["start"]), int(r["end"]), int(r["pattern_index"]), float(r["similarity"]), int(r["insertions"]),
             int(r["deletions"]), int(r["substitutions"]), int(r["swaps"]), int(r["edits"])) for r in raw]
    mine = {}
    for sides in (Anchor.WHOLE, Anchor.END):
        recs, doc_off, st = cache_run(eng, docs, sides)
        narrowed = 4100 if sides == Anchor.WHOLE else sum(min(len(d), eng.max_match_graphemes() + 2) for d in docs)
        assert int(st.windows) in (narrowed, 2 * narrowed)  # (twice: the record buffer grew and the search ran again)
        got = rows_of(recs)
        n_kept = 0
        for d, doc in enumerate(docs):
            own = [r for r in rows[int(raw_off[d]):int(raw_off[d + 1])] if anchored(len(doc), r[0], r[1], int(sides))]
            want = [(r[0], r[1], r[2], sim_bits(r[3])) + tuple(r[4:]) for r in ref.orc.apply_rows(own, Order.Default, Overlap.Keep)]
            assert got[int(doc_off[d]):int(doc_off[d + 1])] == want, (int(sides), d, doc)
            n_kept += len(want)
        assert n_kept > 40 and int(doc_off[-1]) == n_kept
        mine[str(int(sides))] = digest(recs, doc_off)
    env = dict(os.environ, FAC_DIAGNOSTICS="1", FAC_NO_RC="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    child = json.loads(r.stdout.strip().splitlines()[-1])
    assert child["cached"] == 0
    assert {k: child[k] for k in mine} == mine


def child_main():
    eng = ascii_builder().build(CACHE_PATS)
    docs = cache_docs()
    out = {"cached": 0}
    for sides in (Anchor.WHOLE, Anchor.END):
        recs, doc_off, st = cache_run(eng, docs, sides)
        out[str(int(sides))] = digest(recs, doc_off)
        out["cached"] += int(st.states_cached)
    print(json.dumps(out))


# ---------------------------------------------------------------- the dense table

FILLER = struct.pack("<QQIfBBBBB3x", 0, 0, _native.FAC_UNMATCHED, 0.0, 0, 0, 0, 0, 0)


def check_table(recs, found, ref, docs, order, k):
    assert recs.shape == (len(docs), k) and found.dtype == np.uint32 and len(found) == len(docs)
    opts = options(THR, Order.Default if order == Order.Unsorted else order, Overlap.Keep)
    for d, doc in enumerate(docs):
        want = ref.rows(doc, opts, Sides(3))[:k]
        assert int(found[d]) == len(want), (order, k, d, doc)
        assert rows_of(recs[d, :len(want)]) == want, (order, k, d, doc)
        for s in range(len(want), k):
            assert recs[d, s].tobytes() == FILLER, (order, k, d, s)


def test_lookup_records(plain):
    import torch
    eng, ref, docs = plain
    sb = staged(eng, docs)
    assert max(len(ref.rows(d, options(THR), Sides(3))) for d in docs) >= 3  # k = 3 cuts some rows
    for order in Order:
        for k in (1, 3, len(PATS) + 2):
            recs, found = sb.lookup_records(options(THR, order), k)
            check_table(recs, found, ref, docs, order, k)
    base, base_found = sb.lookup_records(options(THR, Order.Default), 3)
    for sides in MASKS:  # the call applies WHOLE whatever the batch carries, and leaves the batch as it is
        recs, found = sb.require_anchors(sides).lookup_records(options(THR, Order.Default), 3)
        assert recs.tobytes() == base.tobytes() and list(found) == list(base_found)
        check_records(sb, ref, docs, THR, Sides(sides), TWO[:1])
    sb.require_anchors(0)
    # the table left in HBM
    k = 3
    buf = torch.full((len(docs) * k * _native.REC_BYTES + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    dev, found = sb.lookup_records(options(THR, Order.Default), k, out=buf)
    assert dev.numel() == len(docs) * k * _native.REC_BYTES and list(found) == list(base_found)
    assert dev.cpu().numpy().tobytes() == base.tobytes()
    assert set(buf[dev.numel():].cpu().tolist()) == {0xAB}
    small = torch.full(((len(docs) * k - 1) * _native.REC_BYTES,), 0xAB, dtype=torch.uint8, device="cuda")
    with pytest.raises(DeviceError) as ei:
        sb.lookup_records(options(THR, Order.Default), k, out=small)
    assert ei.value.code == _native.FAC_E_OUTPUT_CAPACITY and ei.value.needed == len(docs) * k
    assert set(small.cpu().tolist()) == {0xAB}  # nothing written
    with pytest.raises(DeviceError) as ei:
        sb.lookup_records(options(THR), 0)
    assert ei.value.code == _native.FAC_E_INVALID
    # the window count: one per non-empty document
    st = _native.fac_stats()
    sb.lookup_records(options(THR), 1, stats=st)
    assert int(st.windows) == sum(1 for d in docs if d)
    # an empty batch and a batch of empty documents
    recs, found = staged(eng, ["", ""]).lookup_records(options(THR), 2)
    assert recs.shape == (2, 2) and recs.tobytes() == FILLER * 4 and list(found) == [0, 0]


def test_lookup_conveniences():
    names = ["Alice Smith", "Bob Jones", "Carol White", "Dave Brown", "Eve Black"]
    canon_names = ["SMITH, A.", "JONES, B.", None, Wrap("<", ">"), "BLACK, E."]
    b = B().fuzzy(L().edits(2)).case_insensitive(True)
    eng, ref = b.build(names), ARef(b, names)
    texts = ["alice smith", "Bob Jnes", "Carol Whyte", "dave brown", "Eve", "Eve Black and Bob Jones", "", "Eve Blackk"]
    opts = options(0.7, Order.Default)
    got = eng.lookup_batch(texts, opts, k=2)
    for text, ms in zip(texts, got):
        want = ref.rows(text, options(0.7, Order.Default, Overlap.Keep), Sides(3))[:2]
        assert [(m.start, m.end, m.pattern_index, m.sim_bits(), m.insertions, m.deletions, m.substitutions, m.swaps, m.edits)
                for m in ms] == want, text
        assert all(m.text == text for m in ms)
    assert [len(ms) for ms in got] == [1, 1, 1, 1, 0, 0, 0, 1]
    rep = FuzzyReplacer(eng, canon_names)
    assert rep.lookup_batch(texts, opts) == ["SMITH, A.", "JONES, B.", "Carol Whyte", "<dave brown>", None, None, None,
                                             "BLACK, E."]
    # the same answers through engine.search and the batch conveniences with anchors=
    for text in texts:
        ms = eng.search(text, opts, anchors=Anchor.WHOLE)
        assert [m.key() for m in ms] == [m.key() for m in ref.matches(text, opts, Sides(3))]
    seg = options(0.7, Order.Default, Overlap.NonOverlapping)
    ms = [ref.matches(t, seg, Sides(3)) for t in texts]
    assert eng.matched_strings_batch(texts, seg, anchors=Anchor.WHOLE) == [m.matched_strings() for m in ms]
    assert rep.replace_batch(texts, seg, anchors=Anchor.WHOLE) == [m.replace(rep._callback) for m in ms]
    assert eng.strip_suffix_batch(texts, seg, anchors=Anchor.END) == [ref.matches(t, seg, Sides(2)).strip_suffix() for t in texts]
    assert eng.split_batch(texts, seg, anchors=Anchor.START) == [list(ref.matches(t, seg, Sides(1)).split()) for t in texts]
    pre = eng.with_prefilter()
    pms = [ref.matches(t, seg, Sides(3), True) for t in texts]
    assert [[m.key() for m in g] for g in pre.search_batch(texts, seg, anchors=Anchor.WHOLE)] == [[m.key() for m in p] for p in pms]
    assert pre.segment_text_batch(texts, seg, anchors=Anchor.WHOLE) == [m.segment_text() for m in pms]


if __name__ == "__main__":
    child_main()
