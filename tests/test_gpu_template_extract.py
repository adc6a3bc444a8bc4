"""Template replacements (fac_replacements_create_templates) and fac_extract_batch on the device.

Replace. Per document the batch's output == engine.replace(doc, opts, callback) with
callback(m) = None (keep) | the entry | prefix + m.text + suffix (a `Wrap`): the existing host splice
(matches.rs:170-187) over the existing device search. engine.replace is
`engine._segmented(doc, opts).replace(callback)`; the sweeps compute `_segmented` once per document
and share it among their tables. The oracle's records go through the same plain-Python loop
(OracleEngine.replace) for every document whose oracle-kept records have pairwise distinct starts;
the others are the reference's unspecified tie (sort_unstable_by_key, matches.rs:111), as in
test_gpu_replace_batch.

Extract. Every document of every batch, three expected values:
  E0  the records are StagedBatch.search_records' for the same batch and options, byte for byte (for
      Unsorted+Keep as multisets of (record bytes, item)), the two CSR indexes agree, and item i is
      the string of record i.
  E1  engine.search(doc, opts) per document: the exact sequence of (record, item) for every
      order x overlap pair except Unsorted+Keep, which compares multisets. Unsorted with an overlap
      mode walks a document's records in (start, end, pattern_index) order in a batch (fac.h; the
      crate walks its hash map's order, the single search its emission order), so that pair's
      expected value is the engine's own apply over search_raw's records put in that order -- the
      adaptation test_gpu_batch.oracle_doc makes.
  E2  the oracle (test_gpu_batch.oracle_doc): exact where its kept records have distinct starts or
      nothing was resolved, canonical order of equal starts otherwise (test_gpu_batch.canon).
"""
import ctypes

import pytest

from fuzzy_aho_corasick import (DeviceError, FuzzyAhoCorasickBuilder as B, FuzzyLimits as L, FuzzyMatches, Order, Overlap,
                                ReplacementTable, SearchOptions as O, StagedBatch, UnsupportedConfiguration, Wrap,
                                _native, batch_offsets, template_table)
from oracle_harness import OracleEngine
from test_gpu_batch import Rng, canon, oracle_doc, sim_bits
from test_gpu_replace_batch import normalised, options

pytestmark = pytest.mark.gpu

TILE = _native.REPLACE_TILE
assert _native.EXTRACT_TILE == TILE == 4096
COMBOS = [(o, v) for o in Order for v in Overlap]


def raw(x):
    return x if isinstance(x, bytes) else x.encode("utf-8")


def callback(reps):
    """The crate's callback for a table: None, the entry, or format!("{pre}{}{suf}", m.text)."""
    def cb(m):
        r = reps[m.pattern_index]
        if isinstance(r, Wrap):
            return raw(r.prefix).decode("utf-8") + m.text + raw(r.suffix).decode("utf-8")
        return None if r is None else raw(r).decode("utf-8")
    return cb


def staged(eng, docs):
    return StagedBatch(eng, *batch_offsets([raw(d) for d in docs]))


def oracle_tie(orc, doc, opts):
    starts = [m.start for m in orc._segmented(doc, opts)]
    return len(set(starts)) != len(starts)


def check_replace(eng, docs, reps, opts, orc=None, sb=None, table=None, segmented=None, prefilter=False):
    """replace_bytes of the batch == engine.replace per document (`segmented`: that call's matches,
    computed once), == the oracle's where no tie. Returns the per-document output bytes."""
    sb = sb or staged(eng, docs)
    table = table or ReplacementTable(eng, reps)
    out, off = sb.replace_bytes(table, opts, prefilter=prefilter)
    assert isinstance(out, bytes) and len(off) == len(docs) + 1 and off[0] == 0 and int(off[-1]) == len(out)
    got = [out[int(off[d]):int(off[d + 1])] for d in range(len(docs))]
    cb = callback(reps)
    applied = 0
    for d, doc in enumerate(docs):
        ms = segmented[d] if segmented is not None else eng._segmented(doc, opts)
        assert got[d] == ms.replace(cb).encode("utf-8"), (d, doc, reps)
        last = 0
        for m in ms:  # *n_replaced: the records the guard lets through
            if m.start >= last:
                applied, last = applied + 1, m.end
    assert sb.replaced == applied
    if orc is not None:
        for d, doc in enumerate(docs):
            if not oracle_tie(orc, doc, opts):
                assert got[d] == orc.replace(doc, opts, cb).encode("utf-8"), (d, doc, reps)
    return got


def rows_of(recs):
    return [(int(r["start"]), int(r["end"]), int(r["pattern_index"]), sim_bits(float(r["similarity"])),
             int(r["insertions"]), int(r["deletions"]), int(r["substitutions"]), int(r["swaps"]), int(r["edits"]))
            for r in recs]


def match_rows(ms):
    return [(m.start, m.end, m.pattern_index, m.sim_bits(), m.insertions, m.deletions, m.substitutions, m.swaps, m.edits)
            for m in ms]


def item_of(doc: bytes, row, reps):
    """The item of a record: its matched text, or what its table entry makes of it."""
    text = doc[row[0]:row[1]]
    r = None if reps is None else reps[row[2]]
    if isinstance(r, Wrap):
        return raw(r.prefix) + text + raw(r.suffix)
    return text if r is None else raw(r)


def engine_doc(eng, doc, opts):
    """E1's records for one document."""
    if opts.order_ == Order.Unsorted and opts.overlap_ != Overlap.Keep:
        ms = eng.search_raw(doc, opts.threshold_)
        ordered = FuzzyMatches(doc, sorted(ms, key=lambda m: (m.start, m.end, m.pattern_index)), doc.encode("utf-8"))
        return match_rows(eng.apply_on_device(ordered, opts.order_, opts.overlap_))
    return match_rows(eng.search(doc, opts))


def check_extract(eng, docs, opts, reps=None, orc=None, sb=None, table=None, prefilter=False, references=True):
    """E0 always; E1 and E2 (with `orc`) unless `references` is off (pre-filtered calls, whose records
    E0 pins to search_records(prefilter=True)). Returns per document the list of (row, item)."""
    enc = [raw(d) for d in docs]
    sb = sb or staged(eng, docs)
    if table is None and reps is not None:
        table = ReplacementTable(eng, reps)
    recs, doc_off, text, item_off = sb.extract(table, opts, prefilter=prefilter)
    n = len(recs)
    assert isinstance(text, bytes) and len(item_off) == n + 1 and item_off[0] == 0 and int(item_off[-1]) == len(text)
    assert all(item_off[i] <= item_off[i + 1] for i in range(n))
    assert len(doc_off) == len(docs) + 1 and doc_off[0] == 0 and int(doc_off[-1]) == n
    srecs, soff = sb.search_records(opts, prefilter=prefilter)
    assert list(doc_off) == list(soff)
    unordered = opts.order_ == Order.Unsorted and opts.overlap_ == Overlap.Keep
    if not unordered:
        assert recs.tobytes() == srecs.tobytes()
    rows = rows_of(recs)
    got = []
    for d, doc in enumerate(enc):
        lo, hi = int(doc_off[d]), int(doc_off[d + 1])
        pairs = [(rows[i], text[int(item_off[i]):int(item_off[i + 1])]) for i in range(lo, hi)]
        for row, item in pairs:  # the pairing of record and item
            assert item == item_of(doc, row, reps), (d, doc, row)
        if unordered:
            assert sorted(r.tobytes() for r in recs[lo:hi]) == sorted(r.tobytes() for r in srecs[lo:hi])
        got.append(pairs)
        if not references:
            continue
        sdoc = docs[d] if isinstance(docs[d], str) else doc.decode("utf-8")
        want = [(r, item_of(doc, r, reps)) for r in engine_doc(eng, sdoc, opts)]
        assert (sorted(pairs) == sorted(want)) if unordered else (pairs == want), (opts.order_, opts.overlap_, d, doc)
        if orc is not None:
            orows = oracle_doc(orc, sdoc, opts.threshold_, opts.order_, opts.overlap_)
            starts = [r[0] for r in orows]
            if not unordered and (opts.overlap_ == Overlap.Keep or len(set(starts)) == len(starts)):
                assert [p[0] for p in pairs] == orows, (opts.order_, opts.overlap_, d, doc)
            assert canon([p[0] for p in pairs], opts.order_, opts.overlap_) == canon(orows, opts.order_, opts.overlap_)
    return got


# ---------------------------------------------------------------- 1. table kinds

def test_table_kinds_in_one_table():
    """Plain, keep and template entries in one table; k = 0, k = len, and the empty entry with k = 0,
    which is "keep" byte for byte; the crate's documented callback."""
    b = B().fuzzy(L().edits(1)).case_insensitive(True)
    pats = ["ipsum", "lorem", "hello", "world", "dolor", "amet"]
    eng, orc = b.build(pats), OracleEngine(b, pats)
    docs = ["ipsum and l0rem", "", "helo wrld dolor amet", "no match", "lorem", "xamet", "hello hello world"]
    opts = O().threshold(0.5).sorted().non_overlapping()  # matches.rs:443
    reps = [None, Wrap("**", "**"), "HELLO", Wrap("", "!"), Wrap("<ent id=\"4\">", ""), Wrap("", "")]
    assert template_table(reps)[3] == [_native.FAC_NO_INSERT, 2, _native.FAC_NO_INSERT, 0, 12, 0]
    got = check_replace(eng, docs, reps, opts, orc)
    assert got[0] == b"ipsum and **l0rem**"  # matches.rs:445-446
    assert got[2].startswith(b"HELLO") and b"<ent id=\"4\">dolor" in got[2] and got[2].endswith(b"amet")
    items = check_extract(eng, docs, opts, reps, orc)
    assert [i for _, i in items[0]] == [b"ipsum", b"**l0rem**"]
    assert b"HELLO" in [i for _, i in items[2]] and b"<ent id=\"4\">dolor" in [i for _, i in items[2]]
    # an empty entry with the slot at 0 == keep, and a table of such entries gives the input back
    same = [Wrap("", "")] * len(pats)
    keep = [None] * len(pats)
    assert check_replace(eng, docs, same, opts, orc) == check_replace(eng, docs, keep, opts, orc) == [raw(d) for d in docs]
    assert check_extract(eng, docs, opts, same) == check_extract(eng, docs, opts, keep) == check_extract(eng, docs, opts)
    # without a Wrap the table is fac_replacements_create's
    plain = ["A", None, "", "«é»", None, "x" * 20]
    check_replace(eng, docs, plain, opts, orc)
    check_extract(eng, docs, opts, plain, orc)


def test_non_ascii_halves_and_matches():
    b = B().fuzzy(L().edits(1)).case_insensitive(True)
    pats = ["wörld", "héllo", "日本語"]
    eng, orc = b.build(pats), OracleEngine(b, pats)
    docs = ["zz wörld zz wôrld", "héllo wörld", "", "日本語 と 日本话", "é", "hello 😀 wörld😀"]
    reps = [Wrap("«é", "😀»"), Wrap(b"\xe2\x86\x92", ""), Wrap("", "。")]
    for opts in (O().threshold(0.7), options(0.7, Order.Greedy, Overlap.NonOverlappingUnique)):
        got = check_replace(eng, docs, reps, opts, orc)
        assert got[1] == "→héllo «éwörld😀»".encode() and b"\xe3\x80\x82" in got[3]
        for g in got:
            g.decode("utf-8")
    for order, overlap in COMBOS:
        check_extract(eng, docs, options(0.7, order, overlap), reps, orc)
        check_extract(eng, docs, options(0.7, order, overlap), None, orc)


# ---------------------------------------------------------------- 2. errors

def create_templates(eng, entries, insert_at, keep=None):
    data, off = batch_offsets([raw(e) for e in entries])
    h = ctypes.c_void_p()
    rc = _native.lib.fac_replacements_create_templates(
        eng._h, data, (ctypes.c_uint64 * len(off))(*off), keep,
        (ctypes.c_uint64 * max(1, len(insert_at)))(*insert_at) if insert_at is not None else None, len(entries),
        ctypes.byref(h))
    if h.value:
        _native.lib.fac_replacements_free(h)
    return rc


def test_template_errors():
    NO = _native.FAC_NO_INSERT
    eng = B().build(["hello", "world"])
    assert create_templates(eng, ["aé", "b"], [1, 1]) == _native.FAC_OK  # before é, at the end
    assert create_templates(eng, ["aé", "b"], [3, 0]) == _native.FAC_OK
    assert create_templates(eng, ["aé", "b"], None) == _native.FAC_OK    # insert_at NULL: fac_replacements_create
    assert create_templates(eng, ["aé", "b"], [2, NO]) == _native.FAC_E_INVALID   # inside é
    assert create_templates(eng, ["😀", "b"], [NO, 0]) == _native.FAC_OK
    for k in (1, 2, 3):
        assert create_templates(eng, ["😀", "b"], [k, 0]) == _native.FAC_E_INVALID
    assert create_templates(eng, ["aé", "b"], [4, NO]) == _native.FAC_E_INVALID   # k > len
    assert create_templates(eng, ["", "b"], [1, NO]) == _native.FAC_E_INVALID
    assert create_templates(eng, ["aé", "b"], [NO, 2]) == _native.FAC_E_INVALID
    assert create_templates(eng, ["aé", "b"], [2, 5], keep=b"\1\1") == _native.FAC_OK  # keep wins over insert_at
    assert create_templates(eng, ["a"], [0]) == _native.FAC_E_INVALID              # the wrong pattern count
    assert create_templates(eng, ["a", "b", "c"], [0, 0, 0]) == _native.FAC_E_INVALID
    assert create_templates(eng, [b"\xc3", "b"], [0, 0]) == _native.FAC_E_INVALID  # invalid UTF-8, as before
    with pytest.raises(DeviceError) as ei:  # through Python: the halves are not valid on their own
        ReplacementTable(eng, [Wrap(b"\xc3", b"\xa9"), "b"])
    assert ei.value.code == _native.FAC_E_INVALID
    with pytest.raises(DeviceError) as ei:
        ReplacementTable(eng, [Wrap("a", "b")])
    assert ei.value.code == _native.FAC_E_INVALID
    # extract: a table of another engine's pattern count; records_out without text_out
    sb = staged(eng, ["hello"])
    with pytest.raises(DeviceError) as ei:
        sb.extract(ReplacementTable(B().build(["hello"]), [Wrap("a", "b")]), O().threshold(0.9))
    assert ei.value.code == _native.FAC_E_INVALID
    import torch
    a = _native.fac_extract_args()
    a.threshold, a.device_records, a.device_record_cap = 0.9, torch.empty(64, dtype=torch.uint8, device="cuda").data_ptr(), 2
    n, nb = ctypes.c_uint64(), ctypes.c_uint64()
    rc = _native.lib.fac_extract_batch(eng._h, sb._h, None, ctypes.byref(a), None, ctypes.byref(n), None, None,
                                       ctypes.byref(nb), None, None)
    assert rc == _native.FAC_E_INVALID
    bm = B().fuzzy(L().edits(1)).mapping("ss", "ß")  # mappings with non-ASCII documents: as fac_search_batch
    em = bm.build(["strasse"])
    mopts = O().threshold(0.9).sorted().non_overlapping()
    assert em.extract_batch(["strasse", "x"], mopts, [Wrap("[", "]")]) == [["[strasse]"], []]
    with pytest.raises(UnsupportedConfiguration):
        em.matched_strings_batch(["strasse", "straße"], mopts)


# ---------------------------------------------------------------- 3. run boundaries against lanes

@pytest.mark.parametrize("third", [0, 1, 2])
def test_run_boundaries_against_lanes(third):
    """One pattern, documents "x" * g + match + "y", g, |pre| and |suf| over 0..17: every run boundary
    of the splice (gap | pre | text | suf | tail) and of the extraction (pre | text | suf) lands on
    every residue mod 16, and runs of length 0 occur in every position."""
    eng = B().build(["hello"])
    opts = O().threshold(0.9)
    docs = ["x" * g + "hello" + "y" for g in range(18)] + ["hello", "yhello"]
    sb = staged(eng, docs)
    segmented = [eng._segmented(d, opts) for d in docs]
    assert all(len(ms) == 1 for ms in segmented)
    kinds = {k: set() for k in ("pre", "text", "suf", "tail", "ipre", "itext", "isuf")}
    for p in range(6 * third, 6 * third + 6):
        for s in range(18):
            reps = [Wrap("<" * p, ">" * s)]
            table = ReplacementTable(eng, reps)
            got = check_replace(eng, docs, reps, opts, sb=sb, table=table, segmented=segmented)
            items = check_extract(eng, docs, opts, reps, sb=sb, table=table, references=False)
            o = i = 0
            for d, (doc, g) in enumerate(zip(docs, got)):
                lead = doc.index("hello")
                assert g == raw(doc[:lead] + "<" * p + "hello" + ">" * s + doc[lead + 5:])
                assert [it for _, it in items[d]] == [raw("<" * p + "hello" + ">" * s)]
                for kind, at in (("pre", o + lead), ("text", o + lead + p), ("suf", o + lead + p + 5),
                                 ("tail", o + lead + p + 5 + s), ("ipre", i), ("itext", i + p), ("isuf", i + p + 5)):
                    kinds[kind].add(at % 16)
                o += len(g)
                i += p + 5 + s
    for kind, seen in kinds.items():
        assert seen == set(range(16)), kind


def test_guard_skips_a_record_of_a_template():
    """Pattern "a" with one edit at threshold 0 keeps a span and the empty span at its start
    (matches.rs:93-99): the guard's skipped record contributes nothing, template or not, at every
    lane offset; the extraction still gives the skipped record its item."""
    b = B().fuzzy(L().edits(1))
    eng, orc = b.build(["a"]), OracleEngine(b, ["a"])
    docs = ["a", "aa", "", "ba"] + ["b" * g + "a" for g in range(18)]
    opts = O().threshold(0.0)
    sb = staged(eng, docs)
    recs, doc_off = sb.search_records(normalised(opts))
    per_doc = [rows_of(recs[int(doc_off[d]):int(doc_off[d + 1])]) for d in range(len(docs))]
    assert any(r[0] == r[1] for rows in per_doc for r in rows)                      # empty spans are kept
    assert any(len({r[0] for r in rows}) != len(rows) for rows in per_doc)          # two records of one start
    segmented = [eng._segmented(d, opts) for d in docs]
    for p, s in [(0, 0), (1, 0), (0, 1), (2, 3), (7, 9), (16, 0), (0, 16), (17, 17)]:
        reps = [Wrap("<" * p, ">" * s)]
        table = ReplacementTable(eng, reps)
        check_replace(eng, docs, reps, opts, orc, sb=sb, table=table, segmented=segmented)
        check_extract(eng, docs, normalised(opts), reps, orc, sb=sb, table=table)
    check_extract(eng, docs, options(0.0, Order.Unsorted, Overlap.Keep), [Wrap("<", ">")], orc, sb=sb)


# ---------------------------------------------------------------- 4. run boundaries against tiles

def test_a_run_longer_than_a_tile():
    eng = B().build(["hello", "world"])
    opts = O().threshold(0.9)
    pre = "".join(chr(0x41 + i % 26) for i in range(5000))
    docs = ["hello", "zz hello world", "", "world" * 3, "q" * 40]
    for reps in ([Wrap(pre, "]"), None], [Wrap("[", pre), Wrap(pre, pre)], [pre, Wrap("", "")]):
        got = check_replace(eng, docs, reps, opts)
        assert len(got[1]) > 5000
        items = check_extract(eng, docs, opts, reps)
        assert max(len(i) for _, i in items[1]) >= 5000
    # a matched text that spans several lanes, kept and wrapped, at every lane offset
    long_pat = "abcdefghijklmnopqrstuvwxyz0123"
    eng2 = B().build([long_pat])
    docs2 = ["x" * g + long_pat + "y" for g in range(17)]
    for reps in ([None], [Wrap("<", ">")], [Wrap("", "")]):
        got = check_replace(eng2, docs2, reps, opts)
        assert all(long_pat.encode() in g for g in got)
        check_extract(eng2, docs2, opts, reps)
    check_extract(eng2, docs2, opts)


@pytest.mark.parametrize("total", [TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, 15, 16, 17, 16 * 7 - 1, 16 * 7 + 1])
def test_totals_at_tile_and_chunk_edges(total):
    """Outputs of exactly 4096, 4097, 8192 and n * 16 +- 1 bytes: the last tile and the last lane are
    full, one byte short, or one byte over."""
    eng = B().build(["hello", "hellp"])
    opts = O().threshold(0.9)
    # one piece of `total` bytes: the document "hello" inside a template
    p = (total - 5) // 2
    reps = [Wrap("<" * p, ">" * (total - 5 - p)), None]
    assert len(check_replace(eng, ["hello"], reps, opts)[0]) == total
    items = check_extract(eng, ["", "hello"], opts, reps)
    assert [len(i) for pairs in items for _, i in pairs] == [total]
    # `total` bytes in many 5-byte items of matched text and a last item that carries the remainder
    n5, rest = divmod(total - 5, 5)
    docs = ["hello" * n5, "", "hellp"]
    reps = [None, Wrap("", "!" * rest)]
    items = check_extract(eng, docs, opts, reps)
    assert sum(len(i) for pairs in items for _, i in pairs) == total and len(items[0]) == n5
    assert sum(len(g) for g in check_replace(eng, docs, reps, opts)) == total


def test_many_one_byte_items():
    """Items of 0-2 bytes over many tiny and empty documents: one lane crosses 16 items and several
    documents; with an empty entry every item is empty."""
    b = B()
    eng, orc = b.build(["a", "b"]), OracleEngine(b, ["a", "b"])
    rng = Rng(0x17e45)
    docs = ["".join("abc"[rng.next() % 3] for _ in range(rng.next() % 5)) for _ in range(400)] + ["", "", "ab" * 40]
    assert "" in docs and max(len(d) for d in docs[:400]) == 4
    opts = O().threshold(0.9)
    sb = staged(eng, docs)
    got = check_extract(eng, docs, opts, None, orc, sb=sb)
    assert sum(len(p) for p in got) > 400 and all(len(i) == 1 for p in got for _, i in p)
    for reps in ([Wrap("", ""), ""], ["", Wrap("", "Z")], [Wrap("é", ""), None]):
        check_extract(eng, docs, opts, reps, sb=sb, references=False)
        check_replace(eng, docs, reps, opts, orc, sb=sb)


# ---------------------------------------------------------------- 5. degenerate batches

def test_degenerate_batches():
    b = B().fuzzy(L().edits(1))
    eng, orc = b.build(["hello", "world"]), OracleEngine(b, ["hello", "world"])
    opts = O().threshold(0.8)
    reps = [Wrap("<", ">"), None]
    for docs in ([], ["zzzz", "", "qqqq qqqq"], [""], ["", "", ""]):  # zero documents; no matches
        assert check_extract(eng, docs, opts, None, orc) == [[] for _ in docs]
        assert check_extract(eng, docs, opts, reps, orc) == [[] for _ in docs]
        assert check_replace(eng, docs, reps, opts, orc) == [raw(d) for d in docs]
        recs, doc_off, text, item_off = staged(eng, docs).extract(None, opts)
        assert len(recs) == 0 and text == b"" and list(item_off) == [0] and list(doc_off) == [0] * (len(docs) + 1)
    # every item empty: the total is 0 with records present
    docs = ["hello world", "", "helo", "world world"]
    got = check_extract(eng, docs, opts, ["", ""], orc)
    assert sum(len(p) for p in got) >= 6 and all(i == b"" for p in got for _, i in p)
    assert check_replace(eng, ["hello", "", "world"], [Wrap("", ""), ""], opts, orc) == [b"hello", b"", b""]
    assert eng.matched_strings_batch([], opts) == [] and eng.extract_batch([], opts, reps) == []


# ---------------------------------------------------------------- 6. orders, overlaps, Overlap::Keep

def test_every_order_and_overlap():
    """Every order x overlap pair; under Overlap::Keep the items overlap in the source and their total
    exceeds the batch's byte count."""
    b = B().fuzzy(L().edits(1))
    pats = ["hello", "hell", "ello", "lo w", "world", "hello world", "o"]
    eng, orc = b.build(pats), OracleEngine(b, pats)
    docs = ["hello world", "helo wrld hello", "", "lo wo", "hello world hello world", "é hello"]
    reps = [Wrap("[", "]"), None, "E", Wrap("", "~"), Wrap("<w>", "</w>"), "", Wrap("", "")]
    sb = staged(eng, docs)
    table = ReplacementTable(eng, reps)
    sizes = {}
    for order, overlap in COMBOS:
        opts = options(0.6, order, overlap)
        got = check_extract(eng, docs, opts, None, orc, sb=sb)
        check_extract(eng, docs, opts, reps, orc, sb=sb, table=table)
        sizes[order, overlap] = sum(len(i) for p in got for _, i in p)
        if overlap == Overlap.Keep:
            spans = sorted((r[0], r[1]) for r, _ in got[0])
            assert any(a[1] > c[0] for a, c in zip(spans, spans[1:]))  # items overlap in the source
            assert sizes[order, overlap] > sum(len(raw(d)) for d in docs)
        else:
            assert sizes[order, overlap] <= sum(len(raw(d)) for d in docs)
        check_replace(eng, docs, reps, opts, orc, sb=sb, table=table)


# ---------------------------------------------------------------- 7. device output

def test_device_output():
    import torch
    b = B().fuzzy(L().edits(1))
    eng = b.build(["hello", "world"])
    reps = [Wrap("«", "»"), ""]
    docs = ["hello world", "", "helo wrld hello", "wörld", "x" * 50, "hello" * 9]
    opts = O().threshold(0.6).sorted()
    sb = staged(eng, docs)
    table = ReplacementTable(eng, reps)
    for tab in (None, table):
        recs, doc_off, text, item_off = sb.extract(tab, opts)
        n, nb = len(recs), len(text)
        assert n > 8 and nb > 16
        for short_recs, short_text in ((1, 0), (0, 1), (1, 1)):  # either buffer too small: nothing written to either
            r = torch.full(((n - short_recs) * 32,), 0xAB, dtype=torch.uint8, device="cuda")
            t = torch.full((nb - short_text,), 0xAB, dtype=torch.uint8, device="cuda")
            io = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
            with pytest.raises(DeviceError) as ei:
                sb.extract(tab, opts, records_out=r, text_out=t, item_offsets_out=io)
            assert ei.value.code == _native.FAC_E_OUTPUT_CAPACITY
            assert (ei.value.needed, ei.value.needed_text) == (n, nb)
            assert bool((r == 0xAB).all()) and bool((t == 0xAB).all()) and bool((io == -1).all())
        for pad in (0, 1):  # a 16-byte aligned text buffer, and one that is not (the byte-store path)
            r = torch.full((n * 32 + 32,), 0xCD, dtype=torch.uint8, device="cuda")
            buf = torch.full((nb + 32,), 0xCD, dtype=torch.uint8, device="cuda")
            io = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
            do = torch.full((len(docs) + 1,), -1, dtype=torch.int64, device="cuda")
            g_recs, g_doc, g_text, g_item = sb.extract(tab, opts, records_out=r[:n * 32], text_out=buf[pad:pad + nb],
                                                       doc_offsets_out=do, item_offsets_out=io)
            assert g_recs.cpu().numpy().tobytes() == recs.tobytes() and g_text.cpu().numpy().tobytes() == text
            assert list(g_doc) == list(doc_off) and g_item.cpu().tolist() == [int(x) for x in item_off]
            assert io.cpu().tolist() == [int(x) for x in item_off] and do.cpu().tolist() == [int(x) for x in doc_off]
            assert bool((buf[:pad] == 0xCD).all()) and bool((buf[pad + nb:] == 0xCD).all())  # nothing beside it
            assert bool((r[n * 32:] == 0xCD).all())
    # the template splice into a buffer that is not 16-byte aligned
    host, host_off = sb.replace_bytes(table, opts)
    for pad in (0, 1):
        buf = torch.full((len(host) + 32,), 0xCD, dtype=torch.uint8, device="cuda")
        got, got_off = sb.replace_bytes(table, opts, out=buf[pad:pad + len(host)])
        assert got.cpu().numpy().tobytes() == host and list(got_off) == list(host_off)
        assert bool((buf[:pad] == 0xCD).all()) and bool((buf[pad + len(host):] == 0xCD).all())
    with pytest.raises(ValueError):
        sb.extract(None, opts, records_out=torch.empty(64, dtype=torch.uint8, device="cuda"))


# ---------------------------------------------------------------- 8. pre-filtered forms

def test_prefiltered_forms():
    import torch
    b = B().fuzzy(L().edits(1)).case_insensitive(True)
    pats = ["hello", "world", "cell", "abcdefg"]
    eng = b.build(pats)
    assert eng.with_prefilter().is_active()
    reps = [Wrap("<b>", "</b>"), None, "CELL", Wrap("", "#")]
    table = ReplacementTable(eng, reps)
    docs = ["hello world", "", "zq0 helo zq0 wrld hello", "cell abcdefg", "zz", "q" * 300 + "HELLO"]
    sb = staged(eng, docs)
    for order, overlap in ((Order.Default, Overlap.NonOverlapping), (Order.Unsorted, Overlap.Keep), (Order.Greedy, Overlap.Keep)):
        opts = options(0.75, order, overlap)
        for tab, rr in ((None, None), (table, reps)):
            pf = check_extract(eng, docs, opts, rr, sb=sb, table=tab, prefilter=True, references=False)
            plain = check_extract(eng, docs, opts, rr, sb=sb, table=tab)
            assert [sorted(p) for p in pf] == [sorted(p) for p in plain] and sum(len(p) for p in pf) >= 6
            if order != Order.Unsorted:
                assert pf == plain
    opts = options(0.75)
    assert sb.replace_bytes(table, opts, prefilter=True)[0] == sb.replace_bytes(table, opts)[0]
    check_replace(eng, docs, reps, opts, sb=sb, table=table)
    # a fallback engine (a mapping: no filter): the pre-filtered call is the plain call, for any batch
    bm = B().fuzzy(L().edits(1)).mapping("ss", "ß")
    em = bm.build(["strasse", "hello"])
    assert not em.with_prefilter().is_active()
    fdocs = ["strasse hello", "", "no match here", "hello strase"]
    fsb = staged(em, fdocs)
    ftab = ReplacementTable(em, [Wrap("[", "]"), None])
    for opts in (options(0.7), options(0.7, Order.Unsorted, Overlap.Keep)):
        a = check_extract(em, fdocs, opts, ftab.replacements, sb=fsb, table=ftab, prefilter=True, references=False)
        p = check_extract(em, fdocs, opts, ftab.replacements, sb=fsb, table=ftab)
        assert [sorted(x) for x in a] == [sorted(x) for x in p] and sum(len(x) for x in a) >= 3
    # a mixed batch is refused as by the other pre-filtered calls, with nothing written
    mixed = staged(eng, ["hello world", "wörld hello", "cell"])
    r = torch.full((64 * 32,), 0xAB, dtype=torch.uint8, device="cuda")
    t = torch.full((256,), 0xAB, dtype=torch.uint8, device="cuda")
    with pytest.raises(UnsupportedConfiguration):
        mixed.extract(table, options(0.75), records_out=r, text_out=t, prefilter=True)
    with pytest.raises(UnsupportedConfiguration):
        mixed.extract(None, options(0.75), prefilter=True)
    assert bool((r == 0xAB).all()) and bool((t == 0xAB).all())
    assert len(mixed.extract(table, options(0.75))[0]) > 0  # the plain call still takes the batch


# ---------------------------------------------------------------- 9. Python conveniences

def test_python_conveniences():
    import io
    b = B().fuzzy(L().edits(1)).case_insensitive(True)
    pats = ["hello", "wörld", "cell"]
    eng = b.build(pats)
    pf = eng.with_prefilter()
    assert pf.is_active()
    texts = ["helllo wörld", "HELLO cell", "", "wôrld", "say helo to the cell", "é", "zz"]  # mixed is_ascii
    reps = [Wrap("<b>", "</b>"), None, "CELL"]
    for opts in (O().threshold(0.7).sorted().non_overlapping(), O().threshold(0.7).sorted(), O().threshold(0.7)):
        key = (lambda x: x) if opts.order_ != Order.Unsorted else sorted
        want = [eng.search(t, opts).matched_strings() for t in texts]
        assert [key(g) for g in eng.matched_strings_batch(texts, opts)] == [key(w) for w in want]
        assert sum(len(w) for w in want) > 5
        pwant = [pf.search(t, opts).matched_strings() for t in texts]
        assert [key(g) for g in pf.matched_strings_batch(texts, opts)] == [key(w) for w in pwant]
        cb = callback(reps)
        ewant = [[m.text if cb(m) is None else cb(m) for m in eng.search(t, opts)] for t in texts]
        assert [key(g) for g in eng.extract_batch(texts, opts, reps)] == [key(w) for w in ewant]
        assert [key(g) for g in eng.extract_batch(texts, opts, ReplacementTable(eng, reps))] == [key(w) for w in ewant]
        pewant = [[m.text if cb(m) is None else cb(m) for m in pf.search(t, opts)] for t in texts]
        assert [key(g) for g in pf.extract_batch(texts, opts, reps)] == [key(w) for w in pewant]
    opts = O().threshold(0.7).sorted().non_overlapping()
    assert eng.matched_strings_batch(texts[:2], opts) == [["helllo", "wörld"], ["HELLO", "cell"]]  # matches.rs:510
    assert eng.extract_batch(texts[:2], opts, reps) == [["<b>helllo</b>", "wörld"], ["<b>HELLO</b>", "CELL"]]
    # FuzzyReplacer with a Wrap entry: replace, replace_batch and replace_stream agree
    rep = b.build_replacer([("hello", Wrap("**", "**")), ("wörld", "WORLD"), ("cell", Wrap("", "s"))])
    assert rep.replacements[0] == Wrap("**", "**")
    one = [rep.replace(t, opts) for t in texts]
    assert rep.replace_batch(texts, opts) == one
    assert one[0] == "**helllo** WORLD" and one[1] == "**HELLO** cells"
    assert pf.replace_batch(texts, opts, rep.replacements) == [
        eng._search_ranked(t, 0.7, Order.Default, Overlap.NonOverlapping, prefilter=True).replace(rep._callback) for t in texts]
    for t, w in zip(texts, one):
        out = io.BytesIO()
        rep.replace_stream(io.BytesIO(t.encode("utf-8")), out, 0.7)
        assert out.getvalue().decode("utf-8") == w, t
    assert rep.extract_batch(texts[:2], opts) == [["**helllo**", "WORLD"], ["**HELLO**", "cells"]]
