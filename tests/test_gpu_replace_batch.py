"""fac_replace_batch: the fuzzy find-and-replace of a whole batch on the device, per document ==
engine.replace(doc, opts, callback) of the crate (query.rs:46-96, matches.rs:165-188).

Two expected values:
  E1  the loop of matches.rs:170-187 in plain Python over the records StagedBatch.search_records
      returns for the same batch and the normalised options (those records are pinned to the oracle
      by test_gpu_batch). Defined for every document, compared byte for byte, always.
  E2  OracleEngine.replace / OracleReplacer.replace on each document alone, independent of the
      product. Compared on every document whose oracle-kept records have pairwise distinct starts;
      the others are the reference's unspecified tie (sort_unstable_by_key, matches.rs:111) and are
      checked by E1 only. The random test asserts that at most 5 % of the cases are excluded.
"""
import numpy as np
import pytest

from fuzzy_aho_corasick import (DeviceError, FuzzyAhoCorasickBuilder as B, FuzzyLimits as L, Order, Overlap, Pattern,
                                ReplacementTable, SearchOptions as O, StagedBatch, UnsupportedConfiguration, _native,
                                batch_offsets)
from oracle_harness import OracleEngine, OracleReplacer
from test_gpu_batch import ASCII_VOCAB, ASTRAL_VOCAB, SEEDS, UNI_VOCAB, Rng, random_batch, set_knobs  # noqa: F401

pytestmark = pytest.mark.gpu

TILE = _native.REPLACE_TILE
REPS = ["", "X", "«é»", "😀", "0123456789abcdefghij", None]


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


def rep_bytes(r):
    return r if isinstance(r, (bytes, type(None))) else r.encode("utf-8")


def splice(doc: bytes, recs, reps):
    """E1: matches.rs:170-187 over (start, end, pattern) records; returns (bytes, records applied)."""
    out, last, applied = [], 0, 0
    for s, e, p in recs:
        if s >= last:
            out.append(doc[last:s])
            r = rep_bytes(reps[p])
            out.append(doc[s:e] if r is None else r)
            last = e
            applied += 1
    out.append(doc[last:])
    return b"".join(out), applied


def oracle_tie(orc, doc, opts):
    """True if two of the oracle's kept records share a start (E2 is unspecified there)."""
    starts = [m.start for m in orc._segmented(doc, opts)]
    return len(set(starts)) != len(starts)


def check(eng, docs, reps, opts, orc=None, sb=None, table=None):
    """replace_bytes of the batch == E1 for every document, == E2 (with `orc`) where no tie; returns
    (per-document output bytes, documents compared with E2, documents excluded as ties)."""
    enc = [d.encode("utf-8") if isinstance(d, str) else d for d in docs]
    if sb is None:
        sb = StagedBatch(eng, *batch_offsets(enc))
    table = table or ReplacementTable(eng, reps)
    out, off = sb.replace_bytes(table, opts)
    assert isinstance(out, bytes) and len(off) == len(enc) + 1 and off[0] == 0 and int(off[-1]) == len(out)
    got = [out[int(off[d]):int(off[d + 1])] for d in range(len(enc))]
    recs, doc_off = sb.search_records(normalised(opts))
    applied = 0
    for d, doc in enumerate(enc):
        rows = [(int(r["start"]), int(r["end"]), int(r["pattern_index"])) for r in recs[int(doc_off[d]):int(doc_off[d + 1])]]
        want, k = splice(doc, rows, reps)
        applied += k
        assert got[d] == want, (d, doc, rows, reps)
        got[d].decode("utf-8")  # valid UTF-8
    assert sb.replaced == applied
    compared = ties = 0
    if orc is not None:
        for d, doc in enumerate(docs):
            if oracle_tie(orc, doc, opts):
                ties += 1
                continue
            want = orc.replace(doc, opts, lambda m: None if reps[m.pattern_index] is None else reps[m.pattern_index])
            assert got[d] == want.encode("utf-8"), (d, doc, reps)
            compared += 1
    return got, compared, ties


# ---------------------------------------------------------------- 1. the crate's own cases

def test_crate_cases_in_one_batch():
    b = B()
    pats = ["FOO", "BAR", "BAZ"]
    eng, orc = b.build(pats), OracleEngine(b, pats)
    opts = O().threshold(0.8)
    got, compared, _ = check(eng, ["FOO BAR BAZ", "", "BAR", "nothing"], [None, "###", None], opts, orc)  # query.rs:78-84
    assert got == [b"FOO ### BAZ", b"", b"###", b"nothing"] and compared == 4
    assert eng.replace_batch(["FOO BAR BAZ", "BAZ BAR"], opts, [None, "###", None]) == ["FOO ### BAZ", "BAZ ###"]


@pytest.mark.parametrize("builder,pairs,thr,texts,want", [
    (lambda: B().case_insensitive(True),  # tests.rs:436-450
     [("PUBLIC JOINT STOCK COMPANY", "PJSC"), ("PUBLIC JOINT STOCK", "PJSC"), ("LIMITED LIABILITY COMPANY", "LLC"),
      ("LIMITED LIABILITY", "LLC")], 0.8,
     ["PUBLIC JOINT STOCK COMPANY GAZPROM", "limited liability company x", "GAZPROM"], ["PJSC GAZPROM", None, "GAZPROM"]),
    (lambda: B().fuzzy(L().substitutions(1)).case_insensitive(True), [("foo", "bar"), ("baz", "qux")], 0.7,  # tests.rs:513-524
     ["fo0 and BAZ!", "", "BAZ fo0"], ["bar and qux!", "", None]),
    (lambda: B().fuzzy(L().edits(5)).case_insensitive(True), [("CZECHOSLOVAKIA", "SERBIA")], 0.7,  # tests.rs:526-537
     ["CHEKHOSLOVAKIA", "in CHEKHOSLOVAKIA."], ["SERBIA", None]),
])
def test_replacer_cases_as_one_batch(builder, pairs, thr, texts, want):
    rep = builder().build_replacer(pairs)
    orc = OracleReplacer(OracleEngine(builder(), [p for p, _ in pairs]), [r for _, r in pairs])
    opts = O().threshold(thr)
    got = rep.replace_batch(texts, opts)
    assert got == [rep.replace(t, opts) for t in texts]
    assert got == [orc.replace(t, opts) for t in texts]
    assert all(w is None or g == w for g, w in zip(got, want))
    check(rep.engine, texts, rep.replacements, opts)


# ---------------------------------------------------------------- 2. edges of the splice

def test_splice_edges():
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
            "ab",
            "é"]
    opts = O().threshold(0.75)
    for reps in (["", "«é»", "X"],                      # an empty replacement, a multi-byte one
                 ["0123456789" * 3, None, None],        # longer than the document; keep
                 [None, None, None],                    # everything kept: the output is the input
                 ["", "", ""]):
        got, compared, ties = check(eng, docs, reps, opts, orc)
        assert compared + ties == len(docs) and ties == 0
        if reps == [None, None, None]:
            assert got == [d.encode() for d in docs]
    # n_docs == 0, and a batch whose whole output is 0 bytes
    assert check(eng, [], ["", "", ""], opts, orc)[0] == []
    got, _, _ = check(eng, ["hello", "", "ab", "helo"], ["", "", ""], opts, orc)
    assert got == [b"", b"", b"", b""]
    assert eng.replace_batch([], opts, ["", "", ""]) == []


# ---------------------------------------------------------------- 3. guard and ties

def test_guard_and_ties():
    """Pattern "a" with one edit at threshold 0: empty-span records insert at a point, and a span and
    the empty span at its start can both be kept (matches.rs:93-99): the guard drops the second."""
    b = B().fuzzy(L().edits(1))
    eng, orc = b.build(["a"]), OracleEngine(b, ["a"])
    docs = ["a", "aa", "", "ba"]
    opts = O().threshold(0.0)
    sb = StagedBatch(eng, *batch_offsets([d.encode() for d in docs]))
    recs, doc_off = sb.search_records(normalised(opts))
    rows = [[(int(r["start"]), int(r["end"])) for r in recs[int(doc_off[d]):int(doc_off[d + 1])]] for d in range(len(docs))]
    assert any(s == e for r in rows for s, e in r)  # empty spans are kept
    shared = [d for d, r in enumerate(rows) if len({s for s, _ in r}) != len(r)]
    assert shared  # some document keeps two records of one start
    for reps in (["<>"], [""], [None]):
        got, compared, ties = check(eng, docs, reps, opts, orc, sb=sb)
        assert compared >= 1 and compared + ties == len(docs)
    got, _, _ = check(eng, docs, ["<>"], opts, orc, sb=sb)
    assert got[2] == b""  # nothing to match in an empty document


# ---------------------------------------------------------------- 4. alignment sweep

def test_alignment_sweep():
    """Gap / replacement boundaries at every output offset mod 16 and every source offset mod 16:
    prefix documents of 0-17 bytes before a matching document, replacement lengths 0-17."""
    b = B()
    eng = b.build(["hello"])
    opts = O().threshold(0.9)
    out_res, src_res, pairs = set(), set(), set()
    for q in range(18):
        docs = []
        for p in range(18):
            docs += ["z" * p, "ab hello cd hello"]
        reps = ["R" * q]
        got, _, _ = check(eng, docs, reps, opts)
        src = out = 0
        for d, g in zip(docs, got):
            for at in (3, 12):  # the two matches: source start, and where their pieces start in the output
                o = out + (3 if at == 3 else 3 + q + 4)
                for so, oo in ((src + at, o), (src + at + 5, o + q)):
                    out_res.add(oo % 16)
                    src_res.add(so % 16)
                    pairs.add((oo % 16, so % 16))
            if d.startswith("ab"):
                assert g == b"ab " + b"R" * q + b" cd " + b"R" * q
            src += len(d)
            out += len(g)
    assert out_res == set(range(16)) and src_res == set(range(16))
    assert len(pairs) > 128


# ---------------------------------------------------------------- 5. cursor crossing

def test_many_tiny_documents():
    """300 documents of 0-3 bytes: many documents, gaps and pieces inside one 16-byte chunk."""
    b = B()
    eng, orc = b.build(["a"]), OracleEngine(b, ["a"])
    rng = Rng(0x7157)
    docs = ["".join("abc"[rng.next() % 3] for _ in range(rng.next() % 4)) for _ in range(300)]
    assert {len(d) for d in docs} == {0, 1, 2, 3}
    opts = O().threshold(0.9)
    for reps in (["XY"], [""], ["0123456789abcdefg"], [None]):
        _, compared, ties = check(eng, docs, reps, opts, orc)
        assert ties == 0 and compared == 300


@pytest.mark.parametrize("shift", [-1, 0, 1])
def test_tile_edges(shift):
    """A document boundary and a piece boundary at the copy kernel's tile size - 1, + 0, + 1."""
    b = B()
    eng = b.build(["hello"])
    opts = O().threshold(0.9)
    fill = "zyxwv" * (TILE // 5 + 2)
    edge = TILE + shift
    # document boundary at output offset `edge`; the next document starts with a piece
    got, _, _ = check(eng, [fill[:edge], "hello tail", "", "x"], ["HELLO!"], opts)
    assert got[1] == b"HELLO! tail"
    # piece begins at `edge`, ends at `edge`, and a replacement straddles it
    for lead, rep in ((edge, "R" * 7), (edge - 7, "R" * 7), (edge - 3, "R" * 7), (edge, ""), (edge - 5, None)):
        doc = fill[:lead] + "hello" + fill[:40]
        got, _, _ = check(eng, [doc, "hello"], [rep], opts)
        assert got[0] == (fill[:lead] + ("hello" if rep is None else rep) + fill[:40]).encode()


def test_document_longer_than_two_tiles():
    b = B().fuzzy(L().edits(1))
    eng = b.build(["hello", "world"])
    opts = O().threshold(0.8)
    parts, n = [], 0
    rng = Rng(0x10c)
    while n < 2 * TILE + 700:
        w = ["hello", "wxrld", "helo", "world"][rng.next() % 4] if rng.next() % 3 == 0 else "q" * (1 + rng.next() % 23)
        parts.append(w + " ")
        n += len(w) + 1
    doc = "".join(parts)
    # matches on both sides of (and across) the source's tile edges as well
    doc = doc[:TILE - 2] + "hello" + doc[TILE + 3:2 * TILE - 6] + " world" + doc[2 * TILE:]
    for reps in (["<<HELLO>>", ""], ["", "W"], [None, "0123456789abcdefghijklmnopqrstuvwxyz"]):
        got, _, _ = check(eng, ["hello", doc, "", doc[:100]], reps, opts)
        assert len(got[1]) != len(doc) or reps[0] is None


# ---------------------------------------------------------------- 6. options

def test_orders_choose_the_candidate():
    b = B().fuzzy(L().edits(1))
    pats = ["hello", "hellos", "vest", "vestibulum"]
    reps = ["<5>", "<6>", "<4>", "<10>"]
    eng, orc = b.build(pats), OracleEngine(b, pats)
    docs = ["hello!", "vestibulun", "say hello! to vestibulun"]
    res = {}
    for order in (Order.Default, Order.Greedy, Order.CoverageWeighted):
        res[order], compared, _ = check(eng, docs, reps, options(0.7, order), orc)
        assert compared == len(docs)
    assert res[Order.Greedy][0] != res[Order.Default][0]
    assert res[Order.CoverageWeighted][1] != res[Order.Default][1]


def test_unique_is_per_document():
    b = B()
    pats = [Pattern("ab").custom_unique_id(1), Pattern("cd").custom_unique_id(1)]
    eng, orc = b.build(pats), OracleEngine(b, pats)
    docs = ["ab cd ab", "cd ab", "ab", "cd"]
    got, compared, _ = check(eng, docs, ["X", "Y"], options(0.9, overlap=Overlap.NonOverlappingUnique), orc)
    assert got == [b"X cd ab", b"Y ab", b"X", b"Y"] and compared == 4  # once per document, not once per batch
    got, _, _ = check(eng, docs, ["X", "Y"], options(0.9), orc)
    assert got == [b"X Y X", b"Y X", b"X", b"Y"]


def test_unsorted_keep_is_normalised():
    b = B().fuzzy(L().edits(1))
    pats = ["hello", "hell", "lo w", "world"]
    eng, orc = b.build(pats), OracleEngine(b, pats)
    docs = ["hello world", "helo wrld hello", "", "lo wo"]
    reps = ["A", "BB", None, ""]
    a, _, _ = check(eng, docs, reps, options(0.6, Order.Unsorted, Overlap.Keep), orc)
    c, _, _ = check(eng, docs, reps, options(0.6, Order.Default, Overlap.NonOverlapping), orc)
    assert a == c


# ---------------------------------------------------------------- 7. random differential

N_BATCHES = 40


@pytest.mark.parametrize("cache", ["off", "k4"])
def test_random_differential(cache, monkeypatch):
    """The first 40 batches of each seed of test_gpu_batch, a random replacement per pattern, Default
    x {NonOverlapping, NonOverlappingUnique}: E1 on every document, E2 on those without a tie."""
    set_knobs(monkeypatch, cache, False)
    compared = ties = replaced = inserts = 0
    for seed, vocab in SEEDS:
        rng, rrng = Rng(seed), Rng(seed ^ 0x5e9_1ace)
        for _ in range(N_BATCHES):
            b, pats, docs, thr = random_batch(rng, vocab)
            reps = [REPS[rrng.next() % len(REPS)] for _ in pats]
            eng, orc = b.build(pats), OracleEngine(b, pats)
            sb = StagedBatch(eng, *batch_offsets([d.encode("utf-8") for d in docs]))
            table = ReplacementTable(eng, reps)
            for overlap in (Overlap.NonOverlapping, Overlap.NonOverlappingUnique):
                _, c, t = check(eng, docs, reps, options(thr, overlap=overlap), orc, sb=sb, table=table)
                compared += c
                ties += t
                replaced += sb.replaced
            recs, _ = sb.search_records(options(thr))
            inserts += int((recs["start"] == recs["end"]).sum())
    share = ties / (compared + ties)
    print(f"E2 compared {compared}, excluded as ties {ties} ({100 * share:.2f} %), records applied {replaced}, "
          f"empty spans {inserts}")
    assert share <= 0.05
    assert replaced > 0 and inserts > 0


# ---------------------------------------------------------------- 8. device output

def _device(docs):
    import torch
    data, off = batch_offsets([d.encode("utf-8") for d in docs])
    t = torch.from_numpy(np.frombuffer(data or b"\0", dtype=np.uint8).copy()).cuda()
    o = torch.from_numpy(np.asarray(off, dtype=np.uint64).view(np.int64).copy()).cuda()
    return data, off, t, o


def test_device_output():
    import torch
    b = B().fuzzy(L().edits(1))
    eng = b.build(["hello", "world"])
    reps = ["«HELLO»", ""]
    docs = ["hello world", "", "helo wrld hello", "wörld", "x" * 50]
    opts = O().threshold(0.6)
    want, _, _ = check(eng, docs, reps, opts)
    sb = StagedBatch(eng, *batch_offsets([d.encode() for d in docs]))
    table = ReplacementTable(eng, reps)
    host, host_off = sb.replace_bytes(table, opts)
    n = len(host)
    assert host == b"".join(want) and n > 16
    small = torch.full((n - 1,), 0xAB, dtype=torch.uint8, device="cuda")
    with pytest.raises(DeviceError) as ei:
        sb.replace_bytes(table, opts, out=small)
    assert ei.value.code == _native.FAC_E_OUTPUT_CAPACITY and ei.value.needed == n
    assert bool((small == 0xAB).all())  # nothing was written
    for pad in (0, 1):  # a 16-byte aligned buffer, and one that is not
        buf = torch.full((n + 32,), 0xCD, dtype=torch.uint8, device="cuda")
        exact = buf[pad:pad + n]
        dev_off = torch.full((len(docs) + 1,), -1, dtype=torch.int64, device="cuda")
        got, got_off = sb.replace_bytes(table, opts, out=exact, offsets_out=dev_off)
        assert got.cpu().numpy().tobytes() == host and list(got_off) == list(host_off)
        assert dev_off.cpu().tolist() == [int(x) for x in host_off]
        assert bool((buf[:pad] == 0xCD).all()) and bool((buf[pad + n:] == 0xCD).all())  # and nothing beside it


def test_restaged_batch_gives_its_own_answer():
    b = B().fuzzy(L().edits(1))
    eng = b.build(["hello", "world"])
    reps = ["H", None]
    opts = O().threshold(0.6)
    table = ReplacementTable(eng, reps)
    first = ["hello world", "zz", "wrld"]
    second = ["no", "helo " * 30, "", "world hello", "q"]
    want = [check(eng, dd, reps, opts, table=table)[0] for dd in (first, second)]
    keep, sb = [], None
    for which in (0, 1, 0):
        data, off, t, o = _device((first, second)[which])
        keep.append((t, o))
        sb = StagedBatch.from_device(eng, t.data_ptr(), o.data_ptr(), len(off) - 1, len(data), reuse=sb)
        out, offs = sb.replace_bytes(table, opts)
        assert [out[int(offs[d]):int(offs[d + 1])] for d in range(len(off) - 1)] == want[which]


# ---------------------------------------------------------------- 9. errors

def test_errors():
    b = B()
    eng = b.build(["hello", "world"])
    with pytest.raises(DeviceError) as ei:  # the wrong pattern count
        ReplacementTable(eng, ["x"])
    assert ei.value.code == _native.FAC_E_INVALID
    with pytest.raises(DeviceError) as ei:
        ReplacementTable(eng, ["x", "y", "z"])
    assert ei.value.code == _native.FAC_E_INVALID
    with pytest.raises(DeviceError) as ei:  # invalid UTF-8 in a replacement
        ReplacementTable(eng, ["ok", b"\xc3"])
    assert ei.value.code == _native.FAC_E_INVALID
    ReplacementTable(eng, ["ok", None])
    other = b.build(["hello"])  # a table of another engine's pattern count
    sb = StagedBatch(eng, *batch_offsets([b"hello"]))
    with pytest.raises(DeviceError) as ei:
        sb.replace_bytes(ReplacementTable(other, ["x"]), O().threshold(0.9))
    assert ei.value.code == _native.FAC_E_INVALID
    bm = B().fuzzy(L().edits(1)).mapping("ss", "ß")
    em = bm.build(["strasse"])
    tm = ReplacementTable(em, ["road"])
    assert em.replace_batch(["strasse", "x"], O().threshold(0.9), tm) == ["road", "x"]  # ASCII documents are fine
    with pytest.raises(UnsupportedConfiguration):  # as fac_search_batch
        em.replace_batch(["strasse", "straße"], O().threshold(0.9), tm)
