"""The grapheme ids of Unicode text for engines with multi-character mappings, looked up on the device
(grapheme_ids_kernel, batch_grapheme_ids_kernel): for every engine, text and lifecycle below, the
device's ids equal fac_engine_grapheme_id -- the host's fold and hash-map lookup -- of the bytes of
every grapheme the device staged."""
import numpy as np
import pytest
import torch

from fuzzy_aho_corasick import (FuzzyAhoCorasickBuilder as B, FuzzyLimits as L, SearchOptions as O, StagedBatch,
                                StagedHaystack, batch_offsets)
from oracle_harness import OracleEngine, fold, graphemes
from test_gpu_parity import MAP_FILLER_UNI, MAP_RULES, rows

pytestmark = pytest.mark.gpu

E_ACUTE = "e\u0301"  # decomposed: a key of two code points
E_CIRC = "e\u0302"   # shares its first code point with it; in no dictionary
I_DOT = "i\u0307"    # what U+0130 folds to: one code point becomes two
CEDILLA = "\u0327"
SMALL_PATS = ["stra\u00dfe", "encyclop\u00e6dia", "c\u0153ur", "caf" + E_ACUTE, "\u03a9\u03bc\u03ad\u03b3\u03b1", "a\r\nb",
              I_DOT + "stanbul", "alexandr"]
MARKS = ["\u0301", "\u0300", "\u0302", "\u0308", CEDILLA]
LONG = ["x" + "\u0301" * 12 + CEDILLA * (k + 1) for k in range(100)]  # keys of 14..113 code points


def big_patterns():
    """More than 512 keys and more than 2048 pool code points: 600 CJK graphemes, 26 x 5 decomposed
    accented letters (keys of two code points, many sharing their first), and the small dictionary --
    the table stays in global memory, has probe chains, and most ids are above 255."""
    cjk = [chr(0x4E00 + 7 * i) for i in range(600)]
    acc = [chr(ord("a") + i) + m for i in range(26) for m in MARKS if chr(ord("a") + i) + m != E_CIRC]
    units = cjk + acc + LONG
    return SMALL_PATS + ["".join(units[i:i + 10]) for i in range(0, len(units), 10)]


def build(ci: bool, big: bool):
    b = B().fuzzy(L().edits(1)).case_insensitive(ci)
    for a, c in MAP_RULES:
        b = b.mapping(a, c)
    return b, (big_patterns() if big else SMALL_PATS)


@pytest.fixture(scope="module", params=[(True, False), (False, False), (True, True), (False, True)],
                ids=["ci-small", "cs-small", "ci-big", "cs-big"])
def engine(request):
    ci, big = request.param
    b, pats = build(ci, big)
    eng = b.build(pats)
    eng.ci, eng.big, eng.pats = ci, big, pats
    return eng


def want_ids(eng, data: bytes, starts, end=None):
    cuts = list(starts) + [len(data) if end is None else end]
    return [eng.grapheme_id(data[cuts[i]:cuts[i + 1]].decode("utf-8")) for i in range(len(cuts) - 1)]


def check_text(eng, text: str, sh=None):
    data = text.encode("utf-8")
    sh = sh or StagedHaystack(eng, data)
    got = sh.grapheme_ids(engine=eng)
    if data.isascii():
        assert len(got) == 0
        return got
    starts = [int(x) for x in sh.grapheme_starts()]
    assert len(starts) == len(graphemes(text)) == sh.graphemes
    assert got.dtype == np.uint32 and list(got) == want_ids(eng, data, starts), text
    return got


def units_for(eng):
    keys = [g for p in eng.pats[:40] for g in graphemes(p)]
    other = ["\u00c6", "\u0130", E_CIRC, E_ACUTE + CEDILLA, "e", "\U0001f600", "\u00e9", "\u017f", "\u1e9e", "\u03a3"]
    return MAP_FILLER_UNI + other + keys


def text_of(units, n, salt=0):
    """n graphemes drawn from units, the first not ASCII."""
    out, k = ["\u00df"], salt
    while len(out) < n:  # (a unit may hold two graphemes: cut to n of them)
        k = (k * 1103515245 + 12345) & 0x7FFFFFFF
        out.append(units[(k >> 8) % len(units)])
    return "".join(graphemes("".join(out))[:n])


def test_the_dictionary(engine):
    """The host export itself: pattern graphemes have distinct non-zero ids, folded; the mappings'
    haystack sides are in the dictionary; absent graphemes give 0; the big engines have more than 512
    keys, so ids above 255 and the global-memory table."""
    ids = {}
    for p in engine.pats:
        for g in graphemes(p):
            ids.setdefault(fold(g, engine.ci), engine.grapheme_id(g))
    assert all(v > 0 for v in ids.values()) and len(set(ids.values())) == len(ids)
    assert engine.grapheme_id("\u00df") > 0 and engine.grapheme_id("s") > 0 and engine.grapheme_id("\u0153") > 0
    assert engine.grapheme_id("q") == 0 and engine.grapheme_id("e\u0302") == 0 and engine.grapheme_id("\U0001f600") == 0
    assert engine.grapheme_id("") == 0
    assert (engine.grapheme_id("\u03a9") == engine.grapheme_id("\u03c9")) == engine.ci
    assert (len(ids) > 512 and max(ids.values()) > 600) == engine.big
    plain = B().fuzzy(L().edits(1)).build(["stra\u00dfe"])
    assert plain.grapheme_id("s") == 0 and StagedHaystack(plain, "\u00df".encode()).grapheme_ids() is None


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_tile_edges(engine, n):
    text = text_of(units_for(engine), n, salt=n)
    got = check_text(engine, text)
    assert len(got) == len(graphemes(text)) == n
    if n > 1:
        assert np.count_nonzero(got) > n // 4 and np.count_nonzero(got == 0) > 0
    if engine.big and n >= 255:  # an 8-bit store would show
        big_text = "".join(graphemes("".join(engine.pats[len(SMALL_PATS):]))[:n - 1]) + "\u00df"
        assert check_text(engine, big_text).max() > 255


def test_single_graphemes(engine):
    e = engine
    # the last grapheme has several code points and ends at len
    for tail in (E_ACUTE, "x" + "\u0301" * 12 + "\u0327", "\U0001f1e9\U0001f1ea", "e\u0302"):
        got = check_text(e, "\u00df caf" + tail)
        assert got[-1] == e.grapheme_id(tail)
    assert check_text(e, "\u00df" + E_ACUTE)[-1] > 0
    # "\r\n" is one grapheme and a key
    got = check_text(e, "\u00dfa\r\nb\r\n")
    assert len(got) == 5 and got[2] == got[4] == e.grapheme_id("\r\n") > 0
    # \u00c6 against \u00e6, U+0130 against "i" + U+0307, under folding only
    got = check_text(e, "\u00e6\u00c6\u0130" + I_DOT)
    assert got[0] > 0 and got[3] > 0
    if e.ci:
        assert got[1] == got[0] and got[2] == got[3]
    else:
        assert got[2] == 0 and got[1] == e.grapheme_id("\u00c6") != got[0]
    # a grapheme that equals a key in its first code point only; a key that is its prefix
    got = check_text(e, "\u00dfe\u0302" + E_ACUTE + "\u0327" + "e" + E_ACUTE)
    assert got[1] == 0 and got[2] == 0 and got[3] > 0 and got[4] > 0 and got[3] != got[4]
    # the units of the parity tests' mapping filler, each alone and all together
    for u in MAP_FILLER_UNI:
        check_text(e, "\u00df" + u)
    check_text(e, "".join(MAP_FILLER_UNI) * 3)
    assert len(check_text(e, "plain ascii")) == 0


def test_shard_with_an_open_end(engine):
    text = text_of(units_for(engine), 300, salt=7)
    data = text.encode("utf-8")
    cuts = [0]
    for g in graphemes(text):
        cuts.append(cuts[-1] + len(g.encode("utf-8")))
    a, b, e = cuts[20], cuts[150], cuts[270]  # the text goes on after byte e
    sh = StagedHaystack(engine, data, _shard=(a, b, e, 0, True))
    starts = [int(x) for x in sh.grapheme_starts()]
    assert len(starts) == 250 == sh.graphemes
    got = sh.grapheme_ids()
    assert list(got) == want_ids(engine, data[a:e], starts)
    assert list(got) == list(check_text(engine, text)[20:270])


def test_restage_in_place_follows_the_text(engine):
    units = units_for(engine)
    texts = [text_of(units, 400, 1), text_of(units, 37, 2), text_of(units, 900, 3), "ascii now", text_of(units, 5, 4)]
    sh = None
    for t in texts:
        buf = torch.frombuffer(bytearray(t.encode("utf-8")), dtype=torch.uint8).cuda()
        sh = StagedHaystack.from_device(engine, buf.data_ptr(), buf.numel(), reuse=sh)
        first = check_text(engine, t, sh)
        assert list(check_text(engine, t, sh)) == list(first)  # the cached ids
        torch.cuda.synchronize()


def test_one_haystack_two_engines_in_turn(engine):
    other_b, other_pats = build(not engine.ci, not engine.big)
    other = other_b.build(other_pats)
    text = text_of(units_for(engine), 300, salt=11) + "\u00c6\u0130\u03a9"
    sh = StagedHaystack(engine, text.encode("utf-8"))
    a1 = check_text(engine, text, sh)
    b1 = check_text(other, text, sh)
    a2 = check_text(engine, text, sh)
    assert list(a1) == list(a2) and list(a1) != list(b1)
    # and the searches read their own engine's ids
    o = O().threshold(0.8)
    assert rows(engine.search(text, o)) == rows(OracleEngine(*build(engine.ci, engine.big)).search(text, o))


def batch_docs(engine):
    u = units_for(engine)
    uni = lambda n, s: text_of(u, n, s)  # noqa: E731
    return [uni(30, 1) + E_ACUTE, "ascii one", "", uni(1, 2), "", "", uni(257, 3) + "\U0001f1e9\U0001f1ea", uni(12, 4) + "\u00df",  # -> Unicode
            "abc", uni(40, 5) + "\u0153", "", "ss", uni(255, 6) + E_ACUTE + "\u0327", "", uni(3, 7) + E_ACUTE]  # -> nothing


def check_batch_ids(eng, docs, sb=None):
    enc = [d.encode("utf-8") for d in docs]
    sb = sb or StagedBatch(eng, *batch_offsets(enc))
    got = sb.grapheme_ids(engine=eng)
    want = []
    for d, raw in enumerate(enc):
        n, asc = sb.doc_graphemes(d)
        assert asc == raw.isascii()
        if not asc:
            starts = sb.grapheme_starts(d)
            assert len(starts) == n == len(graphemes(docs[d]))
            want += want_ids(eng, raw, starts)
    assert list(got) == want
    return sb, got


def test_batch_ids(engine):
    """Non-ASCII and ASCII documents alternate with empties between; a non-ASCII document that ends in
    a multi-byte grapheme is followed by an ASCII document, by another non-ASCII one, and by nothing."""
    docs = batch_docs(engine)
    assert not docs[0].isascii() and docs[1].isascii() and not docs[6].isascii() and not docs[7].isascii()
    assert not docs[-1].isascii() and all(len(d.encode()) > len(d) for d in (docs[0][-1], docs[6][-1], docs[-1][-1]))
    _, got = check_batch_ids(engine, docs)
    assert np.count_nonzero(got) > len(got) // 4
    check_batch_ids(engine, docs[:7])          # the last document: 258 graphemes, ends in a flag
    check_batch_ids(engine, ["\u00e9"])
    check_batch_ids(engine, ["", "\u00df", ""])
    sb, got = check_batch_ids(engine, ["abc", "", "de"])
    assert len(got) == 0


def test_batch_restaged_in_place_and_read_by_two_engines(engine):
    other_b, other_pats = build(not engine.ci, engine.big)
    other = other_b.build(other_pats)
    docs = batch_docs(engine)
    sb = None
    for part in (docs, docs[3:9], docs[::-1] + docs, ["x", "y"], docs[5:]):
        enc = [d.encode("utf-8") for d in part]
        data, offs = batch_offsets(enc)
        d_data = torch.frombuffer(bytearray(data or b"\0"), dtype=torch.uint8).cuda()
        d_off = torch.tensor(offs, dtype=torch.int64).cuda()
        sb = StagedBatch.from_device(engine, d_data.data_ptr(), d_off.data_ptr(), len(part), len(data), reuse=sb)
        sb.data = data
        check_batch_ids(engine, part, sb)
        check_batch_ids(other, part, sb)
        check_batch_ids(engine, part, sb)
        torch.cuda.synchronize()
