"""The device Unicode tables and the device folding over every scalar value (stage_kernels.hip).

The UAX #29 properties and the folded first code point are reached through three tiers (LDS copies
below 0x800, the BMP tables bmp_tables_kernel builds, the range search for astral code points) by
four segmenters (seg_tile_kernel's fast path and lookback restart, seg_hard_kernel, batch_seg_kernel)
and three folding consumers (write_tile_kernel, batch_seg_kernel, symbol_ids_kernel). Each test
compares what the device wrote (grapheme starts, fac_haystack_text_chars / fac_batch_text_chars,
symbol ids, search records) with regex \\X and str.lower() over all 1 112 064 scalar values in the
eight contexts of unicode_contexts, or over the constructed sets its docstring states. Nothing is
sampled out; a failure names the code point and its tier.

Every whole-context haystack (7-21 MB, a few million graphemes) is staged in one piece: the grapheme
limit is u32::MAX, so no per-plane staging is needed."""
import ctypes

import numpy as np
import pytest

import unicode_contexts as U
from fuzzy_aho_corasick import FuzzyAhoCorasickBuilder as B, _native
from fuzzy_aho_corasick.engine import StagedBatch, StagedHaystack
from oracle_harness import OracleEngine, graphemes
from test_gpu_parity import rows
from test_gpu_prefilter_stream import _symbol_table, _want_ids

pytestmark = pytest.mark.gpu

_u32p = ctypes.POINTER(ctypes.c_uint32)
_u64p = ctypes.POINTER(ctypes.c_uint64)
K_LOOKBACK = 1024  # stage_kernels.hip kLookback
ONE = 0x3F800000   # f32 1.0


@pytest.fixture(scope="module")
def engines():
    """Any engine stages a haystack; only its case-insensitivity reaches the staging kernels."""
    return {ci: B().case_insensitive(ci).device(0).build(["a"]) for ci in (True, False)}


@pytest.fixture(scope="module", params=range(len(U.CONTEXTS)), ids=U.CONTEXT_IDS)
def ctx(request):
    """One context's text over every scalar value with its regex reference, computed once per
    context and shared (read-only) by the tests of that context."""
    pre, post, _ = U.CONTEXTS[request.param]
    c = U.ContextText(pre, post)
    assert len(c.cps) == 1_112_064 and len(c.data) > 400 * 16384  # hundreds of 16 KiB tiles
    for a in (c.starts, c.first):
        a.setflags(write=False)
    return c


@pytest.fixture(scope="module")
def representatives():
    reps = U.class_representatives()
    assert 40 <= len(reps) <= 200
    return reps


def _check_staged(c, st, ci, n_graphemes=None):
    n = len(c.starts) if n_graphemes is None else n_graphemes
    U.check_starts(c, st.grapheme_starts(), c.starts[:n])
    U.check_chars(c, st.text_chars(), c.folds(ci)[:n])
    assert st.graphemes == n


# ---------------------------------------------------------------- seg_tile_kernel / write_tile_kernel

@pytest.mark.parametrize("ci", [True, False], ids=["ci", "cs"])
def test_staged_host_bytes(ctx, engines, ci):
    """StagedHaystack(engine, bytes): the starts, and the folded (ci) or raw (cs) first code points,
    of every line. 1- to 4-byte sequences fall at every lane offset of write_tile_kernel's 8-byte
    register decode, at its 256-byte steps and at the 16 KiB tile edges."""
    _check_staged(ctx, StagedHaystack(engines[ci], ctx.data), ci)


def test_staged_text_ending_inside_a_line(ctx, engines):
    """The same text without its final "\\n": it ends with the last line's `post`, a multi-byte
    sequence in seven of the contexts, in the last lanes of the last, partial tile. The final "\\n"
    was a grapheme of its own (the code point before it is never CR), so the expectation loses
    exactly its last entry."""
    assert ctx.text[-1] == "\n" and ctx.text[-2] != "\r" and int(ctx.starts[-1]) == len(ctx.data) - 1
    _check_staged(ctx, StagedHaystack(engines[True], ctx.data[:-1]), True, len(ctx.starts) - 1)


@pytest.mark.parametrize("ctx", [0], indirect=True, ids=[U.CONTEXT_IDS[0]])
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned16", "offset1"])
def test_staged_from_device_bytes(ctx, engines, shift):
    """StagedHaystack.from_device (UTF-8 check and is_ascii on the device too) on a 16-byte-aligned
    buffer and on one a byte further, which takes the byte loads of the `aligned == 0` branches."""
    import torch
    buf = torch.zeros(len(ctx.data) + 32, dtype=torch.uint8, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    view = buf[shift:shift + len(ctx.data)]
    view.copy_(torch.frombuffer(bytearray(ctx.data), dtype=torch.uint8))
    torch.cuda.synchronize()
    assert view.data_ptr() % 16 == shift
    _check_staged(ctx, StagedHaystack.from_device(engines[True], view.data_ptr(), len(ctx.data)), True)


# ---------------------------------------------------------------- batch_seg_kernel

def _document_failure(bt, sb, d, got):
    """A document whose grapheme count or is_ascii is wrong: name the first wrong boundary's code point."""
    o, n = int(bt.doc_first[d]), int(bt.doc_count[d])
    want = bt.starts[o:o + n]
    i = U.first_difference(np.asarray(sb.grapheme_starts(d), dtype=np.uint64), want)
    rel = 0 if i is None else min(int(x[i]) for x in (sb.grapheme_starts(d), want) if i < len(x))
    raise AssertionError(f"(fac_batch_doc_graphemes, starts, text_chars, is_ascii) = {got}, expected {n} graphemes, "
                         f"is_ascii {bool(bt.doc_ascii[d])}: first differing {bt.where_doc(d, rel)}")


@pytest.mark.parametrize("k", range(len(U.CONTEXTS)), ids=U.CONTEXT_IDS)
def test_batch_documents(k, engines, representatives):
    """One document per 64 consecutive code points (17 376 of them), the first document of every
    plane starting on the code point itself, and one document per class representative that starts
    on it too (seg_init of every property class at start-of-document). Per document: the grapheme
    count and is_ascii, the document-relative starts and the folded first code points against regex
    \\X on that document alone."""
    pre, post, _ = U.CONTEXTS[k]
    bt = U.BatchText(pre, post, alone=representatives)
    assert bt.n_docs == 17376 + len(representatives)
    plane_docs = [int(np.searchsorted(bt.cps[bt.doc_line[:-1]][:17376], p * U.PLANE)) for p in range(U.N_PLANES)]
    for p, d in enumerate(plane_docs):  # the document starts with the plane's first code point, no `pre`
        assert bt.data[int(bt.doc_byte[d]):].startswith(chr(p * U.PLANE).encode()), p
    sb = StagedBatch(engines[True], bt.data, bt.doc_byte)
    lib, h = _native.lib, sb._h
    got_s = np.full(len(bt.starts) + 1, np.iinfo(np.uint64).max, dtype=np.uint64)
    got_c = np.full(len(bt.first) + 1, 0xFFFFFFFF, dtype=np.uint32)
    want_c = U.folded(bt.first, True)
    s_addr, c_addr = got_s.ctypes.data, got_c.ctypes.data
    asc = ctypes.c_int32()
    counts, ascii_flags = bt.doc_count.tolist(), bt.doc_ascii.tolist()
    for d, o in enumerate(bt.doc_first[:-1].tolist()):
        n = counts[d]
        nd = lib.fac_batch_doc_graphemes(h, d, ctypes.byref(asc))
        ns = lib.fac_batch_grapheme_starts(h, d, ctypes.cast(s_addr + 8 * o, _u64p), n)
        nc = lib.fac_batch_text_chars(h, d, ctypes.cast(c_addr + 4 * o, _u32p), n)
        if not (nd == ns == n and bool(asc.value) == ascii_flags[d] and nc == (0 if ascii_flags[d] else n)):
            _document_failure(bt, sb, d, (nd, ns, nc, bool(asc.value)))
        if ascii_flags[d]:  # no folded characters are kept for an ASCII document: nothing was written
            assert (got_c[o:o + n] == 0xFFFFFFFF).all(), bt.where_doc(d)
            got_c[o:o + n] = want_c[o:o + n]
    i = U.first_difference(got_s[:-1], bt.starts)
    if i is not None:
        d = int(np.searchsorted(bt.doc_first, i, side="right")) - 1
        raise AssertionError(f"starts differ at grapheme {i - int(bt.doc_first[d])}: got {int(got_s[i])}, expected "
                             f"{int(bt.starts[i])}: {bt.where_doc(d, min(int(got_s[i]), int(bt.starts[i])))}")
    i = U.first_difference(got_c[:-1], want_c)
    if i is not None:
        d = int(np.searchsorted(bt.doc_first, i, side="right")) - 1
        raise AssertionError(f"folded characters differ: got U+{int(got_c[i]):04X}, expected U+{int(want_c[i]):04X}: "
                             f"{bt.where_doc(d, int(bt.starts[i]))}")
    assert got_s[-1] == np.iinfo(np.uint64).max and got_c[-1] == 0xFFFFFFFF  # nothing past the last document


# ---------------------------------------------------------------- lookback restart, seg_hard_kernel

@pytest.mark.parametrize("post", ["\u0915", "\U0001F469", "\u11A8"], ids=["consonant", "pictographic", "hangulT"])
@pytest.mark.parametrize("run", [300, 700], ids=["lookback", "hard"])
def test_lookback_and_hard_paths(engines, representatives, run, post):
    """The lowest and the highest code point of every (GCB, Extended_Pictographic, InCB) triple in
    every tier, after "x" and a run of U+0301 with no resync code point in it. 300 of them (600
    bytes, under kLookback): every thread of the run and the code point's own restart from the "x"
    (the lookback branch of seg_tile_kernel). 700 (1 400 bytes): the threads further than kLookback
    from the "x", the code point's among them, find no resync point, and seg_hard_kernel segments
    their bytes. The library keeps no counter of the hard path; the construction (asserted below)
    alone puts the code point on it."""
    pre = "x" + "\u0301" * run
    c = U.ContextText(pre, post, cps=representatives)
    n_pre = len(pre.encode())
    if run == 300:
        assert n_pre + 64 + 8 < K_LOOKBACK  # from any thread's first code point of a line back to its "x"
    else:
        assert n_pre - 64 > K_LOOKBACK + 64  # the 64 bytes that hold the code point lie past kLookback
    assert len(c.starts) >= 3 * len(representatives)
    _check_staged(c, StagedHaystack(engines[True], c.data), True)


# ---------------------------------------------------------------- lower_full_dev (symbol_ids_kernel)

def test_symbol_ids_fold_every_cased_code_point():
    """All 1 393 code points whose lowercase differs from them (225 astral, U+0130 with two output
    code points), in groups of 120: a case-insensitive engine whose pattern graphemes are the
    group's lowercase strings must give every uppercase form its lowercase's symbol id, through
    lower_full_dev's full mapping. Uppercase + U+0301 (another grapheme) and non-members give 0."""
    cased = U.cased_code_points()
    assert len(cased) == 1393 and sum(cp >= 0x10000 for cp in cased) == 225 and 0x130 in cased
    for lo in range(0, len(cased), 120):
        group = cased[lo:lo + 120]
        lows = list(dict.fromkeys(chr(cp).lower() for cp in group))
        pats = ["".join(lows[i:i + 40]) for i in range(0, len(lows), 40)]
        for i, p in enumerate(pats):
            assert graphemes(p) == lows[40 * i:40 * i + 40]
        eng = B().case_insensitive(True).device(0).build(pats)
        assert eng.with_prefilter().is_active()
        table = _symbol_table(pats, True)
        assert len(table) == len(lows) <= 255
        ups = [chr(cp) for cp in group]
        text = " ".join(ups + lows + [u + "\u0301" for u in ups] + ["\u65E5", "\U0001F600", "7", "\u0301"])
        want = _want_ids(table, text, True)
        by_g = dict(zip(graphemes(text), want))
        for u in ups:
            assert by_g[u] == table[u.lower()] and by_g[u + "\u0301"] == 0, hex(ord(u))
        got = StagedHaystack(eng, text.encode()).symbol_ids()
        i = U.first_difference(got, want)
        assert i is None, f"symbol id {got[i]} != {want[i]} at grapheme {i}: {graphemes(text)[i]!r} " \
                          f"U+{ord(graphemes(text)[i][0]):04X}, tier {U.tier(ord(graphemes(text)[i][0]))}"


# ---------------------------------------------------------------- host fold against device fold

def test_capitals_found_by_lowercase_patterns():
    """The patterns are folded on the host (builder, unicode.cpp), the haystack on the device: all
    225 astral cased code points and 300 BMP ones, taken in turn from every 256-code-point block that
    has any (every script of the lowercase table), U+0130 among them. Every "x C x" must give the
    oracle's records bit for bit, and C is found with similarity 1.0 by a pattern that begins with its
    lowercase's first code point."""
    cased = U.cased_code_points()
    astral = [cp for cp in cased if cp >= 0x10000]
    blocks = {}
    for cp in cased:
        if cp < 0x10000 and cp != 0x130:
            blocks.setdefault(cp >> 8, []).append(cp)
    bmp, depth = [0x130], 0
    while len(bmp) < 300:
        for b in sorted(blocks):
            if depth < len(blocks[b]) and len(bmp) < 300:
                bmp.append(blocks[b][depth])
        depth += 1
    assert len(astral) == 225 and len(set(bmp)) == 300 and {cp >> 8 for cp in bmp} >= set(blocks)
    capitals = sorted(bmp) + astral
    lows = list(dict.fromkeys(chr(cp).lower() for cp in capitals))
    text = "\n".join(f"x {chr(cp)} x" for cp in capitals)
    builder = B().case_insensitive(True).device(0)
    got = rows(builder.build(lows).search_raw(text, 0.9))
    want = rows(OracleEngine(builder, lows).search_raw(text, 0.9))
    assert got == want
    exact = {}
    for r in got:
        if r[3] == ONE:
            exact.setdefault((r[0], r[1]), set()).add(lows[r[2]][0])
    pos = 0
    for cp in capitals:  # (the search compares first code points: "i" and "i" + U+0307 both match a folded I)
        n = len(chr(cp).encode())
        assert chr(cp).lower()[0] in exact.get((pos + 2, pos + 2 + n), ()), f"U+{cp:04X} ({U.tier(cp)}) not found"
        pos += 2 + n + 2 + 1
