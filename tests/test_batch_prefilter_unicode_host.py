"""Pre-filtered batches with non-ASCII documents, the parts that need no GPU: the opt-in is exported,
declared and bound, and the documents of test_gpu_batch_prefilter_unicode.py meet, by the oracle
alone, the conditions that make its comparisons mean something."""
import ctypes
import inspect
import os
import re

import pytest

import batch_unicode_cases as cases
from fuzzy_aho_corasick import FuzzyAhoCorasickBuilder as B, FuzzyLimits as L, Order, Overlap
from oracle_harness import OracleEngine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def builder():
    return B().fuzzy(L().edits(1)).case_insensitive(True)


def test_the_opt_in_is_exported_declared_and_bound():
    import fuzzy_aho_corasick as fac
    from fuzzy_aho_corasick import _native
    name = "fac_batch_allow_unicode_prefilter"
    lib = ctypes.CDLL(_native.LIB_PATH)
    header = open(os.path.join(REPO, "include", "fac.h")).read()
    assert hasattr(lib, name) and name in _native.SIGNATURES and re.search(r"\b%s\(" % name, header)
    assert _native.SIGNATURES[name] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32])
    assert _native.lib.fac_batch_allow_unicode_prefilter(None, 1) == _native.FAC_E_INVALID
    assert "NULL" in _native.last_error()
    for fn in (fac.StagedBatch.__init__, fac.StagedBatch.from_device):
        p = inspect.signature(fn).parameters
        assert "unicode_prefilter" in p and p["unicode_prefilter"].default is False  # default off
    p = inspect.signature(fac.StagedBatch.allow_unicode_prefilter).parameters
    assert p["on"].default is True
    assert "all ASCII or opted in" in header


@pytest.mark.parametrize("shift", [-1, 0, 1])
@pytest.mark.parametrize("which", ["packed", "qgram", "mixed"])
def test_windows_spread_over_the_boundary_batch(which, shift):
    pats, thr = cases.ENGINES[which]
    assert any(len(g) > 1 for p in pats for g in cases.graphemes(p))  # a pattern grapheme of several code points
    orc = OracleEngine(builder(), pats)
    docs = cases.boundary_docs(pats, shift, 0xB0D5 + shift)
    per_doc = [orc.prefilter_windows(d, thr) for d in docs]
    assert all(w is not None for w in per_doc)
    none = sum(len(w) == 0 for w in per_doc)
    two = sum(len(w) >= 2 for w in per_doc)
    assert 4 * none >= len(docs) and 4 * two >= len(docs), (none, two, len(docs))
    want = cases.oracle_windows(orc, docs, thr)
    ends, starts = cases.is_cut_pair(docs)
    got_ends, got_starts = {(d, e) for d, _, e in want}, {(d, s) for d, s, _ in want}
    for e, s in zip(ends, starts):
        assert e in got_ends and s in got_starts, (e, s)
    # both slice kinds: a merged window of a non-ASCII document that is all ASCII, and one that is not
    kinds = {cases.window_bytes(docs[d], s, e).isascii() for d, s, e in want if not docs[d].isascii()}
    assert kinds == {True, False}
    for batch in cases.small_batches(pats):
        assert not batch[0].isascii() and not batch[-1].isascii()
    last = cases.small_batches(pats)[0]
    assert (len(last) - 1, cases.glen(last[-1])) in {(d, e) for d, _, e in cases.oracle_windows(orc, last, thr)}


def test_slice_documents_hold_the_slices():
    orc = OracleEngine(builder(), cases.SLICE_PATS)
    docs = cases.slice_docs()
    assert all(not d.isascii() for d in docs)
    wins = [(d, s, e, cases.window_bytes(docs[d], s, e)) for d, s, e in cases.oracle_windows(orc, docs, cases.SLICE_THR)]
    texts = [w[3].decode("utf-8") for w in wins]
    assert any(t.isascii() and "\r\n" in t for t in texts)
    first = lambda t: [g.isascii() for g in cases.graphemes(t)]  # noqa: E731
    assert any(len(f) > 1 and not f[0] and all(f[1:]) for f in map(first, texts))  # ASCII except the first grapheme
    assert any(len(f) > 1 and not f[-1] and all(f[:-1]) for f in map(first, texts))  # ... except the last
    assert any(e == cases.glen(docs[d]) and s > 0 for d, s, e, _ in wins)  # at the very end of the document
    assert any(e - s == 1 for _, s, e, _ in wins)  # one grapheme long
    assert any(len(w[3]) > 64 for w in wins)
    assert any(cases.BIG in t for t in texts)
    rows = sum(len(orc.raw_rows(d, cases.SLICE_THR, prefilter=True)) for d in docs[-5:])
    assert rows >= 8  # U+0130, U+1E9E and capital sigma fold onto pattern symbols


def test_the_random_differential_has_windows_records_and_few_ties():
    orc = OracleEngine(builder(), cases.DIFF_PATS)
    uni = with_window = records = tied = total = 0
    for seed in cases.DIFF_SEEDS:
        for doc in cases.random_docs(seed):
            total += 1
            assert cases.glen(doc) <= 200
            rows = orc.raw_rows(doc, cases.DIFF_THR, prefilter=True)
            records += len(rows)
            if not doc.isascii():
                uni += 1
                with_window += len(orc.prefilter_windows(doc, cases.DIFF_THR)) > 0
            kept = orc.apply_rows(rows, Order.Default, Overlap.NonOverlapping)
            tied += len({r[0] for r in kept}) != len(kept)
    assert uni >= total // 3 and 2 * with_window >= uni, (uni, with_window)
    assert records >= 100 and 4 * tied <= total, (records, tied, total)
