"""Batches of non-ASCII documents for engines with multi-character mappings, the parts that need no
GPU: the opt-in and the grapheme-id exports are exported, declared and bound, the Python keywords
exist and default to off, and the documents of test_gpu_batch_mappings.py meet, by the oracle alone,
the conditions that make its comparisons mean something."""
import ctypes
import inspect
import os
import re

import pytest

import batch_mapping_cases as cases
from fuzzy_aho_corasick import FuzzyAhoCorasickBuilder as B, FuzzyLimits as L
from oracle_harness import OracleEngine, graphemes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPORTS = {
    "fac_batch_allow_unicode_mappings": (ctypes.c_int, 2),
    "fac_engine_grapheme_id": (ctypes.c_uint32, 3),
    "fac_haystack_grapheme_ids": (ctypes.c_int64, 5),
    "fac_batch_grapheme_ids": (ctypes.c_int64, 5),
}


def test_the_exports_are_exported_declared_and_bound():
    from fuzzy_aho_corasick import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    header = open(os.path.join(REPO, "include", "fac.h")).read()
    for name, (restype, nargs) in EXPORTS.items():
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _native.SIGNATURES, name
        assert _native.SIGNATURES[name][0] == restype and len(_native.SIGNATURES[name][1]) == nargs, name
    assert _native.SIGNATURES["fac_batch_allow_unicode_mappings"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32])
    assert _native.lib.fac_batch_allow_unicode_mappings(None, 1) == _native.FAC_E_INVALID
    assert "NULL" in _native.last_error()
    assert _native.lib.fac_engine_grapheme_id(None, b"a", 1) == 0
    assert _native.lib.fac_haystack_grapheme_ids(None, None, None, None, 0) == -_native.FAC_E_INVALID
    assert _native.lib.fac_batch_grapheme_ids(None, None, None, None, 0) == -_native.FAC_E_INVALID
    assert "fac_batch_allow_unicode_mappings" in header.split("Limits of the implementation")[1].split("*/")[0]


def test_the_python_keywords_exist_and_default_to_off():
    import fuzzy_aho_corasick as fac
    for fn in (fac.StagedBatch.__init__, fac.StagedBatch.from_device):
        p = inspect.signature(fn).parameters
        assert "unicode_mappings" in p and p["unicode_mappings"].default is False
    assert inspect.signature(fac.StagedBatch.allow_unicode_mappings).parameters["on"].default is True
    for name in ("search_batch", "replace_batch", "extract_batch", "matched_strings_batch", "strip_prefix_batch",
                 "strip_suffix_batch", "segment_text_batch", "segment_batch", "split_batch"):
        p = inspect.signature(getattr(fac.FuzzyAhoCorasick, name)).parameters
        assert "unicode_mappings" in p and p["unicode_mappings"].default is False, name
    for name in ("grapheme_ids",):
        assert hasattr(fac.StagedBatch, name) and hasattr(fac.StagedHaystack, name)
    assert hasattr(fac.FuzzyAhoCorasick, "grapheme_id")


@pytest.mark.parametrize("seed,vocab", cases.DIFF_SEEDS)
def test_the_differential_has_records_that_only_a_mapping_explains(seed, vocab):
    """Per seed, by the oracle alone: at least 50 records in non-ASCII documents, at least 5 of them
    without insertion or deletion whose matched text and pattern differ in grapheme count."""
    rng = cases.Rng(seed)
    records = only = 0
    for _ in range(cases.N_BATCHES):
        b, pats, docs, thr = cases.mapping_batch(rng, vocab)
        orc, w = OracleEngine(b, pats), cases.words(pats)
        for doc in docs:
            if doc.isascii():
                continue
            rows = orc.raw_rows(doc, thr)
            records += len(rows)
            only += sum(cases.mapping_only(r, doc.encode("utf-8"), w[r[2]]) for r in rows)
    assert records >= 50 and only >= 5, (records, only)


def test_the_cuts_cut_where_they_say():
    """The hand-built batches by the oracle alone: a side split by a document boundary matches in
    neither document though it matches in their concatenation; a side that ends a document matches."""
    orc = OracleEngine(cases.cut_builder(B, L), cases.CUT_PATS)
    # (a mapping counts as one substitution of no penalty: the whole pattern at similarity 1)
    hit = lambda doc, p: any(r[2] == p and r[3] == 1.0 for r in orc.raw_rows(doc, cases.CUT_THR))  # noqa: E731
    batches = cases.cut_batches()
    split = batches["split_ss"]
    for a, c in ((0, 1), (2, 3), (4, 5)):
        assert not hit(split[a], 0) and not hit(split[c], 0) and hit(split[a] + split[c], 0)
    assert not hit(split[6], 0) and not hit(split[8], 0) and hit(split[6] + split[7] + split[8], 0)
    ends = batches["ends_at_last"]
    assert hit(ends[0], 2) and hit(ends[2], 2) and hit(ends[3], 1) and hit(ends[5], 2) and hit(ends[6], 0)
    assert hit(ends[-1], 2)  # the batch's last document
    short = batches["one_short"]
    assert not any(hit(d, p) for d in short for p in range(3))
    assert hit(short[0] + short[1], 2) and hit(short[2] + short[3], 1) and hit(short[4] + short[5], 0)
    for name, lens in (("tile_256", {256}), ("tile_257", {256, 257})):
        docs = batches[name]
        assert lens <= {len(graphemes(d)) for d in docs}, name
        assert any(hit(d, 0) for d in docs if len(graphemes(d)) in lens), name
    for docs in batches.values():
        assert any(not d.isascii() for d in docs)
