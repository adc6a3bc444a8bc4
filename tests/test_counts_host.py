"""Term counts, the parts that need no device (fac.h "Term counts of a batch"): the layout of fac_term,
fac_term_total and fac_count_args against the header, the tier constants against fac_internal.h, and
fac_count_records against the pure-Python reference below, which is written from the rule in the
header (a dict by key, max over (order word, -pattern) with the order word computed by struct) and
never calls the library. test_gpu_counts.py imports the reference and the record builder."""
import ctypes
import os
import random
import re
import struct

import numpy as np
import pytest

import fuzzy_aho_corasick as fac
from fuzzy_aho_corasick import FuzzyMatch, FuzzyMatches, FuzzyReplacer, TERM_DTYPE, TermCount, Wrap, _native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits_of(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def order_word(bits):
    """f32::total_cmp as an unsigned compare of the float's bits."""
    return ~bits & 0xFFFFFFFF if bits & 0x80000000 else bits | 0x80000000


def ref_terms(rows, keys=None):
    """The rule: rows are (pattern_index, similarity bits); the terms as (key, count, best similarity
    bits, best pattern) in ascending key order."""
    groups = {}
    for p, bits in rows:
        k = keys[p] if keys is not None else p
        count, best = groups.get(k, (0, (-1, 0)))
        groups[k] = (count + 1, max(best, (order_word(bits), -p)))
    inv = {order_word(bits): bits for _, bits in rows}
    return [(k, groups[k][0], inv[groups[k][1][0]], -groups[k][1][1]) for k in sorted(groups)]


def make_recs(rows):
    """MATCH_DTYPE records with the rows' pattern_index and similarity bits (spans are not read)."""
    recs = np.zeros(len(rows), dtype=_native.MATCH_DTYPE)
    recs["pattern_index"] = [p for p, _ in rows]
    recs["similarity"] = np.array([b for _, b in rows], dtype=np.uint32).view(np.float32)
    recs["end"] = 1
    return recs


def term_rows(terms):
    return [(int(t["key"]), int(t["count"]), int(t["best_similarity"].view(np.uint32)), int(t["best_pattern"])) for t in terms]


def count_records(rows, keys, n_patterns, n_keys, cap=None):
    """fac_count_records itself: (return value, the terms written)."""
    recs = make_recs(rows)
    karr = np.asarray(keys, dtype=np.uint32) if keys is not None else None
    cap = len(rows) if cap is None else cap
    out = np.zeros(max(cap, 1), dtype=TERM_DTYPE)
    out["key"] = 0xDEAD
    n = _native.lib.fac_count_records(recs.ctypes.data if len(rows) else None, len(rows),
                                      karr.ctypes.data if karr is not None else None, n_patterns, n_keys,
                                      out.ctypes.data, cap)
    return n, out


def check(rows, keys, n_patterns, n_keys):
    n, out = count_records(rows, keys, n_patterns, n_keys)
    want = ref_terms(rows, keys)
    assert n == len(want)
    assert term_rows(out[:n]) == want
    return want


# ---------------------------------------------------------------- layout

def header_struct(name):
    header = open(os.path.join(REPO, "include", "fac.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            m = re.match(r"(.*?)(\w+)$", decl)
            fields.append((m.group(2), m.group(1).strip()))
    return fields


CTYPE = {"float": ctypes.c_float, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}


@pytest.mark.parametrize("name, size", [("fac_term", 16), ("fac_term_total", 16), ("fac_count_args", 80)])
def test_layout_matches_header(name, size):
    fields = header_struct(name)
    struct_ = getattr(_native, name)
    assert [n for n, _ in fields] == [n for n, _ in struct_._fields_]
    at = 0
    align = 1
    for (fname, typ), (_, c) in zip(fields, struct_._fields_):
        want = ctypes.c_void_p if typ.endswith("*") else CTYPE[typ]
        assert ctypes.sizeof(c) == ctypes.sizeof(want), fname
        if not typ.endswith("*"):
            assert c is want, fname
        a = ctypes.alignment(want)
        at = (at + a - 1) // a * a
        assert getattr(struct_, fname).offset == at, fname
        at += ctypes.sizeof(want)
        align = max(align, a)
    assert ctypes.sizeof(struct_) == (at + align - 1) // align * align == size
    if name == "fac_term":
        assert TERM_DTYPE.itemsize == 16 and _native.TERM_BYTES == 16
        assert [(n, TERM_DTYPE.fields[n][1]) for n, _ in fields] == [("key", 0), ("count", 4), ("best_similarity", 8),
                                                                      ("best_pattern", 12)]


def test_tier_constants_equal_the_library_source():
    text = open(os.path.join(REPO, "fuzzy-aho-corasick-rs_amd", "csrc", "fac_internal.h")).read()
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr uint32_t kCount(\w+) = (\d+);", text)}
    assert consts == {"LaneMax": _native.COUNT_LANE_MAX, "GroupMax": _native.COUNT_GROUP_MAX,
                      "HistKeys": _native.COUNT_HIST_KEYS}
    assert consts["GroupMax"] & (consts["GroupMax"] - 1) == 0 and consts["LaneMax"] < 64 < consts["GroupMax"]


def test_entry_points_and_methods_exist():
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ("fac_count_batch", "fac_count_batch_prefiltered", "fac_count_records", "fac_diag_count_terms"):
        assert name in _native.SIGNATURES and hasattr(lib, name), name
    assert hasattr(fac.FuzzyAhoCorasick, "count_batch") and hasattr(fac.Prefiltered, "count_batch")
    assert hasattr(fac.FuzzyReplacer, "count_batch") and hasattr(fac.FuzzyMatches, "term_counts")
    assert hasattr(fac.StagedBatch, "count_records") and hasattr(fac.StagedBatch, "term_matrix")
    assert "TERM_DTYPE" in fac.__all__ and "TermCount" in fac.__all__


# ---------------------------------------------------------------- fac_count_records

ONE = bits_of(1.0)
SIMS = [bits_of(x) for x in (0.5, 0.75, 0.8125, 1.0)]


def test_order_word_is_total_cmp():
    neg_nan, pos_nan = 0xFFC00000, 0x7FC00000
    asc = [neg_nan, bits_of(float("-inf")), bits_of(-1.0), bits_of(-0.0), bits_of(0.0), bits_of(1.0), bits_of(float("inf")),
           pos_nan]
    words = [order_word(b) for b in asc]
    assert words == sorted(words) and len(set(words)) == len(words)


def test_small_shapes():
    assert check([], None, 3, 0) == []
    assert check([], [0, 0, 1], 3, 2) == []
    assert check([(2, ONE)], None, 3, 3) == [(2, 1, ONE, 2)]
    assert check([(2, ONE)], [0, 0, 1], 3, 2) == [(1, 1, ONE, 2)]
    one_key = [(p, SIMS[(p * 5 + i) % 4]) for i, p in enumerate([0, 1, 2, 1, 0, 2, 2])]
    got = check(one_key, [4, 4, 4], 3, 5)
    assert len(got) == 1 and got[0][:2] == (4, 7)
    distinct = [(p, SIMS[p % 4]) for p in (5, 0, 3, 1, 4, 2)]
    assert [t[0] for t in check(distinct, None, 6, 6)] == [0, 1, 2, 3, 4, 5]
    assert [t[0] for t in check(distinct, [5, 4, 3, 2, 1, 0], 6, 6)] == [0, 1, 2, 3, 4, 5]
    many = [(0, SIMS[0]), (1, SIMS[3]), (2, SIMS[1]), (3, SIMS[2]), (4, SIMS[3]), (1, SIMS[0])]
    assert check(many, [0, 0, 1, 2, 0], 5, 3) == [(0, 4, SIMS[3], 1), (1, 1, SIMS[1], 2), (2, 1, SIMS[2], 3)]
    assert check(many, None, 5, 0) == check(many, None, 5, 5)  # n_keys 0 or the pattern count


def test_ties_and_special_values():
    # two patterns with bit-equal best similarity: the least index wins, whatever the order
    for rows in ([(3, SIMS[2]), (1, SIMS[2]), (2, SIMS[0])], [(1, SIMS[2]), (3, SIMS[2])], [(2, SIMS[0]), (3, SIMS[2]), (1, SIMS[2])]):
        assert check(rows, [0, 0, 0, 0], 4, 1)[0][2:] == (SIMS[2], 1)
    # +0.0 is greater than -0.0 under total_cmp although they compare equal as floats
    pz, nz = bits_of(0.0), bits_of(-0.0)
    assert check([(0, nz), (1, pz)], [0, 0], 2, 1) == [(0, 2, pz, 1)]
    assert check([(1, nz), (0, pz)], [0, 0], 2, 1) == [(0, 2, pz, 0)]
    assert check([(0, nz), (1, nz)], [0, 0], 2, 1) == [(0, 2, nz, 0)]
    # a positive NaN is the greatest value of all, a negative one the least
    pos_nan, neg_nan = 0x7FC00000, 0xFFC00000
    assert check([(0, ONE), (1, pos_nan), (2, bits_of(float("inf")))], [0, 0, 0], 3, 1) == [(0, 3, pos_nan, 1)]
    assert check([(0, neg_nan), (1, bits_of(-1.0))], [0, 0], 2, 1) == [(0, 2, bits_of(-1.0), 1)]


def test_errors():
    rows = [(0, ONE), (1, ONE), (2, ONE)]
    n, out = count_records(rows, [0, 2, 1], 3, 2)  # a key >= n_keys, even of a pattern with no record
    assert n == -_native.FAC_E_INVALID and "key" in _native.last_error()
    assert count_records(rows[:1], [0, 2, 1], 3, 2)[0] == -_native.FAC_E_INVALID
    assert count_records(rows, None, 3, 2)[0] == -_native.FAC_E_INVALID  # keys NULL: 0 or the pattern count
    assert count_records(rows, None, 2, 0)[0] == -_native.FAC_E_INVALID  # a pattern_index >= n_patterns
    n, out = count_records(rows, None, 3, 3, cap=2)
    assert n == -_native.FAC_E_OUTPUT_CAPACITY and (out["key"] == 0xDEAD).all()  # nothing written
    n, out = count_records(rows, [0, 0, 1], 3, 2, cap=2)
    assert n == 2 and term_rows(out[:2]) == ref_terms(rows, [0, 0, 1])
    recs = make_recs(rows)
    assert _native.lib.fac_count_records(recs.ctypes.data, 3, None, 3, 3, None, 0) == 3  # count only
    assert _native.lib.fac_count_records(None, 3, None, 3, 3, None, 0) == -_native.FAC_E_INVALID


def test_random_documents():
    rng = random.Random(0x7E4A5)
    keys = [2, 0, 2, 1, 0, 3, 1]
    groups = 0
    for _ in range(2000):
        rows = [(rng.randrange(7), rng.choice(SIMS)) for _ in range(rng.randint(0, 40))]
        groups += len(check(rows, keys, 7, 4))
        check(rows, None, 7, 7)
    assert groups > 4000


# ---------------------------------------------------------------- the Python layer

def test_term_counts_of_hand_built_matches():
    sims = [struct.unpack("<f", struct.pack("<I", b))[0] for b in SIMS]
    spec = [(1, sims[0]), (4, sims[3]), (0, sims[3]), (1, sims[2]), (4, sims[1])]
    ms = FuzzyMatches("x" * 9, [FuzzyMatch(0, 0, 0, 0, 0, p, None, i, i + 1, s, "x") for i, (p, s) in enumerate(spec)])
    assert ms.term_counts() == {0: TermCount(1, sims[3], 0), 1: TermCount(2, sims[2], 1), 4: TermCount(2, sims[3], 4)}
    assert list(ms.term_counts()) == [0, 1, 4]  # ascending key order
    assert ms.term_counts([0, 0, 1, 2, 0], 3) == {0: TermCount(5, sims[3], 0)}
    assert ms.term_counts([7, 7, 1, 2, 3]) == {3: TermCount(2, sims[3], 4), 7: TermCount(3, sims[3], 0)}
    assert FuzzyMatches("", []).term_counts() == {} and FuzzyMatches("", []).term_counts([0, 1], 2) == {}
    with pytest.raises(ValueError):
        ms.term_counts([0, 0, 1, 2, 0], 2)  # key 2 is not below n_keys
    with pytest.raises(ValueError):
        ms.term_counts([0, 0, 1])  # a pattern without a key


def test_replacer_keys():
    keys, forms = FuzzyReplacer.term_keys(["Acme", "Bolt", "Acme", b"Bolt", "acme"])
    assert (keys, forms) == ([0, 1, 0, 1, 2], ["Acme", "Bolt", "acme"])
    assert FuzzyReplacer.term_keys([]) == ([], [])
    pats = [fac.Pattern(p) for p in ("ab", "cd", "ef")]
    keys, forms = FuzzyReplacer.term_keys([None, "ab", Wrap("<", ">")], pats)
    assert (keys, forms) == ([0, 0, 1], ["ab", "<ef>"])
    with pytest.raises(ValueError):
        FuzzyReplacer.term_keys([None, "x"])


def test_key_table_sizes():
    """The key space the Python layer sizes its buffers by is the one the library uses: without a table
    the pattern count, whether n_keys is None, 0 or that count."""
    import types
    from fuzzy_aho_corasick import DeviceError
    from fuzzy_aho_corasick.engine import _key_table
    eng = types.SimpleNamespace(patterns_=["a", "b", "c", "d", "e"])
    for n_keys in (None, 0, 5):
        assert _key_table(eng, None, n_keys) == (None, 5)
    karr, nk = _key_table(eng, [0, 0, 1, 2, 0], None)
    assert karr.dtype == np.uint32 and karr.tolist() == [0, 0, 1, 2, 0] and nk == 3
    assert _key_table(eng, [0, 0, 1, 2, 0], 7)[1] == 7
    for keys, n_keys in ((None, 3), (None, 6), ([0, 0, 1, 2, 0], 2), ([0, 0, 1, 2, 0], 0), ([0, 0, 1, -1, 0], None),
                         ([0, 0, 1, 1 << 32, 0], None), ([0, 0, 1, 2, 0], 1 << 32)):
        with pytest.raises(DeviceError) as ei:
            _key_table(eng, keys, n_keys)
        assert ei.value.code == _native.FAC_E_INVALID, (keys, n_keys)
    with pytest.raises(ValueError):
        _key_table(eng, [0, 1], None)
