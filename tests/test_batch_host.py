"""Host-side pieces of the batch path (no GPU): the offsets helper, the ctypes layout of
fac_batch_args against the header's field list, and the bound entry points."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BATCH_NAMES = ["fac_batch_stage", "fac_batch_stage_device", "fac_batch_free", "fac_batch_docs",
               "fac_batch_doc_graphemes", "fac_batch_grapheme_starts", "fac_batch_text_chars",
               "fac_haystack_text_chars", "fac_search_batch"]


def test_batch_offsets_round_trips():
    from fuzzy_aho_corasick import batch_offsets
    docs = [b"abc", b"", "é\r\n".encode(), bytearray(b"xy"), memoryview(b"z"), b""]
    data, off = batch_offsets(docs)
    assert off[0] == 0 and off[-1] == len(data) and len(off) == len(docs) + 1
    assert all(a <= b for a, b in zip(off, off[1:]))
    assert [data[off[d]:off[d + 1]] for d in range(len(docs))] == [bytes(d) for d in docs]
    assert batch_offsets([]) == (b"", [0])


@pytest.mark.parametrize("bad", ["text", 3, None, ["a"]])
def test_batch_offsets_rejects_non_bytes(bad):
    from fuzzy_aho_corasick import batch_offsets
    with pytest.raises(TypeError):
        batch_offsets([b"ok", bad])


def test_batch_args_layout_matches_header():
    """The Python fac_batch_args has the header's fields, in order, with the header's C types."""
    from fuzzy_aho_corasick import _native
    header = open(os.path.join(REPO, "include", "fac.h")).read()
    body = re.search(r"typedef struct fac_batch_args \{(.*?)\} fac_batch_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            m = re.match(r"(.*?)(\w+)$", decl)
            fields.append((m.group(2), m.group(1).strip()))
    ctype = {"float": ctypes.c_float, "int32_t": ctypes.c_int32, "uint64_t": ctypes.c_uint64}
    size = 0
    align = 1
    for name, typ in fields:
        c = ctypes.c_void_p if typ.endswith("*") else ctype[typ]
        a = ctypes.alignment(c)
        size = (size + a - 1) // a * a + ctypes.sizeof(c)
        align = max(align, a)
    size = (size + align - 1) // align * align
    assert [n for n, _ in fields] == [n for n, _ in _native.fac_batch_args._fields_]
    assert ctypes.sizeof(_native.fac_batch_args) == size == 56
    for (name, typ), (_, c) in zip(fields, _native.fac_batch_args._fields_):
        want = ctypes.sizeof(ctypes.c_void_p) if typ.endswith("*") else ctypes.sizeof(ctype[typ])
        assert ctypes.sizeof(c) == want, name


def test_batch_entry_points_are_bound():
    from fuzzy_aho_corasick import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in BATCH_NAMES:
        assert name in _native.SIGNATURES, name
        assert hasattr(lib, name), name
    import fuzzy_aho_corasick as fac
    assert hasattr(fac.FuzzyAhoCorasick, "search_batch")
    for meth in ("from_device", "search_records", "doc_graphemes", "grapheme_starts", "grapheme_starts_into",
                 "text_chars"):
        assert hasattr(fac.StagedBatch, meth), meth
    for meth in ("grapheme_starts", "text_chars"):
        assert hasattr(fac.StagedHaystack, meth), meth
