"""Batched replace, the parts that need no GPU: the entry points are bound and exported, the Python
fac_replace_args mirrors the header, and the pure table helper round-trips."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLACE_NAMES = ["fac_replacements_create", "fac_replacements_free", "fac_replace_batch"]


def test_replace_entry_points_are_bound():
    from fuzzy_aho_corasick import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in REPLACE_NAMES:
        assert name in _native.SIGNATURES, name
        assert hasattr(lib, name), name
    import fuzzy_aho_corasick as fac
    assert hasattr(fac.FuzzyAhoCorasick, "replace_batch")
    assert hasattr(fac.FuzzyReplacer, "replace_batch")
    assert hasattr(fac.StagedBatch, "replace_bytes")
    assert hasattr(fac, "ReplacementTable") and hasattr(fac, "replacement_table")
    header = open(os.path.join(REPO, "include", "fac.h")).read()
    for name in REPLACE_NAMES:
        assert re.search(r"\b%s\(" % name, header), name


def test_replace_args_layout_matches_header():
    """The Python fac_replace_args has the header's fields, in order, with the header's C types."""
    from fuzzy_aho_corasick import _native
    header = open(os.path.join(REPO, "include", "fac.h")).read()
    body = re.search(r"typedef struct fac_replace_args \{(.*?)\} fac_replace_args;", header, re.S).group(1)
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
    offsets = {}
    for name, typ in fields:
        c = ctypes.c_void_p if typ.endswith("*") else ctype[typ]
        a = ctypes.alignment(c)
        offsets[name] = (size + a - 1) // a * a
        size = offsets[name] + ctypes.sizeof(c)
        align = max(align, a)
    size = (size + align - 1) // align * align
    assert [n for n, _ in fields] == [n for n, _ in _native.fac_replace_args._fields_]
    assert [n for n, _ in fields] == ["threshold", "order", "overlap", "unique_ids", "stream", "device_out",
                                      "device_cap", "device_out_offsets"]
    assert ctypes.sizeof(_native.fac_replace_args) == size == 56
    for (name, typ), (_, c) in zip(fields, _native.fac_replace_args._fields_):
        want = ctypes.sizeof(ctypes.c_void_p) if typ.endswith("*") else ctypes.sizeof(ctype[typ])
        assert ctypes.sizeof(c) == want, name
        assert getattr(_native.fac_replace_args, name).offset == offsets[name], name


@pytest.mark.parametrize("reps", [
    [],
    ["x"],
    [None],
    ["", None, ""],
    ["PJSC", "", None, "«é»", "😀", "a" * 20, None, "\0"],
])
def test_replacement_table_round_trips(reps):
    from fuzzy_aho_corasick import replacement_table
    data, offsets, keep = replacement_table(reps)
    assert isinstance(data, bytes) and isinstance(keep, bytes)
    assert len(offsets) == len(reps) + 1 and offsets[0] == 0 and offsets[-1] == len(data) and len(keep) == len(reps)
    assert all(a <= b for a, b in zip(offsets, offsets[1:]))
    back = [None if keep[p] else data[offsets[p]:offsets[p + 1]].decode("utf-8") for p in range(len(reps))]
    assert back == reps
    assert all(offsets[p] == offsets[p + 1] for p in range(len(reps)) if keep[p])  # "keep" holds no bytes


def test_replacement_table_takes_bytes_and_rejects_other_types():
    from fuzzy_aho_corasick import replacement_table
    assert replacement_table([b"\xff", "é"]) == (b"\xff\xc3\xa9", [0, 1, 3], b"\0\0")  # validated by the library
    with pytest.raises(TypeError):
        replacement_table(["a", 3])
