"""Pre-filtered batches, the parts that need no GPU: the three entry points are exported, declared
in the header and bound, the Python surface exists, and NULL arguments are refused before any device
is touched."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fac_search_batch_prefiltered", "fac_replace_batch_prefiltered", "fac_batch_prefilter_windows"]


def test_entry_points_are_exported_declared_and_bound():
    from fuzzy_aho_corasick import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    header = open(os.path.join(REPO, "include", "fac.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES, name
        assert re.search(r"\b%s\(" % name, header), name
    # the pre-filtered calls take exactly the plain calls' arguments
    assert _native.SIGNATURES["fac_search_batch_prefiltered"] == _native.SIGNATURES["fac_search_batch"]
    assert _native.SIGNATURES["fac_replace_batch_prefiltered"] == _native.SIGNATURES["fac_replace_batch"]
    assert "pre-filtered batches and multi-GPU batches are not" not in header


def test_python_surface():
    import inspect

    import fuzzy_aho_corasick as fac
    for meth in ("search_records", "replace_bytes"):
        p = inspect.signature(getattr(fac.StagedBatch, meth)).parameters
        assert "prefilter" in p and p["prefilter"].default is False, meth  # the default keeps the plain call
    assert hasattr(fac.StagedBatch, "prefilter_windows")
    assert hasattr(fac.Prefiltered, "search_batch") and hasattr(fac.Prefiltered, "replace_batch")


@pytest.mark.parametrize("null", ["engine", "batch", "args", "n_out", "out"])
def test_search_null_arguments(null):
    """FAC_E_INVALID before anything else is looked at: the other handles are dummies that a call
    which went any further would have to dereference (there is no device here to touch)."""
    from fuzzy_aho_corasick import _native
    dummy = ctypes.c_void_p(0x10)
    args = _native.fac_batch_args()
    out = ctypes.POINTER(_native.fac_match)()
    n = ctypes.c_uint64(7)
    a = {"engine": dummy, "batch": dummy, "args": ctypes.byref(args), "out": ctypes.byref(out), "n_out": ctypes.byref(n)}
    a[null] = None
    rc = _native.lib.fac_search_batch_prefiltered(a["engine"], a["batch"], a["args"], a["out"], a["n_out"], None, None)
    assert rc == _native.FAC_E_INVALID
    assert "NULL" in _native.last_error()
    assert n.value == 7 and not out  # nothing written


@pytest.mark.parametrize("null", ["engine", "batch", "table", "args", "out_len", "out"])
def test_replace_null_arguments(null):
    from fuzzy_aho_corasick import _native
    dummy = ctypes.c_void_p(0x10)
    args = _native.fac_replace_args()
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_uint64(7)
    a = {"engine": dummy, "batch": dummy, "table": dummy, "args": ctypes.byref(args), "out": ctypes.byref(out),
         "out_len": ctypes.byref(n)}
    a[null] = None
    rc = _native.lib.fac_replace_batch_prefiltered(a["engine"], a["batch"], a["table"], a["args"], a["out"], a["out_len"],
                                                   None, None, None)
    assert rc == _native.FAC_E_INVALID
    assert n.value == 7 and not out


@pytest.mark.parametrize("null", ["engine", "batch", "out"])
def test_windows_null_arguments(null):
    """The diagnostics entry returns minus the error code (-1 is the reference's fallback)."""
    from fuzzy_aho_corasick import _native
    dummy = ctypes.c_void_p(0x10)
    buf = (ctypes.c_uint64 * 3)()
    a = {"engine": dummy, "batch": dummy, "out": buf}
    a[null] = None
    rc = _native.lib.fac_batch_prefilter_windows(a["engine"], a["batch"], 0.8, None, a["out"], 1)
    assert rc == -_native.FAC_E_INVALID
