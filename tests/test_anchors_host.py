"""Anchored matches, the parts that need no device (fac.h "Anchored matches"): fac_anchor_ok against
the test's own two-line predicate over every span of documents of 0..4 bytes and every mask, the
argument errors of fac_batch_require_anchors and fac_lookup_batch that are decided before any device
call, and the Anchor enum against the header's constants."""
import ctypes
import os
import re

import pytest

from fuzzy_aho_corasick import Anchor, FuzzyMatch, FuzzyMatches, _native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def anchored(doc_len, start, end, sides):
    """The rule: start == 0 if START is requested, end == the document's length if END is."""
    return (not sides & 1 or start == 0) and (not sides & 2 or end == doc_len)


def test_anchor_ok_every_span_and_mask():
    kept = dropped = 0
    for n in range(5):
        for start in range(n + 1):
            for end in range(start, n + 1):
                for sides in range(4):
                    got = _native.lib.fac_anchor_ok(n, start, end, sides)
                    assert got == int(anchored(n, start, end, sides)), (n, start, end, sides)
                    kept += got
                    dropped += 1 - got
    assert kept > 0 and dropped > 0
    # the empty span follows the same rule: at byte 0 it starts the document, at byte n it ends it
    assert _native.lib.fac_anchor_ok(0, 0, 0, 3) == 1
    assert _native.lib.fac_anchor_ok(3, 0, 0, 1) == 1 and _native.lib.fac_anchor_ok(3, 0, 0, 2) == 0
    assert _native.lib.fac_anchor_ok(3, 3, 3, 2) == 1 and _native.lib.fac_anchor_ok(3, 3, 3, 1) == 0
    # offsets are plain 64-bit bytes
    big = (1 << 40) - 1
    assert _native.lib.fac_anchor_ok(big, 0, big, 3) == 1 and _native.lib.fac_anchor_ok(big, 0, big - 1, 3) == 0


@pytest.mark.parametrize("args", [(4, 0, 4, 4), (4, 0, 4, -1), (4, 0, 4, 7), (4, 3, 2, 0), (4, 3, 2, 3), (4, 0, 5, 0),
                                  (4, 5, 5, 1), (0, 0, 1, 2)])
def test_anchor_ok_errors(args):
    assert _native.lib.fac_anchor_ok(*args) == -_native.FAC_E_INVALID
    assert _native.last_error()


def test_require_anchors_argument_errors():
    for sides in (0, 1, 2, 3, 4, -1):
        assert _native.lib.fac_batch_require_anchors(None, sides) == _native.FAC_E_INVALID  # NULL first


def test_lookup_argument_errors():
    a = _native.fac_lookup_args()
    a.threshold, a.order, a.k = 0.5, 1, 1
    out = ctypes.POINTER(_native.fac_match)()
    lookup = _native.lib.fac_lookup_batch
    assert lookup(None, None, None, ctypes.byref(out), None, None) == _native.FAC_E_INVALID
    assert lookup(None, None, ctypes.byref(a), ctypes.byref(out), None, None) == _native.FAC_E_INVALID
    assert "NULL" in _native.last_error()
    a.k = 0  # decided before the handles are looked at
    assert lookup(None, None, ctypes.byref(a), ctypes.byref(out), None, None) == _native.FAC_E_INVALID
    assert "k must be" in _native.last_error()
    a.k, a.order = 1, 4
    assert lookup(None, None, ctypes.byref(a), ctypes.byref(out), None, None) == _native.FAC_E_INVALID
    assert "order" in _native.last_error()
    assert not out


def test_enum_equals_the_header():
    text = open(os.path.join(REPO, "include", "fac.h"), encoding="utf-8").read()
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define FAC_ANCHOR_(\w+) (\d+)$", text, re.M)}
    assert consts == {"START": 1, "END": 2, "WHOLE": 3}
    assert (int(Anchor.NONE), int(Anchor.START), int(Anchor.END), int(Anchor.WHOLE)) == (0, 1, 2, 3)
    assert Anchor.START | Anchor.END == Anchor.WHOLE
    assert (_native.FAC_ANCHOR_START, _native.FAC_ANCHOR_END, _native.FAC_ANCHOR_WHOLE) == (1, 2, 3)
    assert ctypes.sizeof(_native.fac_lookup_args) == 40  # float, int32, uint32, pad, two pointers, uint64


def test_retain_anchors_on_the_host():
    doc = "héllo"
    data = doc.encode("utf-8")
    spans = [(s, e) for s in range(len(data) + 1) for e in range(s, len(data) + 1)
             if (s == len(data) or data[s] & 0xC0 != 0x80) and (e == len(data) or data[e] & 0xC0 != 0x80)]
    for sides in Anchor:
        ms = FuzzyMatches(doc, [FuzzyMatch(0, 0, 0, 0, 0, 0, None, s, e, 1.0, data[s:e].decode()) for s, e in spans], data)
        kept = [(m.start, m.end) for m in ms.retain_anchors(sides)]
        assert kept == [(s, e) for s, e in spans if anchored(len(data), s, e, int(sides))]
    with pytest.raises(ValueError):
        FuzzyMatches(doc, [], data).retain_anchors(4)
