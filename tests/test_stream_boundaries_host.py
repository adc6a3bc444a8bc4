"""Whole-token matches in streams, host side (fac.h fac_stream_open_opts): the rule
with left context, fac_boundary_ok_after(before, utf8), against test_boundaries_host.ref_ok on the
concatenation before + utf8. With the whole earlier text as prefix ref_ok is exactly the stream rule;
the reference never calls fac_boundary_*."""
import pytest

from fuzzy_aho_corasick import _native
from test_boundaries_host import Rng, random_doc, ref_ok

CARRY = 128  # bytes of left context a stream task carries: 4 bytes x 32 code points
SIDES = (0, 1, 2, 3)
INVALID = -_native.FAC_E_INVALID


def ok_after(before: bytes, more: bool, text: bytes, start: int, end: int, sides: int) -> int:
    return int(_native.lib.fac_boundary_ok_after(before, len(before), int(more), text, len(text), start, end, sides))


def char_starts(data: bytes):
    return [i for i in range(len(data)) if data[i] & 0xC0 != 0x80] + [len(data)]


def spans(text: bytes, limit=6):
    """Spans of the window text on code-point boundaries: those that start at its first bytes (where
    the walk enters the context at once or after a few code points), and a few that end at its end."""
    cs = char_starts(text)
    out = [(s, e) for s in cs[:limit] for e in cs if s <= e][:4 * limit]
    return out + [(s, cs[-1]) for s in cs[-3:]]


def check_cut(data: bytes, cut: int, truncate: bool):
    text, before, more = data[cut:], data[:cut], False
    if truncate and len(before) > CARRY:
        before, more = before[-CARRY:], True
    for s, e in spans(text):
        for sides in SIDES:
            want = int(ref_ok(data, cut + s, cut + e, sides))
            assert ok_after(before, more, text, s, e, sides) == want, (cut, s, e, sides, truncate)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_documents_cut_at_every_code_point(seed):
    """Every cut of a random document: the full prefix with more_before = 0 (the context's front is
    the stream's start), and its last 128 bytes with more_before = 1. The truncated front lies inside
    a code point for many cuts; the results are the same."""
    rng = Rng(0x9E3779B97F4A7C15 ^ seed)
    data = random_doc(rng, 260).encode("utf-8")
    cuts = char_starts(data)
    inside = 0
    for cut in cuts:
        check_cut(data, cut, truncate=False)
        check_cut(data, cut, truncate=True)
        inside += int(cut > CARRY and data[cut - CARRY] & 0xC0 == 0x80)
    assert inside >= 20 and len(data) > 3 * CARRY


@pytest.mark.parametrize("mark", ["\u0301", "\U000e0100"], ids=["2-byte", "4-byte"])
@pytest.mark.parametrize("k", [0, 1, 31, 32, 33])
@pytest.mark.parametrize("lead", ["a", " ", "é", "、"])
def test_transparent_runs_straddling_the_cut(lead, k, mark):
    """lead + k transparent code points + "art": the cut at every code point of the run, so that the
    run lies before the window, inside it, or on both sides. 32 marks of 4 bytes fill the 128-byte
    context exactly; with 33 the walk ends at its bound."""
    filler = "zz é\U0001d49c" * 30  # more than 128 bytes, so that the truncated context has text before it
    data = (filler + lead + mark * k + "art").encode("utf-8")
    head = len((filler + lead).encode("utf-8"))
    run_end = len(data) - 3
    for cut in [c for c in char_starts(data) if head - len(lead.encode("utf-8")) <= c <= run_end]:
        for truncate in (False, True):
            text, before, more = data[cut:], data[:cut], False
            if truncate:
                before, more = before[-CARRY:], len(before) > CARRY
            s = run_end - cut
            for sides in SIDES:
                want = int(ref_ok(data, run_end, len(data), sides))
                assert ok_after(before, more, text, s, s + 3, sides) == want, (cut, sides, truncate)
    # what the rule says here: a letter before at most 31 marks is seen, 32 marks hide it
    assert ref_ok(data, run_end, len(data), 1) == (not lead.isalnum() or k >= 32)


def test_stream_start():
    """more_before = 0: the front of the context (or of the text, without one) is a boundary."""
    for before, text in ((b"", b"art"), (b"", "\u0301art".encode()), ("\u0301\u0301".encode(), b"art"),
                         (b"", b""), ("\u0301".encode() * 20, "\u0301art".encode())):
        s = len(text) - 3 if text else 0
        assert ok_after(before, False, text, s, len(text), 3) == 1
        assert int(ref_ok(before + text, len(before) + s, len(before) + len(text), 3)) == 1
    assert ok_after(b"x", False, b"art", 0, 3, 1) == 0
    assert ok_after(b"x ", False, b"art", 0, 3, 1) == 1
    assert ok_after(b"", False, b"art7", 0, 3, 2) == 0 and ok_after(b"", False, b"art7", 0, 3, 1) == 1


def test_error_returns():
    f = _native.lib.fac_boundary_ok_after
    assert f(None, 0, 0, b"art", 3, 0, 3, 3) == 1
    assert f(None, 1, 0, b"art", 3, 0, 3, 3) == INVALID  # NULL context with a length
    assert f(b"x", 1, 0, None, 3, 0, 3, 3) == INVALID    # NULL text with a length
    assert f(b"x", 1, 0, None, 0, 0, 0, 3) == 0          # an empty text needs no pointer
    for sides in (-1, 4, 7):
        assert f(b"x", 1, 0, b"art", 3, 0, 3, sides) == INVALID
    assert f(b"x", 1, 0, b"art", 3, 2, 1, 3) == INVALID  # start > end
    assert f(b"x", 1, 0, b"art", 3, 0, 4, 3) == INVALID  # end > len
    text = "aé\U0001d49cb".encode()
    for off in (2, 4, 5, 6):  # inside a code point
        assert f(b"", 0, 0, text, len(text), off, len(text), 3) == INVALID
        assert f(b"", 0, 0, text, len(text), 0, off, 3) == INVALID
    # the undecided short context: the walk reaches the front of a context that has text before it
    marks = "\u0301".encode()
    assert ok_after(b"", True, b"art", 0, 3, 1) == INVALID
    assert ok_after(marks * 5, True, b"art", 0, 3, 1) == INVALID
    assert ok_after(marks * 5, False, b"art", 0, 3, 1) == 1
    assert ok_after(marks[1:] + marks * 4, True, b"art", 0, 3, 1) == INVALID  # a front inside a code point
    assert ok_after(b"a" + marks * 5, True, b"art", 0, 3, 1) == 0             # decided before the front
    assert ok_after(marks * 5, True, b"art", 0, 3, 2) == 1                     # the end side needs no context
    assert ok_after(marks[1:] + marks * 31, True, b"art", 0, 3, 1) == INVALID  # 63 bytes: 31 marks and a tail
    assert ok_after(marks * 32, True, b"art", 0, 3, 1) == 1                    # the bound of 32 decides
    assert b"context" in _native.lib.fac_last_error()
