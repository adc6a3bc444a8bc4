"""Whole-token matches, host side (fac.h fac_batch_require_boundaries): the class table
(fac_boundary_class), the host restatement of the rule (fac_boundary_ok) and
FuzzyMatches.retain_boundaries, against a reference of the rule written here from the `regex`
module's properties. The reference never calls fac_boundary_*; test_gpu_boundaries.py imports it."""
import functools

import pytest
import regex

from fuzzy_aho_corasick import Boundary, FuzzyAhoCorasickBuilder as B, FuzzyLimits as L, FuzzyMatches, _native
from oracle_harness import OracleEngine, graphemes

ALNUM, TRANSPARENT = 1, 2
MAX_SKIP = 32  # transparent code points the start side walks over before it calls the side a boundary


@functools.lru_cache(maxsize=None)
def ref_classes() -> bytes:
    """Class of every code point: ALNUM = Rust's char::is_alphanumeric (Alphabetic, or
    General_Category Nd / Nl / No), TRANSPARENT = General_Category M* and not alphanumeric, else 0
    (surrogates included)."""
    every = "".join(chr(c) for c in range(0x110000) if not 0xD800 <= c <= 0xDFFF)
    out = bytearray(0x110000)
    for ch in regex.findall(r"\p{M}", every):
        out[ord(ch)] = TRANSPARENT
    for ch in regex.findall(r"[\p{Alphabetic}\p{Nd}\p{Nl}\p{No}]", every):
        out[ord(ch)] = ALNUM
    return bytes(out)


def ref_ok(data: bytes, start: int, end: int, sides: int) -> bool:
    """The rule of DESIGN.md 6a "Whole-token matches" on one document's bytes."""
    cls = ref_classes()
    if sides & 2 and end < len(data):
        if cls[ord(data[end:].decode("utf-8")[0])] == ALNUM:
            return False
    if sides & 1:
        skipped = 0
        for ch in reversed(data[:start].decode("utf-8")):
            c = cls[ord(ch)]
            if c != TRANSPARENT:
                return c != ALNUM
            skipped += 1
            if skipped == MAX_SKIP:
                break
    return True


def lib_ok(data: bytes, start: int, end: int, sides: int) -> int:
    return int(_native.lib.fac_boundary_ok(data, len(data), start, end, sides))


class Rng:  # the xorshift of the parity tests (prefilter.rs:441-452)
    def __init__(self, s):
        self.s = s

    def next(self):
        x = self.s
        x ^= (x << 13) & 0xFFFFFFFFFFFFFFFF
        x ^= x >> 7
        x ^= (x << 17) & 0xFFFFFFFFFFFFFFFF
        self.s = x
        return x


# test_gpu_batch.py _fill's pieces, plus '_', digits, a No digit, a combining accent, an alphabetic
# spacing mark, a variation selector, ZWJ and a 4-byte letter
PIECES = ["a", "\u00e9", "\u0915", "\U0001f600", " ", "\u0301", "b", "\u03c9", "\r\n", "\U0001f1eb", "\u200d",
          "_", "7", "0", "\u00b2", "\u0301", "\u093e", "\ufe0f", "\u200d", "\U0001d49c", "-"]


def random_doc(rng, n_pieces):
    return "".join(PIECES[rng.next() % len(PIECES)] for _ in range(n_pieces))


def grapheme_starts(text: str):
    out, pos = [], 0
    for g in graphemes(text):
        out.append(pos)
        pos += len(g.encode("utf-8"))
    return out + [pos]


def test_class_of_every_code_point():
    want = ref_classes()
    f = _native.lib.fac_boundary_class
    bad = [hex(cp) for cp in range(0x110000) if f(cp) != want[cp]]
    assert not bad, bad[:20]
    assert [f(cp) for cp in (0xD800, 0xDFFF, 0x110000, 0xFFFFFFFF)] == [0, 0, 0, 0]
    # the cases the rule names
    assert [f(ord(c)) for c in "_-\u00b2\u2160\u093e\u0301\ufe0f\u200d a9"] == [0, 0, 1, 1, 1, 2, 2, 0, 0, 1, 1]


def test_boundary_ok_on_random_documents():
    rng = Rng(0xB0DA41E5)
    checked = 0
    for k in range(48):
        data = random_doc(rng, 4 + rng.next() % 20).encode("utf-8")
        cuts = grapheme_starts(data.decode("utf-8"))
        for i, s in enumerate(cuts):
            for e in cuts[i:]:
                for sides in range(4):
                    assert lib_ok(data, s, e, sides) == int(ref_ok(data, s, e, sides)), (data, s, e, sides)
                    checked += 1
    assert checked > 10000


@pytest.mark.parametrize("marks", [0, 1, 31, 32, 33])
def test_transparent_run_lengths(marks):
    run = "\u0301" * marks
    for before, start_ok in (("a", marks >= MAX_SKIP), (" ", True), ("", True)):
        data = (before + run + "ab c").encode("utf-8")
        s = len((before + run).encode("utf-8"))
        assert ref_ok(data, s, s + 2, 1) == start_ok
        for sides, want in ((0, True), (1, start_ok), (2, True), (3, start_ok)):
            assert lib_ok(data, s, s + 2, sides) == int(want), (before, marks, sides)
    # a mixed run of transparent code points counts the same way as a uniform one
    mixed = ("a" + "\u0301\ufe0f" * (marks // 2) + "\u20dd" * (marks % 2) + "ab").encode("utf-8")
    s = len(mixed) - 2
    assert lib_ok(mixed, s, s + 2, 1) == int(ref_ok(mixed, s, s + 2, 1)) == int(marks >= MAX_SKIP)


def test_error_returns():
    data = "a\u00e9\U0001d49cb".encode("utf-8")  # 1 + 2 + 4 + 1 bytes
    inv = -_native.FAC_E_INVALID
    assert lib_ok(data, 0, 1, 3) == 0 and lib_ok(data, 0, len(data), 3) == 1
    assert lib_ok(data, 2, 1, 3) == inv          # start > end
    assert lib_ok(data, 0, len(data) + 1, 3) == inv  # end outside the text
    assert lib_ok(data, 2, 3, 3) == inv          # start inside a code point
    assert lib_ok(data, 1, 5, 3) == inv          # end inside a code point
    assert lib_ok(data, 0, 1, 4) == inv and lib_ok(data, 0, 1, -1) == inv
    assert int(_native.lib.fac_boundary_ok(None, 3, 0, 1, 3)) == inv
    assert int(_native.lib.fac_boundary_ok(None, 0, 0, 0, 3)) == 1  # the empty text: both sides are its ends
    assert "boundary" in _native.last_error() or "argument" in _native.last_error()


def test_require_boundaries_checks_its_arguments():
    f = _native.lib.fac_batch_require_boundaries
    assert f(None, 3) == _native.FAC_E_INVALID
    assert f(None, 4) == _native.FAC_E_INVALID
    assert [int(b) for b in (Boundary.NONE, Boundary.START, Boundary.END, Boundary.WHOLE)] == [0, 1, 2, 3]
    assert Boundary.START | Boundary.END == Boundary.WHOLE
    assert (_native.FAC_BOUNDARY_START, _native.FAC_BOUNDARY_END, _native.FAC_BOUNDARY_WHOLE) == (1, 2, 3)


WORDS = ["art", "party", "cart", "art-house", "caf\u00e9", "cafe\u0301bar", "\u00b2art", "art_", "\u0915\u093eart", "start",
         "Art", "9art", "art\ufe0f", "\U0001d49cart", "bar", "a"]


def test_retain_boundaries_is_the_predicate():
    b = B().fuzzy(L().edits(1)).case_insensitive(True)
    pats = ["art", "bar", "caf\u00e9"]
    orc = OracleEngine(b, pats)
    rng = Rng(0x7E7A1)
    seen = set()
    for _ in range(24):
        sep = [" ", "", ", ", "\u0301", "_"]
        doc = "".join(WORDS[rng.next() % len(WORDS)] + sep[rng.next() % len(sep)] for _ in range(1 + rng.next() % 6))
        raw = orc.search_raw(doc, 0.6)
        data = doc.encode("utf-8")
        for sides in (Boundary.NONE, Boundary.START, Boundary.END, Boundary.WHOLE):
            want = [m.key() for m in raw if ref_ok(data, m.start, m.end, int(sides))]
            got = FuzzyMatches(doc, list(raw.inner), data).retain_boundaries(sides)
            assert [m.key() for m in got] == want, (doc, sides)
            seen.add((int(sides), len(want) < len(raw.inner)))
    assert {(1, True), (2, True), (3, True), (0, False)} <= seen and (0, True) not in seen
    with pytest.raises(ValueError):
        FuzzyMatches("a", [], b"a").retain_boundaries(4)
