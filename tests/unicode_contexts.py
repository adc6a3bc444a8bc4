"""Every Unicode scalar value in a context that makes its properties decide a grapheme boundary.

For a context (pre, post) the text is the line pre + chr(cp) + post + "\\n" for every scalar value cp
(U+0000..U+10FFFF without the surrogates; nothing is sampled). The expected grapheme byte starts and
folded first code points come from the `regex` module's \\X and from str.lower(): the sources the
tables of unicode_data.inc were generated from. Shared by the host and the device tests of the
segmenter and of the folding; on a mismatch the message names the first differing byte, the code
point of the line it lies in and that code point's lookup tier."""
import numpy as np
import regex

N_PLANES = 17
PLANE = 0x10000
DOC_CPS = 64  # code points per document of the batch tests

# (pre, post, what a wrong property of the code point between them changes)
CONTEXTS = [
    ("a", "a", "Extend / ZWJ / SpacingMark join left, Prepend joins right, Control / CR / LF"),
    ("\u1100", "\u11A8", "Hangul L . T: L, V, T, LV, LVT"),
    ("\uAC00", "\u1161", "Hangul LV . V: the other Hangul pairs"),
    ("\U0001F1EB", "\U0001F1EB", "Regional_Indicator parity"),
    ("\U0001F469\u200D", "\u200D\U0001F469", "Extended_Pictographic (GB11), both sides"),
    ("\u0915\u094D", "\u094D\u0915", "InCB Consonant / Linker (GB9c)"),
    ("\u0915", "\u0915", "InCB Linker / Extend between consonants"),
    ("\u0600", "\u0301", "Prepend on the left, Extend on the right"),
]
CONTEXT_IDS = ["a_a", "hangulL_T", "hangulLV_V", "ri_ri", "pict_zwj", "incb_linked", "incb_bare", "prepend_extend"]
assert len(CONTEXTS) == len(CONTEXT_IDS) == 8

_GRAPHEME = regex.compile(r"\X")


def scalar_values(lo=0, hi=0x110000):
    """The scalar values of [lo, hi) as a uint32 array: the surrogates are no scalar values."""
    cps = np.arange(lo, hi, dtype=np.uint32)
    return cps[(cps < 0xD800) | (cps > 0xDFFF)]


ALL_SCALARS = scalar_values()
assert len(ALL_SCALARS) == 1_112_064


def utf8_lengths(cps):
    cps = np.asarray(cps)
    return (1 + (cps >= 0x80) + (cps >= 0x800) + (cps >= 0x10000)).astype(np.int64)


def tier(cp):
    return "below 0x800 (LDS tables)" if cp < 0x800 else "BMP (device tables)" if cp < 0x10000 else "astral (range search)"


_LOWER_FIRST = None


def lower_first_table():
    """ord(chr(cp).lower()[0]) for every code point (the surrogates map to themselves and are never used)."""
    global _LOWER_FIRST
    if _LOWER_FIRST is None:
        t = np.arange(0x110000, dtype=np.uint32)
        for cp in ALL_SCALARS.tolist():
            low = chr(cp).lower()
            if low != chr(cp):
                t[cp] = ord(low[0])
        _LOWER_FIRST = t
    return _LOWER_FIRST


def cased_code_points():
    """The code points whose lowercase differs from them, in order."""
    return [cp for cp in ALL_SCALARS.tolist() if chr(cp).lower() != chr(cp)]


def code_points_of(text):
    return np.frombuffer(text.encode("utf-32-le"), dtype=np.uint32)


def expected(text):
    """(byte start of every \\X cluster of `text`, the cluster's first code point), by regex."""
    cps = code_points_of(text)
    first = np.fromiter((m.start() for m in _GRAPHEME.finditer(text)), dtype=np.int64)
    byte_of = np.zeros(len(cps) + 1, dtype=np.int64)
    np.cumsum(utf8_lengths(cps), out=byte_of[1:])
    return byte_of[first].astype(np.uint64), cps[first]


def folded(first_cps, ci):
    """ord(g[0].lower()[0]) for a case-insensitive engine, ord(g[0]) otherwise."""
    return lower_first_table()[first_cps] if ci else np.asarray(first_cps, dtype=np.uint32)


class ContextText:
    """The lines of one context over `cps`: .text, .data (UTF-8), the code point, the first byte and
    the first character of every line, and (reference=True) the regex expectation .starts / .first of
    the whole text. `bare`: a mask of the lines that have no `pre` (they start a document)."""

    def __init__(self, pre, post, cps=ALL_SCALARS, bare=None, reference=True):
        self.pre, self.post = pre, post
        self.cps = np.asarray(cps, dtype=np.uint32)
        bare = np.zeros(len(self.cps), dtype=bool) if bare is None else np.asarray(bare, dtype=bool)
        tail = post + "\n"
        self.text = "".join(("" if b else pre) + chr(cp) + tail for cp, b in zip(self.cps.tolist(), bare.tolist()))
        self.data = self.text.encode("utf-8")
        lens = utf8_lengths(self.cps) + len(tail.encode("utf-8")) + np.where(bare, 0, len(pre.encode("utf-8")))
        chars = 1 + len(tail) + np.where(bare, 0, len(pre))
        self.line_start = np.zeros(len(lens) + 1, dtype=np.int64)
        np.cumsum(lens, out=self.line_start[1:])
        self.line_char = np.zeros(len(lens) + 1, dtype=np.int64)
        np.cumsum(chars, out=self.line_char[1:])
        assert int(self.line_start[-1]) == len(self.data) and int(self.line_char[-1]) == len(self.text)
        if reference:
            self.starts, self.first = expected(self.text)

    def folds(self, ci):
        return folded(self.first, ci)

    def where(self, byte):
        k = int(np.searchsorted(self.line_start, int(byte), side="right")) - 1
        k = min(max(k, 0), len(self.cps) - 1)
        cp = int(self.cps[k])
        pre = self.pre if len(self.pre) <= 4 else f"{self.pre[:2]}... ({len(self.pre)} code points)"
        return f"byte {int(byte)} in the line of U+{cp:04X}, tier {tier(cp)}, context {pre!r} . {self.post!r}"


class BatchText(ContextText):
    """The same lines cut into documents: one per DOC_CPS consecutive code points (the surrogates'
    32 empty ranges give none), the first document of every plane starting on the code point itself,
    then one document chr(cp) + post + "\\n" per code point of `alone`. The reference is regex \\X on
    every document alone: .doc_byte (n_docs + 1 offsets), .doc_count, .doc_ascii, and .starts
    (document-relative) / .first of all documents' graphemes one after another (.doc_first: each
    document's slice). An ASCII document's graphemes are its bytes (search.rs:196)."""

    def __init__(self, pre, post, alone=()):
        alone = np.asarray(sorted(alone), dtype=np.uint32)
        cps = np.concatenate([ALL_SCALARS, alone])
        bare = np.concatenate([ALL_SCALARS % PLANE == 0, np.ones(len(alone), dtype=bool)])
        super().__init__(pre, post, cps, bare, reference=False)
        n_main = len(ALL_SCALARS)
        block = ALL_SCALARS // DOC_CPS
        first_line = np.concatenate([[0], np.flatnonzero(np.diff(block)) + 1, np.arange(n_main, len(cps) + 1)])
        self.doc_line = first_line
        self.n_docs = len(first_line) - 1
        self.doc_byte = self.line_start[first_line].astype(np.uint64)
        doc_char = self.line_char[first_line].tolist()
        docs = [self.text[a:b] for a, b in zip(doc_char, doc_char[1:])]
        self.doc_ascii = np.array([d.isascii() for d in docs], dtype=bool)

        def cluster_starts():
            for off, doc in zip(doc_char, docs):
                if doc.isascii():
                    yield from range(off, off + len(doc))
                else:
                    for m in _GRAPHEME.finditer(doc):
                        yield off + m.start()
        first = np.fromiter(cluster_starts(), dtype=np.int64)
        all_cps = code_points_of(self.text)
        byte_of = np.zeros(len(all_cps) + 1, dtype=np.int64)
        np.cumsum(utf8_lengths(all_cps), out=byte_of[1:])
        self.doc_first = np.searchsorted(first, np.asarray(doc_char, dtype=np.int64), side="left")
        self.doc_count = np.diff(self.doc_first)
        doc_of = np.repeat(np.arange(self.n_docs), self.doc_count)
        self.starts = (byte_of[first] - self.doc_byte[doc_of].astype(np.int64)).astype(np.uint64)
        self.first = all_cps[first]

    def where_doc(self, d, rel_byte=0):
        return f"document {d}: " + self.where(int(self.doc_byte[d]) + int(rel_byte))


def first_difference(got, want):
    """Index of the first entry at which two arrays differ (a missing entry differs), or None."""
    got, want = np.asarray(got), np.asarray(want)
    n = min(len(got), len(want))
    ne = np.flatnonzero(got[:n] != want[:n])
    if len(ne):
        return int(ne[0])
    return None if len(got) == len(want) else n


def check_starts(ctx, got, want=None):
    want = ctx.starts if want is None else want
    i = first_difference(got, want)
    if i is None:
        return
    g = int(got[i]) if i < len(got) else None
    w = int(want[i]) if i < len(want) else None
    byte = min(x for x in (g, w) if x is not None)
    raise AssertionError(f"grapheme starts differ at index {i}: got {g}, expected {w} "
                         f"({len(got)} against {len(want)} graphemes): first differing {ctx.where(byte)}")


def check_chars(ctx, got, want, starts=None):
    starts = ctx.starts if starts is None else starts
    i = first_difference(got, want)
    if i is None:
        return
    g = f"U+{int(got[i]):04X}" if i < len(got) else None
    w = f"U+{int(want[i]):04X}" if i < len(want) else None
    byte = int(starts[min(i, len(starts) - 1)])
    raise AssertionError(f"folded characters differ at grapheme {i}: got {g}, expected {w} "
                         f"({len(got)} against {len(want)} graphemes): {ctx.where(byte)}")


# ---------------------------------------------------------------- property classes

_GCB = ["Other", "CR", "LF", "Control", "Extend", "ZWJ", "Regional_Indicator", "Prepend", "SpacingMark", "L", "V", "T",
        "LV", "LVT"]
_INCB = ["None", "Linker", "Consonant", "Extend"]


def property_triples():
    """(GCB, Extended_Pictographic, InCB) of every code point as three uint8 arrays, from regex."""
    chars = "".join(map(chr, ALL_SCALARS.tolist()))
    g = np.zeros(0x110000, dtype=np.uint8)
    p = np.zeros(0x110000, dtype=np.uint8)
    ib = np.zeros(0x110000, dtype=np.uint8)
    for k, name in enumerate(_GCB[1:], 1):
        g[[ord(c) for c in regex.findall(r"\p{Grapheme_Cluster_Break=%s}" % name, chars)]] = k
    p[[ord(c) for c in regex.findall(r"\p{Extended_Pictographic}", chars)]] = 1
    for k, name in enumerate(_INCB[1:], 1):
        ib[[ord(c) for c in regex.findall(r"\p{Indic_Conjunct_Break=%s}" % name, chars)]] = k
    return g, p, ib


def class_representatives():
    """The lowest and the highest code point of every (GCB, ExtPict, InCB) triple in every tier."""
    g, p, ib = property_triples()
    key = (g.astype(np.int64) << 8) | (p.astype(np.int64) << 4) | ib
    out = set()
    for lo, hi in ((0, 0x800), (0x800, 0x10000), (0x10000, 0x110000)):
        cps = scalar_values(lo, hi)
        k = key[cps]
        for v in np.unique(k).tolist():
            members = cps[k == v]
            out.add(int(members[0]))
            out.add(int(members[-1]))
    return sorted(out)
