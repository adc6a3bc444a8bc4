"""The documents of the pre-filtered batches that hold non-ASCII documents (tests
test_gpu_batch_prefilter_unicode.py on the device, test_batch_prefilter_unicode_host.py on the
oracle alone): engines, batches and helpers, pure Python. A "symbol" is a byte of an ASCII document
and a grapheme of any other -- the coordinates of Prefiltered's merged windows."""
from oracle_harness import graphemes


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


# the three engines of test_gpu_batch_prefilter.py with non-ASCII patterns added to each; "cafés"
# and "résumé writer" hold pattern graphemes of two code points
PACKED_ASCII = ["hello", "world", "cell", "abcdefg", "saddam", "hussein8"]
PACKED_UNI = ["wörld", "москва", "東京都庁", "cafés"]
QGRAM_ASCII = ["vestibulum", "consectetur", "adipiscing elit", "lorem ipsum dolo", "pellentesque"]
QGRAM_UNI = ["naïve café", "здравствуйте", "東京都庁舎前駅北口広場", "résumé writer"]
ENGINES = {"packed": (PACKED_ASCII + PACKED_UNI, 0.75), "qgram": (QGRAM_ASCII + QGRAM_UNI, 0.85),
           "mixed": (PACKED_ASCII + PACKED_UNI + QGRAM_ASCII + QGRAM_UNI, 0.8)}
N_QGRAM = len(QGRAM_ASCII + QGRAM_UNI)

AFILL = ["z", "q", "0", " "]  # no symbol of any pattern but the space
UFILL = ["z", "q", "0", " ", "ж", "ü", "→", "q̈", "😀"]  # ... and none here; every unit is one grapheme


def glen(s):
    """Symbols of a document: bytes if it is ASCII (search.rs:196), else graphemes."""
    return len(s) if s.isascii() else len(graphemes(s))


def fill(rng, n, units=AFILL):
    return "".join(units[rng.next() % len(units)] for _ in range(n))


def ufill(rng, n):
    """n graphemes, the first one not ASCII (n > 0)."""
    return ("ж" + fill(rng, n - 1, UFILL)) if n > 0 else ""


def near(rng, p):
    """p, or p with one grapheme substituted by a filler symbol (still within one edit)."""
    if rng.next() % 2:
        return p
    g = graphemes(p)
    g[rng.next() % len(g)] = "z"
    return "".join(g)


def split_pats(pats):
    return [p for p in pats if p.isascii()], [p for p in pats if not p.isascii()]


def boundary_docs(pats, shift, seed):
    """test_gpu_batch_prefilter.boundary_docs in symbol space: document boundaries at symbols 32, 64,
    4096 and 4096 + 87 (+ shift) of the batch's start-window space, ASCII and non-ASCII documents
    alternating (Unicode|Unicode, Unicode|ASCII, ASCII|Unicode, Unicode|empty|empty|Unicode at the
    four cuts), so a byte position is no symbol position after the first document. At every cut one
    occurrence ends exactly at the cut and another starts right after it. Then the edge documents in
    non-ASCII form, one document of 20 Ki symbols, and documents without any window and with two."""
    rng = Rng(seed)
    apats, upats = split_pats(pats)
    pick = lambda ps: ps[rng.next() % len(ps)]  # noqa: E731
    cuts = [0, 32 + shift, 64 + shift, 4096 + shift, 4096 + 87 + shift]
    kinds = ["u", "u", "a", "u"]
    docs = []
    for (a, b), kind in zip(zip(cuts, cuts[1:]), kinds):
        ps = apats if kind == "a" else upats
        head = near(rng, pick(ps)) if a else ""
        tail = pick(ps)  # exact: its last grapheme is the document's last symbol
        if kind == "u" and a:
            head = pick(upats)  # (keeps the document non-ASCII whatever `near` substitutes)
        body = b - a - len(graphemes(head)) - len(graphemes(tail))
        assert body >= 0, (a, b, head, tail)
        docs.append(head + (fill(rng, body) if kind == "a" else fill(rng, body, UFILL)) + tail)
        assert docs[-1].isascii() == (kind == "a") and glen(docs[-1]) == b - a, (kind, a, b, docs[-1])
    docs += ["", ""]
    docs.append(near(rng, upats[0]) + ufill(rng, 9))  # an occurrence right after the last cut
    p = graphemes(upats[1])
    h = len(p) // 2
    docs += [ufill(rng, 5) + "".join(p[:h]), "".join(p[h:]) + ufill(rng, 7)]  # cut in two by a boundary
    docs += ["".join(p[1:]) + ufill(rng, 30), "ж" + "".join(p[2:]) + ufill(rng, 3), "".join(p[:-1]) + "→",
             ufill(rng, 2) + "".join(p)]  # clamped at the start
    docs += ["", "ж", "é", "q̈", "м", "мо", "".join(p[:3]), ""]  # one grapheme, shorter than every pattern
    docs += [upats[0], "", "", "", upats[0], ""]  # touching occurrences around empty documents
    long = []
    while sum(map(glen, long)) < 20 * 1024:
        long.append(near(rng, pick(pats)) if rng.next() % 5 == 0 else ufill(rng, 1 + rng.next() % 90))
    docs.append("".join(long))
    for i in range(24):  # no window at all / two windows: an all-ASCII slice and one that is not
        if i % 2 == 0:
            docs.append(ufill(rng, 3 + rng.next() % 40) if i % 4 == 0 else fill(rng, 3 + rng.next() % 40))
        else:
            docs.append("é" + fill(rng, 40) + apats[i % len(apats)] + fill(rng, 40) + upats[i % len(upats)] + ufill(rng, 5))
    docs += [apats[-1], upats[-1]]  # the last document: an occurrence ending at its last grapheme
    assert glen(docs[-1 - 26]) >= 20 * 1024 and not docs[0].isascii() and not docs[-1].isascii()
    pre = [0]
    for d in docs:
        pre.append(pre[-1] + glen(d))
    assert pre[1:5] == cuts[1:]
    return docs


def small_batches(pats):
    """The first document non-ASCII, the last one too with an occurrence ending at its last grapheme;
    an all-non-ASCII batch; batches of one document."""
    apats, upats = split_pats(pats)
    rng = Rng(0x5A11)
    return [
        [upats[0] + ufill(rng, 6), fill(rng, 12) + apats[0], "", fill(rng, 20), ufill(rng, 25), ufill(rng, 9) + upats[1]],
        [ufill(rng, 7) + upats[2], upats[3] + ufill(rng, 3), ufill(rng, 18), ufill(rng, 31), "ж", upats[0] + "→" + upats[0]],
        [ufill(rng, 40) + upats[1] + ufill(rng, 40) + upats[2]],
        ["é"],
        [upats[3]],
    ]


def is_cut_pair(docs):
    """(document, symbol) of the window end / start the two occurrences at each of the four cuts give."""
    ends = [(d, glen(docs[d])) for d in range(4)]
    starts = [(1, 0), (2, 0), (3, 0), (6, 0)]  # (documents 4 and 5 are the empty ones after the last cut)
    return ends, starts


def oracle_windows(orc, docs, thr):
    """(document, start, end) of the oracle's merged windows in symbols, ends clamped to the document."""
    out = []
    for d, doc in enumerate(docs):
        ws = orc.prefilter_windows(doc, thr)
        assert ws is not None
        out += [(d, s, min(e, glen(doc))) for s, e in ws]
    return out


def window_bytes(doc, s, e):
    """The byte slice of symbols [s, e) of a document."""
    if doc.isascii():
        return doc[s:e].encode()
    return "".join(graphemes(doc)[s:e]).encode("utf-8")


# ---- slices (test 3): one engine whose haystacks fold onto pattern symbols, a one-grapheme pattern
SLICE_PATS = PACKED_ASCII + PACKED_UNI + ["i̇stanbul", "straße", "σοφία", "я"]
SLICE_THR = 0.75
BIG = "l" + "́" * 39  # one grapheme of 40 code points


def slice_docs():
    z = lambda n: "z" * n  # noqa: E731
    docs = ["éé" + z(12) + "hello\r\nworld" + z(12) + "ü",  # an all-ASCII window with "\r\n" inside
            "ж" + z(10) + "world\r\n\r\nhello" + z(14) + "\r\n" + z(3) + "é"]
    for j in range(12):  # one non-ASCII grapheme sweeping over the window's first / last positions
        docs.append(z(j) + "ж" + z(11 - j) + "hello" + z(12))
        docs.append(z(12) + "hello" + z(j) + "ж" + z(11 - j))
    docs += ["ж" + z(14) + "hello", z(9) + "→" + z(9) + "wörld", "é" + z(20) + "cafés"]  # at the very end
    docs += ["я", z(9) + "я" + z(9) + "é", "é" + z(5) + "Я" + z(3)]  # a window one grapheme long
    docs += [z(5) + " ".join(["wörld"] * 14) + z(5), "é" + z(7) + " ".join(["hello", "world", "cell"] * 6) + z(7)]  # > 64 bytes
    docs += [z(8) + "hel" + BIG + "o" + z(8), "ж" + z(8) + "wör" + BIG + "d" + BIG + z(8)]  # a 40-code-point grapheme
    docs += [z(6) + "İSTANBUL" + z(6), z(6) + "STRAẞE" + z(6), z(6) + "ΣΟΦΊΑ" + z(6), "İẞΣ", z(4) + "İstanbul straẞe Σοφία"]
    return docs


# ---- the random differential (test 5)
SCRIPTS = [["a", "b", "e", "l", "o", " ", "z", "0"], ["é", "ö", "ñ", "a", " ", "z", "ü", "é"],
           ["м", "о", "с", "к", "в", "а", " ", "ж", "z"], ["東", "京", "都", "庁", "z", "。", " "], ["😀", "z", "\r\n", " ", "q̈"]]
DIFF_PATS = ["hello", "world", "wörld", "москва", "東京都庁", "cafés", "vestibulum", "naïve café", "здравствуйте"]
DIFF_THR = 0.8
DIFF_SEEDS = [0x1234_5678_9abc_def1, 0xdead_beef_0bad_f00d, 0x0a57_2a1c_0de5_51de, 0x5eed_0004, 0x5eed_0005]


def one_edit(rng, p):
    g = graphemes(p)
    i = rng.next() % len(g)
    kind = rng.next() % 3
    if kind == 0:
        g[i] = "z"
    elif kind == 1 and len(g) > 4:
        del g[i]
    else:
        g.insert(i, "z")
    return "".join(g)


def random_docs(seed, n_docs=40):
    """About 40 documents of up to 200 symbols, a random mix of scripts and of ASCII and non-ASCII
    documents, with planted exact and one-edit occurrences."""
    rng = Rng(seed)
    docs = []
    for _ in range(n_docs):
        ascii_doc = rng.next() % 3 == 0
        scripts = [SCRIPTS[0]] if ascii_doc else [SCRIPTS[rng.next() % len(SCRIPTS)] for _ in range(1 + rng.next() % 3)]
        pats = [p for p in DIFF_PATS if p.isascii()] if ascii_doc else DIFF_PATS
        n, doc = rng.next() % 60, ""
        for _ in range(n):
            r = rng.next() % 16
            if r == 0:
                doc += pats[rng.next() % len(pats)]
            elif r == 1:
                doc += one_edit(rng, pats[rng.next() % len(pats)])
            else:
                s = scripts[rng.next() % len(scripts)]
                doc += s[rng.next() % len(s)]
        docs.append(doc)
    return docs
