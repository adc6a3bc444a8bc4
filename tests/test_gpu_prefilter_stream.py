"""Pre-filtered streams (fac_stream_open_ex / fac_replace_stream_open_ex) and the device transcode
of Unicode text (symbol_ids_kernel, slice_desc_kernel).

Expected values come from the CPU oracle through the existing emulators, which take any object with
.search: stream_emulation.stream_rows and test_replace_stream_host.emulate_replace_stream over
OracleEngine(...).with_prefilter(). The symbol ids are checked against a restatement of
prefilter.rs:186-202 / 247-281 (ids in first-seen order over the patterns' folded graphemes, from 1).

The streams run with FAC_STREAM_READ_BYTES=128 (the reader's read size, a diagnostics knob like
FAC_STREAM_BATCH_BYTES), window_bytes 512 and tasks of 1-2 KiB, so that a few KiB of input give
several windows and several tasks, cut exactly as the emulators cut them for reads of 128 bytes.
The overlap is the engine's own (max_match_graphemes + 1 = 11 for both generators): a stream takes no
other, and the replay's 50 and 42 rows are the same for 11 and 12."""
import ctypes
import io
import random

import numpy as np
import pytest

from fuzzy_aho_corasick import FuzzyAhoCorasickBuilder as B, FuzzyLimits as L, _native
from fuzzy_aho_corasick.engine import (DeviceError, FuzzyReplacer, ReplacementTable, StagedHaystack, StreamMatch, Wrap,
                                       _ReplaceStream, _Stream, f32)
from oracle_harness import OracleEngine, fold, graphemes
from stream_emulation import stream_rows
from test_replace_stream_host import (OVERLAP, PATTERNS, TABLE, THRESHOLD, UNIT, emulate_replace_stream,
                                      fixture_builder, reader_windows)

pytestmark = pytest.mark.gpu

THR = 0.8
WINDOW, READ = 512, 128


def _builder():
    return B().fuzzy(L().edits(1)).case_insensitive(True)


# ---------------------------------------------------------------- symbol ids

E_ACUTE = "e\u0301"
E_ACUTE_CIRC = "e\u0301\u0302"
FLAG_DE, FLAG_DK = "\U0001F1E9\U0001F1EA", "\U0001F1E9\U0001F1F0"
FAMILY = "\U0001F468\u200D\U0001F469\u200D\U0001F467"
FAMILY_BOY = "\U0001F468\u200D\U0001F469\u200D\U0001F466"
HANGUL_LVT, HANGUL_LV = "\u1100\u1161\u11A8", "\u1100\u1161"
I_DOT = "i\u0307"
LONG40 = "a" + "".join(chr(0x300 + i) for i in range(39))  # one grapheme of 40 code points
SYMBOLS = ["a", "\u00E9", "\u65E5", "\U0001D11E", E_ACUTE, "e", E_ACUTE_CIRC, FLAG_DE, FAMILY, HANGUL_LVT, "\r\n",
           I_DOT, "\u00DF", "\u03C3", LONG40]
# graphemes that share a first code point (or a prefix) with a symbol but are not one, then case
# variants that fold onto a symbol only when the engine is case-insensitive; and unknown graphemes
NEVER = ["e\u0302", "\u00E9\u0301", FLAG_DK, FAMILY_BOY, HANGUL_LV, "i\u0308", "\r", "\n", LONG40[:39],
         LONG40 + "\u0300", "a\u0300"]
LOOKALIKES = NEVER + ["\u0130", "\u1E9E", "\u03A3", "A", "\u00C9", "E\u0301"]
UNKNOWN = ["z", "\u0436", "\u8A9E", "\U0001F600", " "]
SYMBOL_PATTERNS = [" ".join(SYMBOLS[:8]), " ".join(SYMBOLS[8:])]


def _symbol_table(patterns, ci):
    table = {}
    for p in patterns:
        for g in graphemes(p):
            table.setdefault(fold(g, ci), len(table) + 1)
    return table


def _want_ids(table, text, ci):
    data = text.encode()
    if data.isascii():
        return [table.get(fold(chr(b), ci), 0) for b in data]
    return [table.get(fold(g, ci), 0) for g in graphemes(text)]


def _symbol_text(n, last):
    """A text of n graphemes over symbols, look-alikes and unknown graphemes whose last grapheme is `last`."""
    rng = random.Random(n)
    pool = SYMBOLS + LOOKALIKES + UNKNOWN
    gs = []
    while len(gs) < n + 8:
        gs = graphemes("".join(gs) + " ".join(rng.sample(pool, len(pool))))
    text = "".join(gs[:n - 1]) + last
    assert len(graphemes(text)) == n and not text.isascii()
    return text


@pytest.fixture(scope="module", params=[True, False], ids=["ci", "cs"])
def sym(request):
    ci = request.param
    for p in SYMBOL_PATTERNS:
        assert [g for g in graphemes(p) if g != " "] == [s for s in SYMBOLS if s in graphemes(p)]
    eng = B().case_insensitive(ci).device(0).build(SYMBOL_PATTERNS)
    table = _symbol_table(SYMBOL_PATTERNS, ci)
    assert len(table) == len(SYMBOLS) + 1 and eng.with_prefilter().is_active()
    return eng, table, ci


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_symbol_ids_of_unicode_text(sym, n):
    eng, table, ci = sym
    for last in ("\u65E5", FAMILY, LONG40):  # the haystack's last grapheme is a multi-byte symbol
        text = _symbol_text(n, last)
        want = _want_ids(table, text, ci)
        assert want[-1] == table[last]
        got = StagedHaystack(eng, text.encode()).symbol_ids()
        assert got.dtype == np.uint8 and got.tolist() == want, text


def test_symbol_ids_hit_every_symbol_and_lookalike(sym):
    eng, table, ci = sym
    text = " ".join(SYMBOLS + LOOKALIKES + UNKNOWN) + " \u65E5"
    want = _want_ids(table, text, ci)
    assert set(want) == set(range(len(table) + 1))  # every symbol and "other"
    by_g = dict(zip(graphemes(text), want))
    for g in NEVER + UNKNOWN[:4]:
        assert by_g[g] == 0, g
    # U+0130 folds to i + U+0307, U+1E9E to U+00DF, capital sigma to U+03C3: hits exactly when folding
    folded = (table[I_DOT], table["\u00DF"], table["\u03C3"], table["a"], table["\u00E9"], table[E_ACUTE])
    assert tuple(by_g[g] for g in LOOKALIKES[len(NEVER):]) == (folded if ci else (0,) * 6)
    assert StagedHaystack(eng, text.encode()).symbol_ids().tolist() == want


def test_symbol_ids_of_ascii_text(sym):
    eng, table, ci = sym
    text = "A needle\r\nE e a\n"
    want = _want_ids(table, text, ci)
    assert len(want) == len(text) and (want[0] == table["a"]) == ci and want[-2] == table["a"]
    assert StagedHaystack(eng, text.encode()).symbol_ids().tolist() == want


def test_symbol_ids_after_a_restage(sym):
    import torch
    eng, table, ci = sym
    first, second = _symbol_text(257, FAMILY), _symbol_text(63, "\u65E5")
    bufs = [torch.tensor(list(t.encode()), dtype=torch.uint8, device="cuda") for t in (first, second)]
    st = StagedHaystack.from_device(eng, bufs[0].data_ptr(), bufs[0].numel())
    assert st.symbol_ids().tolist() == _want_ids(table, first, ci)
    st = StagedHaystack.from_device(eng, bufs[1].data_ptr(), bufs[1].numel(), reuse=st)
    assert st.graphemes == 63 and st.symbol_ids().tolist() == _want_ids(table, second, ci)


@pytest.mark.parametrize("n_symbols", [1, 255, 256])
def test_symbol_ids_alphabet_sizes(n_symbols):
    syms = [chr(0x4E00 + i) for i in range(n_symbols)]
    pats = ["".join(syms[i:i + 51]) for i in range(0, n_symbols, 51)]
    eng = B().device(0).build(pats)
    text = "".join(reversed(syms)) + "あz" + syms[-1]
    st = StagedHaystack(eng, text.encode())
    if n_symbols == 256:  # a 256th distinct symbol: no filter
        assert not eng.with_prefilter().is_active() and st.symbol_ids() is None
        return
    table = _symbol_table(pats, False)
    assert len(table) == n_symbols and max(table.values()) == n_symbols
    assert st.symbol_ids().tolist() == _want_ids(table, text, False)


# ---------------------------------------------------------------- pre-filter parity on crafted inputs

PARITY_PATTERNS = ["nadel", "москва", "école", "straße"]
CJK = "日本語"


class Parity:
    def __init__(self, builder, patterns):
        self.eng, self.orc = builder.device(0).build(patterns), OracleEngine(builder, patterns)

    def slices(self, text):
        """The oracle's merged windows of `text`: (start, end clamped, the window's text)."""
        gs = graphemes(text)
        return [(s, min(e, len(gs)), "".join(gs[s:min(e, len(gs))])) for s, e in self.orc.prefilter_windows(text, THR)]

    def check(self, text):
        assert not text.isascii()
        want = self.orc.raw_rows(text, THR, prefilter=True)
        got, _ = self.eng.stage(text.encode()).search_prefiltered(THR)
        assert sorted(got) == sorted(want), text
        return want


@pytest.fixture(scope="module")
def par():
    return Parity(_builder(), PARITY_PATTERNS)


def test_parity_ascii_window_with_crlf_inside_unicode_text(par):
    text = (CJK + " ") * 3 + "zzzz zzzz zzzz nadel\r\nnadl zzzz zzzz zzzz" + (" " + CJK) * 3
    (s, e, sl), = par.slices(text)
    assert sl.isascii() and "\r\n" in sl and len(sl) == e - s + 1  # ("\r\n": one grapheme, two bytes)
    assert len(par.check(text)) >= 2


def test_parity_window_with_its_only_non_ascii_byte_first_or_last(par):
    base = "z" * 14 + " nadel " + "z" * 14
    seen = set()
    for p in [i for i, c in enumerate(base) if c == "z"]:
        text = base[:p] + "é" + base[p + 1:]
        (s, e, sl), = par.slices(text)
        if not sl.isascii():
            seen.add("first" if sl[0] == "é" else "last" if sl[-1] == "é" else "inside")
        else:
            seen.add("ascii")
        assert len(par.check(text)) >= 1
    assert seen == {"first", "last", "inside", "ascii"}


def test_parity_window_ending_at_the_end_of_the_text(par):
    for text in (CJK + " zzzz zzzz nadel", CJK + " zzzz zzzz nade", "zzzz zzzz mosk москва"):
        s, e, sl = par.slices(text)[-1]
        assert e == len(graphemes(text))
        assert len(par.check(text)) >= 1


def test_parity_window_of_a_single_grapheme():
    one = Parity(B().case_insensitive(True), ["é"])
    for text in (CJK + " zzzz É zzzz", "zzé", "é"):
        (s, e, sl), = one.slices(text)
        assert e - s == 1
        assert len(one.check(text)) == 1


def test_parity_windows_longer_than_64_bytes(par):
    uni = CJK + " " + "nadel zz " * 12 + "日"
    asc = CJK + " zzzz zzzz " + "nadel zz " * 12 + "zzzz zzzz " + CJK
    for text, is_ascii in ((uni, False), (asc, True)):
        (s, e, sl), = par.slices(text)
        assert sl.isascii() == is_ascii and len(sl.encode()) > 64 and len(sl.encode()) % 64 != 0
        assert len(par.check(text)) >= 12


def test_parity_more_than_64_merged_windows(par):
    text = (CJK + " zzzz zzzz zzzz nadel zzzz zzzz zzzz straße zzzz zzzz zzzz ") * 36
    sl = par.slices(text)
    assert len(sl) > 64 and {w[2].isascii() for w in sl} == {True, False}
    assert len(par.check(text)) >= 72


def test_parity_views_of_a_unicode_haystack(par):
    """stream_window(g_begin > 0, prefilter=True): the view's text searched as Prefiltered::search."""
    text = (CJK + " zzzz zzzz zzzz nadel\r\nzzzz zzzz zzzz straße zzzz zzzz zzzz ") * 6
    gs = graphemes(text)
    starts = [0]
    for g in gs:
        starts.append(starts[-1] + len(g.encode()))
    st = par.eng.stage(text.encode())
    from fuzzy_aho_corasick import SearchOptions as O
    pre = par.orc.with_prefilter()
    for g0, g1 in ((3, len(gs)), (17, 120), (40, 41), (len(gs) - 30, len(gs)), (5, 5)):
        sub = "".join(gs[g0:g1])
        commit = max(0, len(sub.encode()) - 7)
        want = sorted((starts[g0] + m.start + 1000, starts[g0] + m.end + 1000, m.pattern_index, m.sim_bits())
                      for m in pre.search(sub, O().threshold(THR).sorted().non_overlapping()) if m.start < commit)
        rows, _ = st.stream_window(g0, g1, commit, starts[g0] + 1000, THR, True)
        got = sorted((int(r["start"]), int(r["end"]), int(r["pattern_index"]),
                      int(np.float32(r["similarity"]).view(np.uint32))) for r in rows)
        assert got == want, (g0, g1)


# ---------------------------------------------------------------- search streams

ASCII_GEN = (["needle", "haystack", "automaton"], ["lorem", "ipsum", "dolor", "sit", "amet", "quux", "zzz"],
             ["nedle", "haystack", "automatn", "needle"])
UNI_GEN = (["nadel", "heuhaufen", "москва", "école", "straße"],
           ["lorem", "ипсум", "dolor", "sït", "amet", CJK, "zzz"],
           ["nadl", "Москва", "ecole", "strasse", "ÉCOLE", "heuhaufn"])


def _generate(fillers, hits, words=600, seed=7):
    rng = random.Random(seed)
    return " ".join(rng.choice(hits) if i % 12 == 11 else rng.choice(fillers) for i in range(words))


def _count(text: str) -> int:
    return len(text) if text.isascii() else len(graphemes(text))


def _covered(orc, text: str, thr: float) -> int:
    n = _count(text)
    return sum(min(e, n) - s for s, e in orc.prefilter_windows(text, thr))


class Case:
    """One generator: the engine, the oracle, the text, and the oracle's replay (computed once)."""

    def __init__(self, gen, builder=None, thr=THR, data=None, check=True):
        pats, fillers, hits = gen
        b = builder or _builder()
        self.thr = thr
        self.eng, self.orc = b.device(0).build(pats), OracleEngine(b, pats)
        self.data = data if data is not None else _generate(fillers, hits).encode()
        self.overlap = self.eng.max_match_graphemes() + 1
        self.wins = reader_windows(self.data, self.overlap, WINDOW, READ)
        self.texts = [self.data[b0:e0].decode() for b0, e0, _ in self.wins]
        self.want_plain = sorted(stream_rows(self.orc, self.data, thr, self.overlap, window=WINDOW, chunk=READ))
        self.want = sorted(stream_rows(self.orc.with_prefilter(), self.data, thr, self.overlap, window=WINDOW, chunk=READ))
        self.plain_windows = sum(_count(t) for t in self.texts)
        if check:  # the conditions on a generator, before any GPU comparison
            text = self.data.decode()
            assert _covered(self.orc, text, thr) <= 0.30 * _count(text)
            assert len(self.want) >= 30 and len(self.wins) >= 5

    def filtered_windows(self):
        return sum(_covered(self.orc, t, self.thr) for t in self.texts)


def _knobs(monkeypatch, batch=2048):
    monkeypatch.setenv("FAC_STREAM_READ_BYTES", str(READ))
    monkeypatch.setenv("FAC_STREAM_BATCH_BYTES", str(batch))


def _rows(ms):
    return [(m.start, m.end, m.pattern_index, int(np.float32(m.similarity).view(np.uint32)), m.text) for m in ms]


def _run_stream(st, data, piece=4096):
    out = []
    pieces = [data[i:i + piece] for i in range(0, len(data), piece)] or [b""]
    for i, p in enumerate(pieces):
        out += st.feed(p, eof=i == len(pieces) - 1)
    assert st.total() == len(data)
    return sorted(_rows(out)), st.windows_searched()


@pytest.fixture(scope="module")
def ascii_case():
    c = Case(ASCII_GEN)
    assert (c.overlap, len(c.want), len(c.want_plain)) == (11, 50, 50)
    return c


@pytest.fixture(scope="module")
def uni_case():
    c = Case(UNI_GEN)
    assert (c.overlap, len(c.want), len(c.want_plain)) == (11, 42, 42)
    return c


@pytest.mark.parametrize("which", ["ascii", "unicode"])
def test_prefiltered_stream_rows_and_windows_searched(which, ascii_case, uni_case, monkeypatch):
    c = ascii_case if which == "ascii" else uni_case
    assert c.data.isascii() == (which == "ascii")
    for batch in (2048, 1):  # several windows a task (ASCII: the batched path), and every window a task of its own
        _knobs(monkeypatch, batch)
        for piece in (4096, 7):
            got, searched = _run_stream(_Stream(c.eng, c.thr, WINDOW, prefilter=True), c.data, piece)
            assert got == c.want
            assert searched == c.filtered_windows() < c.plain_windows
        got, searched = _run_stream(_Stream(c.eng, c.thr, WINDOW), c.data)
        assert got == c.want_plain and searched == c.plain_windows


def _open_plain(eng, thr, window):
    """The existing call, fac_stream_open, behind a _Stream."""
    st = _Stream.__new__(_Stream)
    h = ctypes.c_void_p()
    assert _native.lib.fac_stream_open(eng._h, f32(thr), window, ctypes.byref(h)) == 0
    st._h, st.engine = h, eng
    return st


@pytest.mark.parametrize("which", ["ascii", "unicode"])
def test_prefilter_off_through_the_ex_calls_is_the_existing_stream(which, ascii_case, uni_case, monkeypatch):
    c = ascii_case if which == "ascii" else uni_case
    _knobs(monkeypatch)
    a = _run_stream(_open_plain(c.eng, c.thr, WINDOW), c.data)
    assert a == _run_stream(_Stream(c.eng, c.thr, WINDOW, prefilter=False), c.data) == (c.want_plain, c.plain_windows)
    # the replace stream: fac_replace_stream_open and _ex(..., 0, ...) give the same bytes
    table = ReplacementTable(c.eng, ["<%d>" % i for i in range(len(c.eng.patterns()))])
    h = ctypes.c_void_p()
    assert _native.lib.fac_replace_stream_open(c.eng._h, table._h, f32(c.thr), WINDOW, ctypes.byref(h)) == 0
    old = _ReplaceStream.__new__(_ReplaceStream)
    old._h, old.engine, old.table = h, c.eng, table
    new = _ReplaceStream(c.eng, table, c.thr, WINDOW, prefilter=False)
    assert old.feed(c.data, eof=True) == new.feed(c.data, eof=True)
    assert old.windows_searched() == new.windows_searched() == c.plain_windows


def _alternating_text():
    """2 KiB blocks: ASCII words in the first half, the non-ASCII generator's words in the second."""
    _, fillers, hits = UNI_GEN
    rng = random.Random(11)
    a_fill, a_hits = [w for w in fillers if w.isascii()], [w for w in hits if w.isascii()]
    out, block = "", 0
    while block < 5:
        half, i = "", 0
        while len(half.encode()) < 1024 - 12:
            half += (rng.choice(a_hits) if i % 12 == 11 else rng.choice(a_fill)) + " "
            i += 1
        half += "z" * (1024 - len(half.encode()))
        out += half
        half = ""
        while len(half.encode()) < 1024 - 24:
            half += (rng.choice(hits) if i % 12 == 11 else rng.choice(fillers)) + " "
            i += 1
        half += "z" * (1024 - len(half.encode()))
        out += half
        block += 1
    assert len(out.encode()) == 5 * 2048
    return out.encode()


def _tasks(wins, batch):
    """stream.cpp's tasks: consecutive windows until their text holds `batch` bytes."""
    tasks, cur = [], []
    for w in wins:
        cur.append(w)
        if cur[-1][1] - cur[0][0] >= batch:
            tasks.append(cur)
            cur = []
    return tasks + ([cur] if cur else [])


def test_stream_whose_tasks_alternate_between_ascii_and_unicode(monkeypatch):
    c = Case(UNI_GEN, data=_alternating_text(), check=False)
    kinds = [(c.data[t[0][0]:t[-1][1]].isascii(), len(t)) for t in _tasks(c.wins, 600)]
    assert sum(1 for a, n in kinds if a and n > 1) >= 3 and sum(1 for a, n in kinds if not a) >= 3
    assert len(c.want) >= 30
    _knobs(monkeypatch, 600)
    got, searched = _run_stream(_Stream(c.eng, c.thr, WINDOW, prefilter=True), c.data)
    assert got == c.want and searched == c.filtered_windows()


def test_fallback_threshold_is_the_plain_stream(monkeypatch):
    """No edit limits and a long pattern: k_for > 24 at this threshold, the reference searches in full."""
    pats = ASCII_GEN[0] + ["the quick brown fox jumps over the lazy dog"]
    c = Case((pats, ASCII_GEN[1], ASCII_GEN[2]), builder=B().case_insensitive(True), thr=0.7, check=False)
    assert c.eng.with_prefilter().is_active() and c.orc.with_prefilter().is_active()
    assert c.orc.prefilter_windows(c.data.decode(), 0.7) is None
    assert c.orc.prefilter_windows(c.data.decode(), 0.99) is not None
    assert len(c.want) >= 20 and len(c.wins) >= 5
    _knobs(monkeypatch)
    plain = _run_stream(_Stream(c.eng, c.thr, WINDOW), c.data)
    assert plain == (c.want_plain, c.plain_windows)
    assert _run_stream(_Stream(c.eng, c.thr, WINDOW, prefilter=True), c.data) == plain


@pytest.mark.parametrize("which", ["ascii", "unicode"])
def test_mapping_engine_has_no_filter_and_streams_plain(which, monkeypatch):
    pats, fillers, hits = UNI_GEN  # ("straße": the mapping applies, so the engine has no filter)
    data = _generate([w for w in fillers if w.isascii()], [w for w in hits if w.isascii()]).encode() if which == "ascii" else None
    c = Case(UNI_GEN, builder=_builder().mapping("ss", "ß"), data=data, check=False)
    assert c.data.isascii() == (which == "ascii")
    assert not c.eng.with_prefilter().is_active() and not c.orc.with_prefilter().is_active() and len(c.want_plain) >= 30
    _knobs(monkeypatch)
    plain = _run_stream(_Stream(c.eng, c.thr, WINDOW), c.data)
    assert plain == (c.want_plain, c.plain_windows)
    assert _run_stream(_Stream(c.eng, c.thr, WINDOW, prefilter=True), c.data) == plain


@pytest.mark.parametrize("which", ["ascii", "unicode"])
def test_auto_beam_engine_prefiltered_stream(which, monkeypatch):
    c = Case(ASCII_GEN if which == "ascii" else UNI_GEN, builder=_builder().auto_beam(40, 8), check=False)
    assert len(c.want) >= 30
    _knobs(monkeypatch)
    got, searched = _run_stream(_Stream(c.eng, c.thr, WINDOW, prefilter=True), c.data)
    assert got == c.want and searched == c.filtered_windows()


@pytest.mark.parametrize("which", ["ascii", "unicode"])
def test_prefiltered_python_stream_methods_agree(which, ascii_case, uni_case, monkeypatch):
    c = ascii_case if which == "ascii" else uni_case
    _knobs(monkeypatch)
    pre = c.eng.with_prefilter()
    a, b = [], []
    assert pre.search_stream(io.BytesIO(c.data), c.thr, a.append, window=WINDOW) == len(c.data)
    assert all(isinstance(m, StreamMatch) for m in a) and sorted(_rows(a)) == c.want
    assert _rows(pre.stream_matches(io.BytesIO(c.data), c.thr, window=WINDOW)) == _rows(a)
    # (the parallel form has no window argument: the default 256 KiB window holds the whole text)
    assert pre.search_stream_parallel(io.BytesIO(c.data), c.thr, 4, b.append) == len(c.data)
    whole = sorted(stream_rows(c.orc.with_prefilter(), c.data, c.thr, c.overlap))
    assert sorted(_rows(b)) == whole


# ---------------------------------------------------------------- replace streams

def _replace(eng, table, data, piece, thr=THRESHOLD, window=WINDOW, prefilter=True):
    st = _ReplaceStream(eng, table, thr, window, prefilter=prefilter)
    out = bytearray()
    pieces = [data[i:i + piece] for i in range(0, len(data), piece)] or [b""]
    for i, p in enumerate(pieces):
        out += st.feed(p, eof=i == len(pieces) - 1)
    assert st.written() == len(out)
    return bytes(out), st.counts(), st.windows_searched()


def test_prefiltered_replace_stream_ascii_fixture(monkeypatch):
    """UNIT * 40 against TABLE: all ASCII, several windows a task (the batched path)."""
    b = fixture_builder()
    eng, orc = b.device(0).build(PATTERNS), OracleEngine(b, PATTERNS)
    data = (UNIT * 40).encode()
    assert eng.max_match_graphemes() + 1 == OVERLAP
    want = emulate_replace_stream(orc.with_prefilter(), data, TABLE, THRESHOLD, overlap=OVERLAP, window=WINDOW, read=READ)
    assert want.ties == 0 and len(want.windows) >= 5 and want.applied > 100
    searched = sum(_covered(orc, data[b0:e0].decode(), THRESHOLD) for b0, e0, _ in want.windows)
    _knobs(monkeypatch)
    table = ReplacementTable(eng, TABLE)
    for piece in (1, 7, 4096):
        assert _replace(eng, table, data, piece) == (want.out, (want.applied, want.skipped), searched), piece


def test_prefiltered_replace_stream_unicode(uni_case, monkeypatch):
    c = uni_case
    entries = ["NADEL", None, Wrap("[", "]"), "", ""]
    want = emulate_replace_stream(c.orc.with_prefilter(), c.data, entries, c.thr, overlap=c.overlap, window=WINDOW,
                                  read=READ)
    assert want.ties == 0 and want.applied >= 30 and [w[:2] for w in want.windows] == [w[:2] for w in c.wins]
    want.out.decode("utf-8")
    _knobs(monkeypatch)
    table = ReplacementTable(c.eng, entries)
    for piece in (1, 7, 4096):
        got = _replace(c.eng, table, c.data, piece, thr=c.thr)
        assert got == (want.out, (want.applied, want.skipped), c.filtered_windows()), piece
    # the Python forms: FuzzyReplacer's device table, and a callable over the pre-filtered search stream
    for f in (lambda r, w: FuzzyReplacer(c.eng, entries).replace_stream(r, w, c.thr, prefilter=True),
              lambda r, w: c.eng.with_prefilter().replace_stream(r, w, c.thr, entries),
              lambda r, w: c.eng.with_prefilter().replace_stream_parallel(r, w, 4, c.thr, entries),
              lambda r, w: c.eng.with_prefilter().replace_stream(
                  r, w, c.thr, lambda m: FuzzyReplacer(c.eng, entries)._callback(m))):
        out = io.BytesIO()
        # (no window argument: one window holds the whole text, whose matches are the stream's here)
        assert f(io.BytesIO(c.data), out) == len(out.getvalue())
        whole = emulate_replace_stream(c.orc.with_prefilter(), c.data, entries, c.thr, overlap=c.overlap)
        assert out.getvalue() == whole.out


def test_prefiltered_replace_stream_refuses_another_engines_table():
    eng = fixture_builder().device(0).build(PATTERNS)
    other = fixture_builder().device(0).build(["needle"])
    with pytest.raises(DeviceError) as ei:
        _ReplaceStream(eng, ReplacementTable(other, ["X"]), THRESHOLD, prefilter=True)
    assert ei.value.code == _native.FAC_E_INVALID
