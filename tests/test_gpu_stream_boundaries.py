"""Whole-token matches in streams (fac.h fac_stream_open_opts / fac_replace_stream_open_opts,
boundary_kernels.hip stream_boundary_filter_kernel): the boundary filter with left
context on both one-pass paths of a stream task (the ASCII union path and the window documents), on
the window-by-window path and in replace streams.

Expected rows, output bytes and counts come from stream_boundary_emulation: the CPU oracle's raw rows
of every window, the `regex`-based rule of test_boundaries_host.py with the whole earlier stream as
prefix, the oracle's apply, the ownership cut; replace streams through
test_replace_stream_host.emulate_replace_stream. Comparisons are bit-exact, similarity bits and
matched text included. Shapes are those of test_gpu_stream_window_docs.py: window_bytes 512, tasks of
FAC_STREAM_BATCH_BYTES = 2048, reads of 64 to 4096 bytes, texts of a few KiB."""
import ctypes
import io
import random

import pytest

from fuzzy_aho_corasick import Boundary, DeviceError, FuzzyAhoCorasickBuilder as B, FuzzyLimits as L, _native
from fuzzy_aho_corasick.engine import FuzzyReplacer, ReplacementTable, Wrap, _rendered_entry, _ReplaceStream, _Stream, f32
from oracle_harness import OracleEngine
from stream_boundary_emulation import StreamEmulation
from test_boundaries_host import Rng, random_doc
from test_gpu_boundaries import LETTERS, OTHERS
from test_gpu_prefilter_stream import _rows, _tasks
from test_replace_stream_host import PATTERNS, TABLE, UNIT, fixture_builder

pytestmark = pytest.mark.gpu

THR = 0.7
WINDOW, READ, BATCH = 512, 128, 2048
SIDES = (Boundary.NONE, Boundary.START, Boundary.END, Boundary.WHOLE)
SIDE_IDS = ["none", "start", "end", "whole"]
PF = pytest.mark.parametrize("prefilter", [False, True], ids=["plain", "prefiltered"])


def _builder(ci=True):
    return B().fuzzy(L().edits(1)).case_insensitive(ci)


def _knobs(monkeypatch, read=READ, batch=BATCH):
    monkeypatch.setenv("FAC_DIAGNOSTICS", "1")
    monkeypatch.setenv("FAC_STREAM_READ_BYTES", str(read))
    monkeypatch.setenv("FAC_STREAM_BATCH_BYTES", str(batch))
    monkeypatch.delenv("FAC_STREAM_WINDOW_DOCS", raising=False)


def _pieces(data, piece):
    return [data[i:i + piece] for i in range(0, len(data), piece)] or [b""]


def _search(eng, data, thr, prefilter, sides, piece=4096):
    """(rows, task_counts) of a flagged search stream fed in `piece`-byte pieces."""
    st = _Stream(eng, thr, WINDOW, prefilter=prefilter, boundaries=sides)
    out = []
    ps = _pieces(data, piece)
    for i, p in enumerate(ps):
        out += st.feed(p, eof=i == len(ps) - 1)
    assert st.total() == len(data)
    return sorted(_rows(out)), st.task_counts()


def _replace(eng, table, data, thr, prefilter, sides, piece=4096):
    st = _ReplaceStream(eng, table, thr, WINDOW, prefilter=prefilter, boundaries=sides)
    out = bytearray()
    ps = _pieces(data, piece)
    for i, p in enumerate(ps):
        out += st.feed(p, eof=i == len(ps) - 1)
    return bytes(out), st.written(), st.counts(), st.task_counts()


class Case:
    """An engine and its oracle; emulations are computed once per (text, read, pre-filter, mask)."""

    def __init__(self, pats, builder=None, thr=THR):
        b = builder or _builder()
        self.thr = thr
        self.eng, self.orc = b.device(0).build(pats), OracleEngine(b, pats)
        self.overlap = self.eng.max_match_graphemes() + 1
        self._emu = {}

    def emu(self, data, prefilter, sides, read=READ) -> StreamEmulation:
        key = (data, read, prefilter, int(sides))
        if key not in self._emu:
            self._emu[key] = StreamEmulation(self.orc, data, self.thr, self.overlap, WINDOW, read, prefilter, sides)
        return self._emu[key]

    def counts(self, emu, batch=BATCH):
        tasks = _tasks(emu.wins, batch)
        multi = sum(1 for t in tasks if len(t) > 1)
        return multi, len(tasks) - multi

    def check(self, monkeypatch, data, prefilter, sides, read=READ, batch=BATCH, piece=4096):
        emu = self.emu(data, prefilter, sides, read)
        _knobs(monkeypatch, read, batch)
        rows, counts = _search(self.eng, data, self.thr, prefilter, sides, piece)
        assert rows == emu.rows(), (int(sides), prefilter, read, batch, piece)
        assert counts == self.counts(emu, batch)
        return emu


def conditions(emu, batch=BATCH):
    """What a sweep must contain, from the emulation alone: (a) windows not first in their (batched)
    task with a raw record at window byte 0 that the rule drops with the stream's text before the
    window and would keep with the window as its document; (b) the same for the first window of a
    task after the first, where that text comes from the carried context; (c) raw records that end at
    a non-final window's end."""
    a = b = c = k = 0
    for ti, task in enumerate(_tasks(emu.wins, batch)):
        for wi in range(len(task)):
            if len(task) > 1 and emu.context_drops(k):
                a += int(wi > 0)
                b += int(wi == 0 and ti > 0)
            c += int(k < len(emu.wins) - 1 and bool(emu.ends_at_window_end(k)))
            k += 1
    return a, b, c


def sweep(case, texts, prefilter, sides, monkeypatch, need=(), **kw):
    """The emulation of every text first: the sweep's conditions are asserted before any stream runs."""
    emus = [case.emu(t, prefilter, sides, kw.get("read", READ)) for t in texts]
    tot = [sum(x) for x in zip(*[conditions(e, kw.get("batch", BATCH)) for e in emus])]
    if int(sides) & 1:  # (only the start side looks to the left of a window)
        assert tot[0] >= 1 and tot[1] >= 1, tot
    assert tot[2] >= 1, tot
    for n in need:
        assert any(n(e) for e in emus), n.__name__
    assert sum(case.counts(e)[0] for e in emus) >= 2 * len(emus)  # the tasks run batched
    for t in texts:
        case.check(monkeypatch, t, prefilter, sides, **kw)
    return emus


# ---------------------------------------------------------------- 1. the ASCII union path

ASCII_PATS = ["art", "cat", "smart"]
ASCII_UNIT = "party cart art, smart-art art7 _art "


def ascii_texts():
    """The pad takes every length of the unit: each commit point (fixed byte positions for ASCII
    text) lands on every position of every token."""
    return [("." * p + ASCII_UNIT * 130).encode() for p in range(len(ASCII_UNIT))]


@pytest.fixture(scope="module")
def ascii_case():
    return Case(ASCII_PATS)


@PF
@pytest.mark.parametrize("sides", SIDES, ids=SIDE_IDS)
def test_ascii_union_path(ascii_case, sides, prefilter, monkeypatch):
    texts = ascii_texts()
    assert all(t.isascii() for t in texts)
    emus = sweep(ascii_case, texts, prefilter, sides, monkeypatch)
    if int(sides):
        plain = ascii_case.emu(texts[0], prefilter, Boundary.NONE).rows()
        assert len(emus[0].rows()) < len(plain)  # the mask drops rows of this text


# ---------------------------------------------------------------- 2. the window-documents path

UNI_WORDS = ["art", "écol", "straße"]


def uni_unit():
    """Every word with neighbours of 1, 2, 3 and 4 bytes, letters and others, on both sides; decomposed
    "e" + U+0301 and U+0915 + U+093E (an alphabetic spacing mark) right before a word; a combining mark
    after a space; '_'."""
    before = LETTERS + OTHERS + ["cafe\u0301", "\u0915\u093e", " \u0301", "_"]
    after = LETTERS + OTHERS
    # (the four special cases are followed by a non-letter: only their start side can drop them)
    return "".join(n + UNI_WORDS[i % 3] + (after[(3 * i + 1) % 8] if i < 8 else OTHERS[i % 4]) + " "
                   for i, n in enumerate(before))


def uni_texts(pads=48):
    unit = uni_unit()
    return [("." * p + unit * 42).encode() for p in range(pads)]


def _window_after(tail: str):
    def found(emu):
        """A window after the first that begins right after `tail` and has a record there the rule drops."""
        t = tail.encode()
        return any(emu.data[:w[0]].endswith(t) and emu.context_drops(k) for k, w in enumerate(emu.wins) if k)
    found.__name__ = "window_after_" + ascii(tail)
    return found


UNI_ENGINES = {
    "ci": lambda: (UNI_WORDS, _builder(True)),
    "map": lambda: (["art", "écol", "strasse"], _builder(True).mapping("ss", "ß")),
}


@pytest.fixture(scope="module")
def uni_cases():
    return {}


def _uni_case(uni_cases, kind):
    if kind not in uni_cases:
        pats, b = UNI_ENGINES[kind]()
        uni_cases[kind] = Case(pats, b)
    return uni_cases[kind]


@PF
@pytest.mark.parametrize("sides", SIDES, ids=SIDE_IDS)
@pytest.mark.parametrize("kind", ["ci", "map"])
def test_window_documents_path(uni_cases, kind, sides, prefilter, monkeypatch):
    case = _uni_case(uni_cases, kind)
    texts = uni_texts()
    assert not any(t.isascii() for t in texts)
    need = (_window_after("e\u0301"), _window_after("\u093e")) if int(sides) & 1 else ()
    sweep(case, texts, prefilter, sides, monkeypatch, need=need)


# ---------------------------------------------------------------- 3. transparent runs across a window start

def run_text(overlap, k, mark):
    """"z" + k marks + "art" twice: the commit point of the window that ends at byte 1024 lies right
    after the first cluster (the next window is the third of the first task), that of the window that
    ends at byte 2048 right after the second (the next window is the first of the second task)."""
    cluster = "z" + mark * k
    tail = ("art " + "zz " * overlap)[:overlap]  # `overlap` graphemes, the first of them the 'a'
    out = b""
    for end in (1024, 2048):
        piece = (cluster + tail).encode()
        fill = end - len(out) - len(piece)
        out += (". " * fill)[:fill].encode() + piece
    return out + ("zz art " * 140).encode()[:1000], [1024 - overlap, 2048 - overlap]


@pytest.mark.parametrize("mark", ["\u0301", "\U000e0100"], ids=["2-byte", "4-byte"])
@pytest.mark.parametrize("k", [1, 31, 32, 33])
def test_transparent_runs_across_a_window_start(ascii_case, k, mark, monkeypatch):
    data, after = run_text(ascii_case.overlap, k, mark)
    cluster = ("z" + mark * k).encode()
    assert all(data[:p].endswith(cluster) and data[p:p + 3] == b"art" for p in after)
    for sides in (Boundary.START, Boundary.WHOLE, Boundary.END):
        for prefilter in (False, True):
            emu = ascii_case.emu(data, prefilter, sides)
            tasks = _tasks(emu.wins, BATCH)
            assert len(tasks) >= 2 and all(len(t) > 1 for t in tasks)
            assert after[0] in [w[0] for w in tasks[0][1:]] and after[1] == tasks[1][0][0]  # the emulated cuts
            kept = {r[0] for r in emu.rows() if r[:3] == (r[0], r[0] + 3, 0) and r[0] in after}
            if int(sides) & 1:  # 32 marks hide the letter; fewer do not
                assert kept == (set(after) if k >= 32 else set())
            ascii_case.check(monkeypatch, data, prefilter, sides)
    assert not k == 32 or len(mark.encode()) < 4 or len(cluster) == 129  # 32 four-byte marks fill the carry


# ---------------------------------------------------------------- 4. the window-by-window path

@pytest.mark.parametrize("sides", [Boundary.START, Boundary.WHOLE], ids=["start", "whole"])
def test_window_by_window_path(ascii_case, uni_cases, sides, monkeypatch):
    """FAC_STREAM_BATCH_BYTES = 1: every task is one window, filtered by the host rule."""
    def with_context_drop(case, texts):  # the first text of the sweep with a record only the left context drops
        return next(t for t in texts for e in [case.emu(t, False, sides)]
                    if any(e.context_drops(k) for k in range(1, len(e.wins))))

    uni = _uni_case(uni_cases, "ci")
    cases = ((ascii_case, with_context_drop(ascii_case, ascii_texts())), (uni, with_context_drop(uni, uni_texts())))
    for case, data in cases:
        for prefilter in (False, True):
            emu = case.emu(data, prefilter, sides)
            assert sum(1 for k in range(1, len(emu.wins)) if emu.context_drops(k)) >= 1
            _knobs(monkeypatch, batch=1)
            rows, counts = _search(case.eng, data, case.thr, prefilter, sides)
            assert rows == emu.rows()
            assert counts == (0, len(emu.wins)) and counts[1] > 0


# ---------------------------------------------------------------- 5. replace streams

def _check_replace(case, entries, data, prefilter, sides, monkeypatch, pieces=(4096,), read=READ):
    emu = case.emu(data, prefilter, sides, read)
    want = emu.replace(entries)
    assert want.ties == 0
    table = ReplacementTable(case.eng, entries)
    _knobs(monkeypatch, read)
    for piece in pieces:
        got = _replace(case.eng, table, data, case.thr, prefilter, sides, piece)
        assert got == (want.out, len(want.out), (want.applied, want.skipped), case.counts(emu)), (int(sides), piece)
    # the callable route: the flagged search stream, spliced on the host
    out = io.BytesIO()
    n = (case.eng.with_prefilter() if prefilter else case.eng).replace_stream(
        io.BytesIO(data), out, case.thr, lambda m: _rendered_entry(entries[m.pattern_index], m), WINDOW, boundaries=sides)
    assert (out.getvalue(), n) == (want.out, len(want.out))
    return want


@PF
@pytest.mark.parametrize("sides", [Boundary.START, Boundary.END, Boundary.WHOLE], ids=SIDE_IDS[1:])
def test_replace_streams(ascii_case, uni_cases, sides, prefilter, monkeypatch):
    entries = ["<ART>", None, Wrap("[", "]")]
    for case, texts in ((ascii_case, ascii_texts()), (_uni_case(uni_cases, "ci"), uni_texts())):
        for data in (texts[3], texts[20]):
            want = _check_replace(case, entries, data, prefilter, sides, monkeypatch, (7, 4096))
            plain = case.emu(data, prefilter, Boundary.NONE).replace(entries)
            assert 10 <= want.applied < plain.applied and want.out != plain.out
    # FuzzyReplacer.replace_stream takes the mask too
    data = ascii_texts()[3]
    _knobs(monkeypatch)
    out = io.BytesIO()
    reps = ["<ART>", "<CAT>", "<SMART>"]
    FuzzyReplacer(ascii_case.eng, reps).replace_stream(io.BytesIO(data), out, THR, prefilter=prefilter, boundaries=sides)
    assert out.getvalue() == ascii_case.emu(data, prefilter, sides).replace(reps).out


@pytest.fixture(scope="module")
def guard_case():
    return Case(PATTERNS, fixture_builder(), thr=0.8)


def test_replace_stream_guard_skips_across_a_task_boundary(guard_case, monkeypatch):
    """Mask END: "abcdefgh" before "efgh" is dropped, the records that remain still overlap across
    windows, and the cursor's guard skips one in the first window of a task."""
    c, sides = guard_case, Boundary.END
    data = ("z" * 36 + UNIT.replace("xx", "xé") * 100).encode()
    assert c.overlap == 10
    emu = c.emu(data, False, sides)
    tasks = _tasks(emu.wins, BATCH)
    first = [emu.wins.index(t[0]) for t in tasks[1:] if len(t) > 1]
    crossing = 0
    for k in first:  # the first window of a task whose record starts inside text the previous task wrote
        a = emu.replace(TABLE, emu.wins[:k])
        crossing += emu.replace(TABLE, emu.wins[k:k + 1], emitted=a.emitted).skipped
    assert crossing >= 1
    want = _check_replace(c, TABLE, data, False, sides, monkeypatch, (7, 4096))
    assert want.skipped >= crossing and want.applied > 100
    assert want.out != c.emu(data, False, Boundary.NONE).replace(TABLE).out


# ---------------------------------------------------------------- 6. feeding independence

@pytest.mark.parametrize("kind", ["ascii", "unicode"])
def test_feeding_and_task_size_do_not_change_the_rows(ascii_case, uni_cases, kind, monkeypatch):
    case, data = (ascii_case, ascii_texts()[11]) if kind == "ascii" else (_uni_case(uni_cases, "ci"), uni_texts(12)[11])
    want = case.emu(data, False, Boundary.WHOLE).rows()
    assert len(want) >= 20
    seen = []
    for batch in (BATCH, 1 << 25):
        for piece in (64, 1000, 4096):
            _knobs(monkeypatch, batch=batch)
            rows, counts = _search(case.eng, data, case.thr, False, Boundary.WHOLE, piece)
            assert counts == case.counts(case.emu(data, False, Boundary.WHOLE), batch)
            seen.append(rows)
    assert all(r == want for r in seen)


# ---------------------------------------------------------------- 7. off is off

def _open(eng, fn, *args):
    """A _Stream over a handle opened by `fn`."""
    h = ctypes.c_void_p()
    rc = fn(eng._h, *args, ctypes.byref(h))
    if rc:
        raise DeviceError(rc, _native.lib.fac_last_error().decode())
    st = _Stream.__new__(_Stream)
    st._h, st.engine = h, eng
    return st


def _feed_all(st, data):
    out = []
    ps = _pieces(data, 1000)
    for i, p in enumerate(ps):
        out += st.feed(p, eof=i == len(ps) - 1)
    return sorted(_rows(out)), st.windows_searched(), st.task_counts()


@PF
def test_off_is_off(ascii_case, uni_cases, prefilter, monkeypatch):
    lib = _native.lib
    for case, data in ((ascii_case, ascii_texts()[2]), (_uni_case(uni_cases, "ci"), uni_texts(3)[2])):
        _knobs(monkeypatch)
        eng, thr = case.eng, case.thr
        ex = _feed_all(_open(eng, lib.fac_stream_open_ex, f32(thr), WINDOW, int(prefilter)), data)
        o = _native.fac_stream_options(f32(thr), WINDOW, int(prefilter), 0)
        assert _feed_all(_open(eng, lib.fac_stream_open_opts, ctypes.byref(o)), data) == ex
        assert _feed_all(_Stream(eng, thr, WINDOW, prefilter=prefilter, boundaries=Boundary.NONE), data) == ex
        assert ex[0] == case.emu(data, prefilter, Boundary.NONE).rows() and len(ex[0]) >= 20
        table = ReplacementTable(eng, ["<A>", None, "C"])
        h = ctypes.c_void_p()
        assert lib.fac_replace_stream_open_ex(eng._h, table._h, f32(thr), WINDOW, int(prefilter), ctypes.byref(h)) == 0
        st = _ReplaceStream.__new__(_ReplaceStream)
        st._h, st.engine, st.table = h, eng, table
        old = st.feed(data, eof=True)
        assert _replace(eng, table, data, thr, prefilter, Boundary.NONE)[0] == old
    eng = ascii_case.eng
    for bad in (4, -1, 7):
        o = _native.fac_stream_options(f32(THR), WINDOW, 0, bad)
        h = ctypes.c_void_p()
        assert lib.fac_stream_open_opts(eng._h, ctypes.byref(o), ctypes.byref(h)) == _native.FAC_E_INVALID and not h
        assert lib.fac_replace_stream_open_opts(eng._h, table._h, ctypes.byref(o), ctypes.byref(h)) == _native.FAC_E_INVALID
        assert not h
    o = _native.fac_stream_options(f32(THR), WINDOW, 0, 3)
    assert lib.fac_stream_open_opts(eng._h, None, ctypes.byref(h)) == _native.FAC_E_INVALID
    assert lib.fac_stream_open_opts(None, ctypes.byref(o), ctypes.byref(h)) == _native.FAC_E_INVALID
    assert lib.fac_stream_open_opts(eng._h, ctypes.byref(o), None) == _native.FAC_E_INVALID
    assert lib.fac_replace_stream_open_opts(eng._h, None, ctypes.byref(o), ctypes.byref(h)) == _native.FAC_E_INVALID
    with pytest.raises(DeviceError) as ei:
        _Stream(eng, THR, WINDOW, boundaries=4)
    assert ei.value.code == _native.FAC_E_INVALID
    with pytest.raises(DeviceError) as ei:
        eng.search_stream(io.BytesIO(b"art"), THR, lambda m: None, boundaries=4)
    assert ei.value.code == _native.FAC_E_INVALID


# ---------------------------------------------------------------- 8. differential

DIFF_PIECES = ["art", "cat", "écol", "straße", "का", "é", "smart"]
_DIFF = {}


def _diff_case(ascii_only):
    if ascii_only not in _DIFF:
        rng = random.Random(77 + ascii_only)
        pool = [p for p in DIFF_PIECES if p.isascii()] if ascii_only else DIFF_PIECES
        _DIFF[ascii_only] = Case(rng.sample(pool, 3), _builder(bool(ascii_only)))
    return _DIFF[ascii_only]


def _diff_text(rng, case, ascii_only, size):
    """random_doc's pieces around planted patterns, one-edit variants included."""
    pats = [p.pattern for p in case.orc.patterns_]
    out = []
    while sum(len(x.encode()) for x in out) < size:
        doc = random_doc(rng, 1 + rng.next() % 4)
        if ascii_only:
            doc = "".join(ch for ch in doc if ch.isascii())
        out.append(doc)
        if rng.next() % 2:
            p = pats[rng.next() % len(pats)]
            out.append(p if rng.next() % 3 else p[:1] + p[2:])
    return "".join(out).encode()


@pytest.mark.parametrize("seed", range(8))
def test_differential(seed, monkeypatch):
    rng = Rng(0xD1FF + 977 * seed)
    ascii_only = seed % 2
    case = _diff_case(ascii_only)
    sides = SIDES[1 + rng.next() % 3]
    prefilter, read = bool(rng.next() % 2), (64, 128, 1000, 4096)[rng.next() % 4]
    data = _diff_text(rng, case, ascii_only, 3300 if read < 4096 else 9000)
    assert data.isascii() == bool(ascii_only)
    emu = case.check(monkeypatch, data, prefilter, sides, read=read, piece=(7, 4096)[seed % 2])
    assert len(emu.rows()) >= 5 and len(emu.wins) >= 2
    entries = ["<0>", None, Wrap("«", "»")]
    want = emu.replace(entries)
    if want.ties == 0:
        _check_replace(case, entries, data, prefilter, sides, monkeypatch, read=read)
