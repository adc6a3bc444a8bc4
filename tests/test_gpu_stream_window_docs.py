"""Streams whose tasks hold non-ASCII text: every task of more than one window is searched as one
device batch whose documents are the windows' texts (stream.cpp run_window_task, api.cpp
stream_windows_docs; the gather of the expanded text in stage_kernels.hip, the commit cut in
rank_kernels.hip).

Expected rows, output bytes and counts come from the CPU oracle through stream_emulation.stream_rows
and test_replace_stream_host.emulate_replace_stream; rows compare exactly, similarity bits and matched
text included. The streams run as tests/test_gpu_prefilter_stream.py runs them: FAC_STREAM_READ_BYTES
(the reader's read size) 64-4096, window_bytes 512 and tasks of FAC_STREAM_BATCH_BYTES = 2048 bytes, so
a few KiB of input give several windows a task and several tasks. FAC_STREAM_WINDOW_DOCS=0 turns the
path off (the windows of a non-ASCII task are then searched one by one), which is the A/B the
differential uses; task_counts() tells which way a task went."""
import ctypes
import random

import numpy as np
import pytest

from fuzzy_aho_corasick import FuzzyAhoCorasickBuilder as B, FuzzyLimits as L, HaystackTooLarge, _native
from fuzzy_aho_corasick.engine import ReplacementTable, Wrap, _ReplaceStream, _Stream
from oracle_harness import OracleEngine, graphemes
from stream_emulation import stream_rows
from test_gpu_batch_prefilter import PACKED_PATS, PACKED_THR, packed_builder
from test_gpu_prefilter_stream import ASCII_GEN, UNI_GEN, _count, _covered, _generate, _rows, _tasks
from test_replace_stream_host import PATTERNS, TABLE, UNIT, emulate_replace_stream, fixture_builder, reader_windows

pytestmark = pytest.mark.gpu

THR = 0.8
WINDOW, READ, BATCH = 512, 128, 2048


def _builder(ci=True):
    return B().fuzzy(L().edits(1)).case_insensitive(ci)


def _knobs(monkeypatch, read=READ, batch=BATCH, docs=True):
    monkeypatch.setenv("FAC_STREAM_READ_BYTES", str(read))
    monkeypatch.setenv("FAC_STREAM_BATCH_BYTES", str(batch))
    if docs:
        monkeypatch.delenv("FAC_STREAM_WINDOW_DOCS", raising=False)
    else:
        monkeypatch.setenv("FAC_STREAM_WINDOW_DOCS", "0")


def _pieces(data, piece):
    return [data[i:i + piece] for i in range(0, len(data), piece)] or [b""]


def _search(eng, data, thr, prefilter, piece=4096):
    """(rows, windows_searched, task_counts) of a search stream fed in `piece`-byte pieces."""
    st = _Stream(eng, thr, WINDOW, prefilter=prefilter)
    out, ps = [], _pieces(data, piece)
    for i, p in enumerate(ps):
        out += st.feed(p, eof=i == len(ps) - 1)
    assert st.total() == len(data)
    return sorted(_rows(out)), st.windows_searched(), st.task_counts()


def _replace(eng, table, data, thr, prefilter, piece=4096):
    st = _ReplaceStream(eng, table, thr, WINDOW, prefilter=prefilter)
    out, ps = bytearray(), _pieces(data, piece)
    for i, p in enumerate(ps):
        out += st.feed(p, eof=i == len(ps) - 1)
    assert st.written() == len(out)
    return bytes(out), st.counts(), st.windows_searched(), st.task_counts()


class Case:
    """An engine, its oracle and a text: the reader's windows, the tasks and the oracle's replay."""

    def __init__(self, pats, data, builder=None, thr=THR, read=READ, batch=BATCH):
        b = builder or _builder()
        self.thr, self.data, self.read, self.batch = thr, data, read, batch
        self.eng, self.orc = b.device(0).build(pats), OracleEngine(b, pats)
        self.overlap = self.eng.max_match_graphemes() + 1
        self.wins = reader_windows(data, self.overlap, WINDOW, read)
        self.texts = [data[b0:e0].decode() for b0, e0, _ in self.wins]
        self.tasks = _tasks(self.wins, batch)
        self._want = {}

    def want(self, prefilter):
        if prefilter not in self._want:
            orc = self.orc.with_prefilter() if prefilter else self.orc
            self._want[prefilter] = sorted(stream_rows(orc, self.data, self.thr, self.overlap, window=WINDOW,
                                                       chunk=self.read))
        return self._want[prefilter]

    def searched(self, prefilter):
        """windows_searched() of the window-by-window path: every window's graphemes (bytes where its
        text is ASCII), or with the filter the lengths of its merged windows."""
        if prefilter and self.orc.with_prefilter().is_active() and \
                self.orc.prefilter_windows(self.texts[0], self.thr) is not None:
            return sum(self._covered(t) for t in self.texts)
        return sum(_count(t) for t in self.texts)

    def _covered(self, text):
        """The start windows of a text's merged windows, each searched as a haystack of its own: an ASCII
        slice of a non-ASCII text is searched byte by byte (search.rs:196), so its CRLF counts twice."""
        if text.isascii():
            return _covered(self.orc, text, self.thr)
        gs = graphemes(text)
        slices = ["".join(gs[s:min(e, len(gs))]) for s, e in self.orc.prefilter_windows(text, self.thr)]
        return sum(_count(sl) for sl in slices)

    def counts(self, docs=True, ascii_batched=True):
        """task_counts(): every task of several windows is batched; with the path off only the all-ASCII
        ones that the union path takes (ascii_batched)."""
        multi = [t for t in self.tasks if len(t) > 1]
        if not docs:
            multi = [t for t in multi if ascii_batched and self.data[t[0][0]:t[-1][1]].isascii()]
        return len(multi), len(self.tasks) - len(multi)

    def check(self, monkeypatch, prefilter, piece=4096, ascii_batched=True):
        _knobs(monkeypatch, self.read, self.batch)
        got = _search(self.eng, self.data, self.thr, prefilter, piece)
        assert got[0] == self.want(prefilter)
        assert got[1:] == (self.searched(prefilter), self.counts())
        _knobs(monkeypatch, self.read, self.batch, docs=False)
        off = _search(self.eng, self.data, self.thr, prefilter, piece)
        assert off[:2] == got[:2]
        # an all-ASCII task: the union path takes it unless the filter's tables need the packed full scan
        # (the engine's tables decide, for all of its tasks alike)
        union, declined = self.counts(False, True), self.counts(False, False)
        assert off[2] in ((union,) if not prefilter else (declined,) if not ascii_batched else (union, declined))
        return got


# ---------------------------------------------------------------- the expanded text

def _gather(eng, text, wins):
    flat = (ctypes.c_uint64 * (2 * len(wins)))(*[x for w in wins for x in w])
    total = sum(n for _, n in wins)
    out = np.full(total + 64, 0xAA, dtype=np.uint8)
    offs = (ctypes.c_uint64 * (len(wins) + 1))()
    rc = _native.lib.fac_diag_stream_gather(eng._h, text, len(text), flat, len(wins), out.ctypes.data, total, offs)
    assert rc == 0
    assert (out[total:] == 0xAA).all()  # nothing written past the expanded length
    return out[:total].tobytes(), list(offs)


def test_gather_alignment():
    """Window offsets and lengths 0-15 modulo 16, overlaps shorter and longer than 16 bytes, windows
    shorter than a lane's 16 bytes, empty windows, windows of several 4096-byte tiles, and a window that
    ends with the text (no read may pass it)."""
    eng = _builder().device(0).build(["needle"])
    rng = random.Random(3)
    for tail in range(0, 20):
        text = bytes(rng.randrange(1, 256) for _ in range(20000 + tail))
        wins, off = [], 0
        for k in range(256):
            n = (k % 16) + 16 * rng.choice([0, 0, 1, 2, 40, 300]) if k % 7 else rng.choice([0, 1, 5, 15])
            off = min(off, len(text) - n)
            wins.append((off, n))
            off = max(0, off + n - rng.choice([0, 3, 15, 16, 17, 40]))  # the next window starts inside this one
            off += (k // 16 - off) % 16  # its offset modulo 16 takes every value
            if off > len(text) - 5000:
                off = rng.randrange(0, 16)
        wins += [(len(text) - 4321, 4321), (len(text) - 16, 16), (len(text) - 1, 1), (len(text), 0), (0, len(text))]
        if tail == 0:
            assert {o % 16 for o, _ in wins} == set(range(16)) == {n % 16 for _, n in wins}
        got, offs = _gather(eng, text, wins)
        want_offs = [0]
        for _, n in wins:
            want_offs.append(want_offs[-1] + n)
        assert offs == want_offs
        assert got == b"".join(text[o:o + n] for o, n in wins), tail
    assert _gather(eng, b"", [(0, 0), (0, 0)]) == (b"", [0, 0, 0])
    assert _native.lib.fac_diag_stream_gather(eng._h, b"abc", 3, (ctypes.c_uint64 * 2)(2, 2), 1, None, 0,
                                              (ctypes.c_uint64 * 2)()) == _native.FAC_E_INVALID


# ---------------------------------------------------------------- search streams

@pytest.fixture(scope="module")
def uni():
    return {ci: Case(UNI_GEN[0], _generate(UNI_GEN[1], UNI_GEN[2], words=1000).encode(), _builder(ci)) for ci in (True, False)}


@pytest.mark.parametrize("prefilter", [False, True], ids=["plain", "prefiltered"])
@pytest.mark.parametrize("ci", [True, False], ids=["ci", "cs"])
def test_all_unicode_text(uni, ci, prefilter, monkeypatch):
    """Fails without the window-documents path: task_counts() does not exist there, and with the path
    off every task of this text is counted under `single`."""
    c = uni[ci]
    assert not c.data.isascii() and len(c.wins) >= 5 and len(c.want(prefilter)) >= 20
    assert c.counts()[0] >= 3 and c.counts(False) == (0, len(c.tasks))
    if prefilter:
        assert c.searched(True) < c.searched(False)
    c.check(monkeypatch, prefilter)
    c.check(monkeypatch, prefilter, piece=7)


def test_reads_of_4096_bytes(monkeypatch):
    """The reader's windows are whole reads: 4096-byte windows, three to a task of 9000 bytes."""
    c = Case(UNI_GEN[0], _generate(UNI_GEN[1], UNI_GEN[2], words=2600).encode(), read=4096, batch=9000)
    assert len(c.wins) >= 4 and c.counts()[0] >= 2 and max(len(t) for t in c.tasks) >= 3
    c.check(monkeypatch, False)
    c.check(monkeypatch, True, piece=7)


def _ascii_with_one(where):
    """ASCII text whose only non-ASCII character lies in the first / a middle / the last window of a
    task of at least three windows."""
    base = _generate(ASCII_GEN[1], ASCII_GEN[2], words=1000).encode()
    wins = reader_windows(base, 11, WINDOW, READ)
    task = next(t for t in _tasks(wins, BATCH)[1:-1] if len(t) >= 3)
    win = task[{"first": 0, "middle": len(task) // 2, "last": -1}[where]]
    # past the previous window's end, before the next one's start
    p = next(q for q in range(win[0] + 200, win[0] + 300) if base[q:q + 2].isalpha())
    return base[:p] + "é".encode() + base[p + 1:], p


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("prefilter", [False, True], ids=["plain", "prefiltered"])
def test_ascii_text_with_one_non_ascii_character(where, prefilter, monkeypatch):
    data, p = _ascii_with_one(where)
    c = Case(ASCII_GEN[0], data)
    assert c.overlap == 11
    holders = [(ti, wi) for ti, t in enumerate(c.tasks) for wi, w in enumerate(t) if w[0] <= p < w[1]]
    (ti, wi), = holders  # one window of one task holds it
    task = c.tasks[ti]
    assert len(task) >= 3 and wi == {"first": 0, "middle": len(task) // 2, "last": len(task) - 1}[where]
    assert [data[w[0]:w[1]].isascii() for w in task] == [i != wi for i in range(len(task))]
    assert len(c.want(prefilter)) >= 30
    assert c.counts(False) == (c.counts()[0] - 1, c.counts()[1] + 1)  # that task alone changes sides
    c.check(monkeypatch, prefilter)


E_RUN = "e" + "́̂̃" * 9  # one grapheme of 55 bytes
FLAGS = "\U0001F1E9\U0001F1EA" * 7 + "\U0001F1E9"  # a regional-indicator run of odd length
FAMILY = "\U0001F468‍\U0001F469‍\U0001F467‍\U0001F466"
CLUSTER_SEPS = [" ", "\r\n", " " + E_RUN + " ", " " + FLAGS + " ", FAMILY, "\r\n\r\n", " é ", E_RUN + FAMILY]


def _cluster_text(seed=5, words=260):
    rng = random.Random(seed)
    _, fillers, hits = UNI_GEN
    out = []
    for i in range(words):
        out.append(rng.choice(hits) if i % 9 == 8 else rng.choice(fillers))
        out.append(rng.choice(CLUSTER_SEPS))
    return "".join(out).encode()


def _boundaries(data):
    s, off = set(), 0
    for g in graphemes(data.decode()):
        s.add(off)
        off += len(g.encode())
    return s | {off}


@pytest.mark.parametrize("prefilter", [False, True], ids=["plain", "prefiltered"])
def test_cuts_inside_clusters(prefilter, monkeypatch):
    """Long combining runs, regional-indicator runs, ZWJ sequences and CRLF: window texts begin and end
    inside clusters of the whole text, and multi-byte characters are split across feeds."""
    data = _cluster_text()
    c = Case(UNI_GEN[0], data, read=64)
    bounds = _boundaries(data)
    assert sum(1 for w in c.wins if w[1] not in bounds) >= 3  # a window's text ends inside a cluster
    ends = {w[1] for w in c.wins[:-1]}
    assert any(data[e] & 0xC0 == 0x80 for e in range(64, len(data), 64) if e not in ends)  # a read edge inside a character
    assert len(c.want(prefilter)) >= 15 and c.counts()[0] >= 3
    for piece in (1, 7, 4096):
        c.check(monkeypatch, prefilter, piece)


def test_window_that_owns_one_grapheme_and_last_window(monkeypatch):
    g = "e" + "́" * 28  # 57 bytes: nine graphemes a window, the overlap is eight
    data = ((g * 25 + " needle ") * 3).encode()
    c = Case(["needle"], data, fixture_builder())
    assert c.overlap == 8
    owned = [len(graphemes(data[b0:b0 + cm].decode())) for b0, _, cm in c.wins]
    inside = [n for t in c.tasks if len(t) > 1 for n in owned[c.wins.index(t[0]):c.wins.index(t[-1]) + 1]]
    assert 1 in inside
    assert len(c.tasks[-1]) > 1 and c.wins[-1][1] == len(data) and c.wins[-1][2] == c.wins[-1][1] - c.wins[-1][0]
    assert len(c.want(False)) >= 2
    for prefilter in (False, True):
        c.check(monkeypatch, prefilter)


def test_engine_with_multi_character_mappings(monkeypatch):
    b = _builder().mapping("ss", "ß").mapping("ae", "æ")
    pats = UNI_GEN[0] + ["kaese", "fußball"]
    data = _generate(UNI_GEN[1], UNI_GEN[2] + ["käse", "kæse", "fussball", "Fußbal", "strase"]).encode()
    c = Case(pats, data, b)
    assert not c.eng.with_prefilter().is_active() and not c.orc.with_prefilter().is_active()
    rows = c.want(False)
    assert len(rows) >= 30 and {"kæse", "fussball", "strasse"} <= {r[4] for r in rows}
    plain = c.check(monkeypatch, False)
    assert c.check(monkeypatch, True) == plain  # no filter: the pre-filtered stream is the plain one


@pytest.mark.parametrize("prefilter", [False, True], ids=["plain", "prefiltered"])
def test_auto_beam_engine(prefilter, monkeypatch):
    c = Case(UNI_GEN[0], _generate(UNI_GEN[1], UNI_GEN[2]).encode(), _builder().auto_beam(40, 8))
    assert len(c.want(prefilter)) >= 30
    c.check(monkeypatch, prefilter)


def test_fallback_threshold_on_ascii_text(monkeypatch):
    """No edit limits and a long pattern: k_for > 24 at this threshold, the reference searches in full
    and the union path takes the task."""
    pats = ASCII_GEN[0] + ["the quick brown fox jumps over the lazy dog"]
    c = Case(pats, _generate(ASCII_GEN[1], ASCII_GEN[2]).encode(), B().case_insensitive(True), thr=0.7)
    assert c.orc.with_prefilter().is_active() and c.orc.prefilter_windows(c.data.decode(), 0.7) is None
    assert len(c.want(True)) >= 20 and c.want(True) == c.want(False)
    assert c.check(monkeypatch, True) == c.check(monkeypatch, False)


def test_packed_full_scan_tables_on_ascii_text(monkeypatch):
    """Pre-filter tables that need the packed full scan: the union path declines the task, which goes
    to the window documents (before: window by window)."""
    rng = random.Random(9)
    words = [rng.choice(PACKED_PATS + ["helo", "wrld", "sadam"]) if i % 10 == 9 else rng.choice(["zq0", "qqzz", "0z0z"])
             for i in range(900)]
    c = Case(PACKED_PATS, " ".join(words).encode(), packed_builder(), thr=PACKED_THR)
    assert c.data.isascii() and len(c.want(True)) >= 30 and c.searched(True) < c.searched(False)
    c.check(monkeypatch, True, ascii_batched=False)
    c.check(monkeypatch, False)  # without the filter the union path takes it, as before


def test_record_buffer_regrows_and_windows_without_records(monkeypatch):
    """A task of about 8 KiB where a one-character pattern hits nearly everywhere: more raw records
    than the search's first device buffer holds (4096), and windows that own none."""
    data = ("e" * 3000 + "é" + "e" * 500 + "z" * 2200 + "é" + "e" * 3000).encode()
    c = Case(["e"], data, B(), thr=0.9, batch=8192)
    assert len(c.tasks) >= 2 and len(c.tasks[0]) > 8
    first = c.wins[:len(c.tasks[0])]
    assert sum(len(c.orc.raw_rows(data[b0:e0].decode(), 0.9)) for b0, e0, _ in first) > 4096
    want = c.want(False)
    assert sum(1 for b0, _, cm in first if not any(b0 <= r[0] < b0 + cm for r in want)) >= 2
    c.check(monkeypatch, False)
    c.check(monkeypatch, True)


# ---------------------------------------------------------------- replace streams

def _check_replace(c, entries, monkeypatch, prefilter, pieces=(4096,)):
    orc = c.orc.with_prefilter() if prefilter else c.orc
    want = emulate_replace_stream(orc, c.data, entries, c.thr, overlap=c.overlap, window=WINDOW, read=c.read)
    assert want.ties == 0 and [w[:2] for w in want.windows] == [w[:2] for w in c.wins]
    table = ReplacementTable(c.eng, entries)
    expect = (want.out, (want.applied, want.skipped), c.searched(prefilter))
    for piece in pieces:
        _knobs(monkeypatch, c.read, c.batch)
        assert _replace(c.eng, table, c.data, c.thr, prefilter, piece) == expect + (c.counts(),), piece
    _knobs(monkeypatch, c.read, c.batch, docs=False)
    assert _replace(c.eng, table, c.data, c.thr, prefilter)[:3] == expect
    return want


@pytest.mark.parametrize("prefilter", [False, True], ids=["plain", "prefiltered"])
def test_replace_stream_unicode(uni, prefilter, monkeypatch):
    c = uni[True]
    want = _check_replace(c, ["NADEL", None, Wrap("[", "]"), "", "ß→ss"], monkeypatch, prefilter, (1, 7, 4096))
    assert want.applied >= 30
    want.out.decode("utf-8")


def test_replace_stream_keep_table_copies_the_input(uni, monkeypatch):
    for data in (uni[True].data, _cluster_text()):
        c = Case(UNI_GEN[0], data, read=64)
        want = _check_replace(c, [None] * 5, monkeypatch, False)
        assert want.out == data and want.applied >= 15


def test_replace_stream_one_non_ascii_character_and_clusters(monkeypatch):
    c = Case(ASCII_GEN[0], _ascii_with_one("middle")[0])
    assert _check_replace(c, ["<N>", None, Wrap("«", "»")], monkeypatch, True).applied >= 30
    c = Case(UNI_GEN[0], _cluster_text(), read=64)
    assert _check_replace(c, ["NADEL", None, Wrap("[", "]"), "", "X"], monkeypatch, False, (7, 4096)).applied >= 15


def test_replace_stream_guard_skips_across_a_task_boundary(monkeypatch):
    data = ("z" * 36 + UNIT.replace("xx", "xé") * 100).encode()
    c = Case(PATTERNS, data, fixture_builder())
    assert c.overlap == 10 and not data.isascii()
    first = [c.wins.index(t[0]) for t in c.tasks[1:] if len(t) > 1]
    crossing = 0
    for k in first:  # the first window of a task whose record starts inside text the previous task wrote
        a = emulate_replace_stream(c.orc, data, TABLE, THR, windows=c.wins[:k])
        crossing += emulate_replace_stream(c.orc, data, TABLE, THR, windows=c.wins[k:k + 1], emitted=a.emitted).skipped
    assert crossing >= 1
    want = _check_replace(c, TABLE, monkeypatch, False, (7, 4096))
    assert want.skipped >= crossing and want.applied > 100
    _check_replace(c, TABLE, monkeypatch, True)


# ---------------------------------------------------------------- differential

TEXT_KINDS = ["unicode", "one", "clusters", "ascii"]
ENGINE_KINDS = {
    "ci": lambda: (UNI_GEN[0], _builder(True)),
    "cs": lambda: (UNI_GEN[0], _builder(False)),
    "map": lambda: (UNI_GEN[0], _builder().mapping("ss", "ß").mapping("ae", "æ")),
    "beam": lambda: (UNI_GEN[0], _builder().auto_beam(40, 8)),
    "packed": lambda: (PACKED_PATS + ["straße"], packed_builder()),
}
_ENGINES = {}


def _random_text(kind, rng):
    _, fillers, hits = UNI_GEN
    hits = hits + ["helo", "wrld", "hussein8"]
    if kind in ("one", "ascii"):
        fillers, hits = [w for w in fillers if w.isascii()], [w for w in hits if w.isascii()]
    seps = CLUSTER_SEPS if kind == "clusters" else [" "]
    words = []
    for i in range(rng.randrange(250, 450)):
        words += [rng.choice(hits) if i % 10 == 9 else rng.choice(fillers), rng.choice(seps)]
    text = "".join(words)
    if kind == "one":
        p = rng.randrange(len(text))
        text = text[:p] + "ö" + text[p + 1:]
    return text.encode()


def _drawn_case(ek, data, read):
    """A Case over one of the shared engines (built once per kind)."""
    if ek not in _ENGINES:
        pats, b = ENGINE_KINDS[ek]()
        _ENGINES[ek] = (pats, b, b.device(0).build(pats), OracleEngine(b, pats))
    pats, b, eng, orc = _ENGINES[ek]
    c = Case.__new__(Case)
    c.thr, c.data, c.read, c.batch, c.eng, c.orc, c._want = (PACKED_THR if ek == "packed" else THR), data, read, BATCH, eng, orc, {}
    c.overlap = eng.max_match_graphemes() + 1
    c.wins = reader_windows(data, c.overlap, WINDOW, read)
    c.texts = [data[b0:e0].decode() for b0, e0, _ in c.wins]
    c.tasks = _tasks(c.wins, BATCH)
    assert len(c.wins) >= 3
    return c


@pytest.mark.parametrize("seed", range(40))
def test_differential(seed, monkeypatch):
    """Text kind, engine kind, pre-filter and piece size drawn from the seed: the window-documents
    path, the path turned off and the emulation give the same rows and windows_searched()."""
    rng = random.Random(1000 + seed)
    kind = TEXT_KINDS[seed % 4]
    ek = list(ENGINE_KINDS)[(seed // 4) % 5]
    prefilter, piece, read = rng.random() < 0.5, rng.choice([1, 7, 4096]), rng.choice([64, 128, 256])
    c = _drawn_case(ek, _random_text(kind, rng), read)
    c.check(monkeypatch, prefilter, piece, ascii_batched=not (ek == "packed" and prefilter))


@pytest.mark.parametrize("seed", range(8))
def test_differential_replace(seed, monkeypatch):
    """The same draws through replace streams with plain, keep, template and empty entries: the output
    bytes, the (applied, skipped) counts and windows_searched() of the window-documents path, of the
    path turned off and of the emulation agree."""
    rng = random.Random(2000 + seed)
    kind = TEXT_KINDS[seed % 4]
    ek = ("ci", "cs")[(seed // 4) % 2]
    prefilter, piece, read = seed % 2 == 1, rng.choice([1, 7, 4096]), rng.choice([64, 128, 256])
    c = _drawn_case(ek, _random_text(kind, rng), read)
    _check_replace(c, ["NADEL", None, Wrap("[", "]"), "", "X"], monkeypatch, prefilter, (piece,))


# ---------------------------------------------------------------- errors

def test_window_over_the_grapheme_limit(uni, monkeypatch):
    """A window over the limit fails the stream with the window-by-window path's return code
    (FAC_E_HAYSTACK_TOO_LARGE, raised as HaystackTooLarge) on both paths, plain and pre-filtered. The
    return code is all a stream reports: fac_stream_feed has no channel for a grapheme count, so the
    exception's `graphemes` is 0 whichever path failed, and the comparison of it below pins only that
    neither path invents one."""
    c = uni[True]
    assert min(_count(t) for t in c.texts[:-1]) > 100
    monkeypatch.setenv("FAC_GRAPHEME_LIMIT", "100")
    seen = []
    for docs in (True, False):
        _knobs(monkeypatch, docs=docs)
        for prefilter in (False, True):
            with pytest.raises(HaystackTooLarge) as ei:
                _search(c.eng, c.data, c.thr, prefilter)
            seen.append((type(ei.value), ei.value.graphemes))
    assert set(seen) == {(HaystackTooLarge, 0)}
