"""Streaming replace on the device: fac_replace_windows_staged_device (the plan of one long document
and the one-document copy, replace_kernels.hip) and fac_replace_stream_* (stream.cpp's replace mode),
against the crate's semantics (stream.rs:465-517 + ReplaceCursor::emit_window, :645-705) replayed on
the CPU oracle by test_replace_stream_host.emulate_replace_stream. Two kept records of one window
share a start only if one is an empty span (matches.rs:93-99), which no pattern of three or more
graphemes produces under edits(1): every case asserts the emulator saw no such tie."""
import io

import pytest

from fuzzy_aho_corasick import _native
from fuzzy_aho_corasick.engine import (DeviceError, FuzzyReplacer, ReplacementTable, StagedHaystack, Wrap,
                                       _ReplaceStream)
from oracle_harness import OracleEngine
from test_replace_stream_host import (OVERLAP, PATTERNS, TABLE, THRESHOLD, UNIT, emulate_replace_stream,
                                      fixture_builder, reader_windows, strided_windows)

pytestmark = pytest.mark.gpu


class Fixture:
    def __init__(self, patterns=PATTERNS):
        b = fixture_builder().device(0)
        self.eng, self.orc = b.build(patterns), OracleEngine(b, patterns)
        self._tables, self._staged = {}, {}

    def table(self, entries):
        key = tuple(entries)
        if key not in self._tables:
            self._tables[key] = ReplacementTable(self.eng, entries)
        return self._tables[key]

    def staged(self, data: bytes):
        if data not in self._staged:
            starts = _native.grapheme_starts(data) if not data.isascii() else None
            g_of = None if starts is None else {int(b): g for g, b in enumerate(list(starts) + [len(data)])}
            self._staged[data] = (StagedHaystack(self.eng, data), g_of)
        return self._staged[data]

    def emulate(self, data, entries, **kw):
        r = emulate_replace_stream(self.orc, data, entries, THRESHOLD, **kw)
        assert r.ties == 0
        return r

    def run(self, data, wins, entries, prefilter=False, emitted=0, shift=0, cap=None, fill=None):
        """fac_replace_windows_staged_device over byte windows (first, end, commit) of `data`, staged at
        stream offset `shift`: (output bytes, cursor, applied, skipped)."""
        import torch
        st, g_of = self.staged(data)
        g = (lambda b: b) if g_of is None else (lambda b: g_of[b])
        tuples = [(g(b), g(e), c, shift + b) for (b, e, c) in wins]
        out = torch.empty(2 * len(data) + 4096 if cap is None else cap, dtype=torch.uint8, device="cuda")
        if fill is not None:
            out.fill_(fill)
        self.last_out = out
        got, em, na, ns, _ = st.replace_windows_device(tuples, self.table(entries), THRESHOLD, prefilter, out,
                                                       emitted=emitted)
        return bytes(got.cpu().numpy().tobytes()), em, na, ns


@pytest.fixture(scope="module")
def fx():
    return Fixture()


def _check(fx, data, wins, entries, want, **kw):
    got = fx.run(data, wins, entries, **kw)
    assert got == (want.out, want.emitted, want.applied, want.skipped), (got[1:], want[1:6])


# ---- 1. the carry passes whole windows (windows overlap beyond their neighbours: the per-window path)

@pytest.mark.parametrize("step,size", [(2, 30), (3, 40), (5, 25)])
def test_carry_passes_whole_windows(fx, step, size):
    data = (UNIT * 6).encode()
    wins = strided_windows(len(data), size, step)
    assert wins[0][1] >= wins[2][0]  # not a batch of stream_windows_batch
    want = fx.emulate(data, TABLE, windows=wins)
    assert want.skipped > 0 and want.chain > 0
    if (step, size) == (2, 30):
        assert (len(wins), want.applied, want.skipped, want.chain, len(want.out)) == (154, 42, 23, 72, 192)
    _check(fx, data, wins, TABLE, want)
    # the staged text at another stream offset: only the cursor moves
    got = fx.run(data, wins, TABLE, emitted=1000, shift=1000)
    assert got == (want.out, want.emitted + 1000, want.applied, want.skipped)


def test_more_windows_than_one_round_of_the_carry_chain(fx):
    """stream_carry_kernel walks the windows 256 at a time: more than 256 windows on both paths, the
    cursor past the commit point (per-window path) or a crossing record (batched path) at the seam."""
    data = ("-" + UNIT * 12).encode()
    wins = strided_windows(len(data), 30, 2)
    want = fx.emulate(data, TABLE, windows=wins)
    assert len(wins) > 300 and want.chain > 100 and want.skipped > 40
    assert fx.emulate(data, TABLE, windows=wins[:256]).emitted > wins[255][0] + wins[255][2]  # carried into round 2
    _check(fx, data, wins, TABLE, want)
    data = (UNIT * 80).encode()
    wins = reader_windows(data, OVERLAP, 24, 8)
    assert all(wins[w - 2][1] < wins[w][0] for w in range(2, len(wins)))
    want = fx.emulate(data, TABLE, windows=wins)
    assert len(wins) > 270 and want.skipped == 80
    assert fx.emulate(data, TABLE, windows=wins[:256]).emitted > wins[255][0] + wins[255][2]
    _check(fx, data, wins, TABLE, want)


# ---- 2. reader-shaped windows (each overlaps only its neighbours: the batched ASCII path)

@pytest.mark.parametrize("prefilter", [False, True])
@pytest.mark.parametrize("window,read,n_windows,skipped", [(24, 8, 140, 40), (32, 16, None, 20), (33, 7, None, 0)])
def test_reader_windows_batched(fx, window, read, n_windows, skipped, prefilter):
    data = (UNIT * 40).encode()
    wins = reader_windows(data, OVERLAP, window, read)
    assert all(wins[w - 2][1] < wins[w][0] for w in range(2, len(wins)))  # a batch of stream_windows_batch
    want = fx.emulate(data, TABLE, windows=wins)
    assert want.skipped == skipped and (n_windows is None or len(wins) == n_windows)
    _check(fx, data, wins, TABLE, want, prefilter=prefilter)
    # E_in > 0: the list in two calls, the cursor carried; one cut in the middle, and (where there is
    # one) one right after a window whose last record crosses its commit point
    cuts = [len(wins) // 2]
    for w in range(len(wins) - 1):
        a = fx.emulate(data, TABLE, windows=wins[:w + 1])
        if a.emitted > wins[w][0] + wins[w][2]:
            cuts.append(w + 1)
            break
    assert skipped == 0 or len(cuts) == 2
    for cut in cuts:
        a = fx.emulate(data, TABLE, windows=wins[:cut])
        b = fx.emulate(data, TABLE, windows=wins[cut:], emitted=a.emitted)
        assert a.out + b.out == want.out
        _check(fx, data, wins[:cut], TABLE, a, prefilter=prefilter)
        _check(fx, data, wins[cut:], TABLE, b, prefilter=prefilter, emitted=a.emitted)


# ---- 3. output alignment: pieces and gaps of 0-17 bytes, more than two 4096-byte tiles, template,
# keep, and a Unicode text whose byte offsets are not grapheme indices

def _gaps_text():
    return ("".join("abcdefgh" + "-" * g for g in range(18)) * 30).encode()


@pytest.mark.parametrize("rep_len", range(18))
def test_piece_and_gap_boundaries_at_every_offset(fx, rep_len):
    data = _gaps_text()
    wins = reader_windows(data, OVERLAP, 64, 16)
    entries = ["0123456789abcdefg"[:rep_len], "", None]
    want = fx.emulate(data, entries, windows=wins)
    assert want.applied >= 18 * 30
    if rep_len == 17:
        assert len(want.out) > 2 * _native.REPLACE_TILE
    _check(fx, data, wins, entries, want)


@pytest.mark.parametrize("entries", [[Wrap("[", "]"), None, "0123456789abcdefg"], [None, Wrap("<<", ""), Wrap("", "!")]])
def test_template_and_keep_entries(fx, entries):
    data = (UNIT * 40).encode()
    for wins in (reader_windows(data, OVERLAP, 24, 8), strided_windows(len(data), 30, 7)):
        want = fx.emulate(data, entries, windows=wins)
        assert want.applied > 100
        _check(fx, data, wins, entries, want)


def test_unicode_text():
    fu = Fixture(["straße", "aße", "москва", "école"])  # ("aße": found again by a window cut inside "Straße")
    data = ("die Straße nach Москва 🇩🇪 strasse école " * 12).encode()
    starts = [int(b) for b in _native.grapheme_starts(data)] + [len(data)]
    n = len(starts) - 1
    assert n < len(data)
    wins, g = [], 0
    while g + 24 < n:  # 24 graphemes cut 9 apart
        wins.append((starts[g], starts[g + 24], starts[g + 9] - starts[g]))
        g += 9
    wins.append((starts[g], len(data), len(data) - starts[g]))
    for entries in (["STRASSE", "?", None, Wrap("[", "]")], [Wrap("«", "»"), None, "", "É"]):
        want = fu.emulate(data, entries, windows=wins)
        assert want.applied >= 24 and want.skipped > 0
        want.out.decode("utf-8")
        _check(fu, data, wins, entries, want)


# ---- 4. FAC_E_OUTPUT_CAPACITY

def test_output_capacity(fx):
    data = (UNIT * 6).encode()
    wins = strided_windows(len(data), 30, 2)
    want = fx.emulate(data, TABLE, windows=wins)
    with pytest.raises(DeviceError) as ei:
        fx.run(data, wins, TABLE, cap=len(want.out) - 1, fill=0xAB, emitted=0)
    assert ei.value.code == _native.FAC_E_OUTPUT_CAPACITY
    assert ei.value.needed == len(want.out) and ei.value.emitted == 0
    assert bool((fx.last_out == 0xAB).all())
    _check(fx, data, wins, TABLE, want, cap=len(want.out), fill=0xAB)
    # the same with a cursor that is not 0
    a = fx.emulate(data, TABLE, windows=wins[:50])
    b = fx.emulate(data, TABLE, windows=wins[50:], emitted=a.emitted)
    with pytest.raises(DeviceError) as ei:
        fx.run(data, wins[50:], TABLE, cap=len(b.out) - 1, fill=0xAB, emitted=a.emitted)
    assert (ei.value.needed, ei.value.emitted) == (len(b.out), a.emitted) and bool((fx.last_out == 0xAB).all())


def test_window_bases_must_agree(fx):
    data = (UNIT * 6).encode()
    import torch
    st, _ = fx.staged(data)
    out = torch.empty(4096, dtype=torch.uint8, device="cuda")
    with pytest.raises(DeviceError) as ei:
        st.replace_windows_device([(0, 30, 2, 0), (2, 32, 2, 3)], fx.table(TABLE), THRESHOLD, False, out)
    assert ei.value.code == _native.FAC_E_INVALID


# ---- 5. the stream API

BIG = ((UNIT + "the quick brown fox ") * 5000).encode()
BIG_UNICODE = ((UNIT + "the quick brown fox école Москва ") * 2500).encode()
_EMULATED = {}


def _emulated(fx, data, window):
    key = (data, window)
    if key not in _EMULATED:
        _EMULATED[key] = fx.emulate(data, TABLE, overlap=fx.eng.max_match_graphemes() + 1, window=window)
    return _EMULATED[key]


def _stream(fx, data, piece, window, entries=TABLE, eof_alone=False):
    st = _ReplaceStream(fx.eng, fx.table(entries), THRESHOLD, window)
    out = bytearray()
    pieces = [data[i:i + piece] for i in range(0, len(data), piece)] or [b""]
    for i, p in enumerate(pieces):
        out += st.feed(p, eof=not eof_alone and i == len(pieces) - 1)
    if eof_alone:
        out += st.feed(b"", eof=True)
    assert st.written() == len(out)
    return bytes(out), st.counts()


@pytest.mark.parametrize("knob", [None, "65536"])
@pytest.mark.parametrize("window,n_windows", [(64 << 10, 6), (100_003, 4)])
def test_stream_api(fx, monkeypatch, window, n_windows, knob):
    assert fx.eng.max_match_graphemes() + 1 == OVERLAP
    if knob:  # every window a task of its own: the skipped records lie behind task boundaries
        monkeypatch.setenv("FAC_STREAM_BATCH_BYTES", knob)
    want = _emulated(fx, BIG, window)
    assert (len(BIG), len(want.windows), want.skipped) == (380_000, n_windows, 2)
    for piece in (1 << 20, 4099, 7):
        got, counts = _stream(fx, BIG, piece, window)
        assert got == want.out, piece
        assert counts == (want.applied, want.skipped)


@pytest.mark.parametrize("knob", [None, "65536"])
def test_stream_api_unicode(fx, monkeypatch, knob):
    if knob:
        monkeypatch.setenv("FAC_STREAM_BATCH_BYTES", knob)
    want = _emulated(fx, BIG_UNICODE, 64 << 10)
    assert len(want.windows) > 3 and want.applied > 10_000
    for piece in (1 << 20, 7):  # (7 bytes: pieces end inside characters)
        got, counts = _stream(fx, BIG_UNICODE, piece, 64 << 10)
        assert got == want.out, piece
        assert counts == (want.applied, want.skipped)


def test_stream_api_edge_cases(fx):
    assert _stream(fx, b"", 7, 0) == (b"", (0, 0))
    assert _stream(fx, b"", 7, 0, eof_alone=True) == (b"", (0, 0))
    plain = b"the quick brown fox " * 5000
    assert _stream(fx, plain, 4099, 64 << 10) == (plain, (0, 0))
    small = (UNIT * 3).encode()
    want = fx.emulate(small, TABLE, overlap=OVERLAP)
    assert _stream(fx, small, 1 << 20, 0, eof_alone=True) == (want.out, (want.applied, want.skipped))
    # the input ends inside a character: its bytes are read, and never written (stream.rs:117-131)
    cut = (UNIT + "école ").encode() + "é".encode()[:1]
    want = fx.emulate(cut, TABLE, overlap=OVERLAP)
    assert want.out == fx.emulate(cut[:-1], TABLE, overlap=OVERLAP).out and want.out.endswith("école ".encode())
    assert _stream(fx, cut, 5, 0) == (want.out, (want.applied, want.skipped))
    # a table of another engine
    other = fixture_builder().device(0).build(["needle"])
    with pytest.raises(DeviceError) as ei:
        _ReplaceStream(fx.eng, ReplacementTable(other, ["X"]), THRESHOLD)
    assert ei.value.code == _native.FAC_E_INVALID


# ---- 6. Python: the table forms take the device stream and equal the host path

@pytest.mark.parametrize("data", [BIG, BIG_UNICODE], ids=["ascii", "unicode"])
def test_python_paths_agree(fx, data):
    def run(f):
        out = io.BytesIO()
        n = f(io.BytesIO(data), out)
        assert n == len(out.getvalue())
        return out.getvalue()

    host = run(lambda r, w: fx.eng.replace_stream(r, w, THRESHOLD, lambda m: TABLE[m.pattern_index]))
    assert host == _emulated(fx, data, 256 << 10).out
    assert run(lambda r, w: FuzzyReplacer(fx.eng, TABLE).replace_stream(r, w, THRESHOLD)) == host
    assert run(lambda r, w: fx.eng.replace_stream(r, w, THRESHOLD, TABLE)) == host
    assert run(lambda r, w: fx.eng.replace_stream(r, w, THRESHOLD, fx.table(TABLE))) == host
    assert run(lambda r, w: fx.eng.replace_stream_parallel(r, w, 4, THRESHOLD, TABLE)) == host
