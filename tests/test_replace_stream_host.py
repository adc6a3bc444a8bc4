"""The crate's streaming replace (stream.rs:465-517 + ReplaceCursor::emit_window, :645-705) replayed
in Python over the CPU oracle, and pinned against the reference's own cases (tests.rs:1153-1273).

`emulate_replace_stream` is the expected-bytes source of tests/test_gpu_replace_stream.py: the window
cut is stream_emulation's (WindowReader, stream.rs:77-159), or an explicit window list; each window is
searched sorted().non_overlapping(), keeps the matches that start before its commit point, sorted by
(start, end), and is emitted through the cursor with callback(m) = the table's entry for
m.pattern_index (a str, None = keep, Wrap = prefix + m.text + suffix)."""
from typing import List, NamedTuple, Optional, Tuple

import pytest
import regex

from fuzzy_aho_corasick import FuzzyAhoCorasickBuilder as B, FuzzyLimits as L, SearchOptions as O
from fuzzy_aho_corasick.engine import Wrap, _rendered_entry
from oracle_harness import OracleEngine
from stream_emulation import _valid_prefix


class Emulated(NamedTuple):
    out: bytes
    applied: int
    skipped: int
    chain: int      # windows entered with the cursor already past their commit point
    ties: int       # windows whose kept records share a start
    emitted: int    # ReplaceCursor::emitted after the last window
    windows: List[Tuple[int, int, int]]  # (first byte, end byte, commit bytes) of every window
    total: int      # bytes read


def reader_windows(data: bytes, overlap: int, window: int, read: int = 64 * 1024) -> List[Tuple[int, int, int]]:
    """WindowReader's cuts (stream.rs:102-158; stream_emulation.stream_rows' loop) as (first byte, end
    byte, commit bytes): reads of `read` bytes until the buffer holds `window`, the valid UTF-8 prefix,
    the commit at the overlap-th grapheme from the end, growth where there are too few graphemes."""
    wins, buf, base, pos, done = [], b"", 0, 0, False
    while not done:
        while len(buf) < window and pos < len(data):
            buf += data[pos:pos + read]
            pos += read
        eof = len(buf) < window
        valid = _valid_prefix(buf)
        if eof:
            commit, done = valid, True
        else:
            starts, off = [], 0
            for g in regex.findall(r"\X", buf[:valid].decode("utf-8")):
                starts.append(off)
                off += len(g.encode("utf-8"))
            if len(starts) < overlap or starts[len(starts) - overlap] == 0:
                window += max(window, 64 * 1024)
                continue
            commit = starts[len(starts) - overlap]
        wins.append((base, base + valid, commit))
        if not done:
            buf = buf[commit:]
            base += commit
    return wins


def strided_windows(n: int, size: int, step: int) -> List[Tuple[int, int, int]]:
    """Windows of `size` bytes cut `step` apart, each committing `step` bytes, the last one (the first
    to reach the end of the input) all of its text."""
    wins, c = [], 0
    while c + size < n:
        wins.append((c, c + size, step))
        c += step
    wins.append((c, n, n - c))
    return wins


def emulate_replace_stream(engine, data: bytes, table, threshold: float, overlap: Optional[int] = None,
                           window: int = 256 * 1024, read: int = 64 * 1024, windows=None, emitted: int = 0) -> Emulated:
    """replace_stream (stream.rs:465-492) of `data` over `engine.search`, with an explicit list of
    windows (first byte, end byte, commit bytes) or the reader's cuts for (window, read). `emitted`:
    the cursor on entry (a list that continues an earlier one)."""
    if windows is None:
        windows = reader_windows(data, overlap, window, read)
    opts = O().threshold(threshold).sorted().non_overlapping()
    out = bytearray()
    applied = skipped = chain = ties = 0
    for (base, end, commit) in windows:
        text = data[base:end]
        ms = [m for m in engine.search(text.decode("utf-8"), opts) if m.start < commit]
        ms.sort(key=lambda m: (m.start, m.end))  # stream.rs:515
        ties += int(len({m.start for m in ms}) != len(ms))
        chain += int(emitted > base + commit)
        for m in ms:  # emit_window, stream.rs:669-692
            if base + m.start < emitted:
                skipped += 1
                continue
            out += text[emitted - base:m.start]
            r = _rendered_entry(table[m.pattern_index], m)
            out += text[m.start:m.end] if r is None else r.encode("utf-8")
            emitted = base + m.end
            applied += 1
        if emitted < base + commit:  # :696-702
            out += text[emitted - base:commit]
            emitted = base + commit
    return Emulated(bytes(out), applied, skipped, chain, ties, emitted, list(windows), len(data))


# ---- the fixture of tests/test_gpu_replace_stream.py

PATTERNS = ["abcdefgh", "efgh", "needle"]
TABLE = ["<A>", "", None]
THRESHOLD = 0.8
OVERLAP = 10
UNIT = "abcdefgh " * 3 + "xx needle abcdefghefgh nedle "


def fixture_builder():
    return B().fuzzy(L().edits(1)).case_insensitive(True)


@pytest.fixture(scope="module")
def needle():
    return OracleEngine(fixture_builder(), ["needle"])


def _run(engine, text, table, **kw):
    r = emulate_replace_stream(engine, text.encode(), table, 0.8, overlap=7, **kw)
    assert r.emitted == len(text.encode())
    return r.out.decode()


def test_small_cases(needle):  # tests.rs:1153-1183, 1240-1259
    x = ["X"]
    assert _run(needle, "a needle b", x) == "a X b"
    assert _run(needle, "needle b", x) == "X b"
    assert _run(needle, "a needle", x) == "a X"
    assert _run(needle, "needle needle", x) == "X X"
    assert _run(needle, "a neeedle b", x) == "a X b"  # one insertion
    assert _run(needle, "nothing here", x) == "nothing here"
    assert _run(needle, "", x) == ""
    assert _run(needle, "a needle b", [None]) == "a needle b"
    assert _run(needle, "a needle b", [Wrap("**", "**")]) == "a **needle** b"


@pytest.mark.parametrize("window", [256 * 1024, 4096, 64 << 10])
def test_stream_equals_whole_input_replace(needle, window):  # tests.rs:1186-1237
    filler = "the quick brown fox " * 50
    text = ""
    while len(text) < 600_000:
        text += filler + "needle "
    truth = needle.replace(text, O().threshold(0.8), lambda m: f"<{m.pattern_index}>")
    r = emulate_replace_stream(needle, text.encode(), ["<0>"], 0.8, overlap=7, window=window)
    assert r.out.decode() == truth and "<0>" in truth
    assert r.skipped == 0 and r.ties == 0 and len(r.windows) > 2


def test_fuzzy_replacer_case():  # tests.rs:1262-1273
    eng = OracleEngine(B().case_insensitive(True).fuzzy(L().edits(1)), ["hello", "world"])
    assert _run(eng, "hell0 w0rld!", ["hi", "earth"]) == "hi earth!"


def test_explicit_windows_and_split_lists():
    """The fixture's figures: windows far shorter than a match's reach, so that the cursor passes
    whole windows; and a window list split in two with the cursor carried gives the same output."""
    eng = OracleEngine(fixture_builder(), PATTERNS)
    data = (UNIT * 6).encode()
    wins = strided_windows(len(data), 30, 2)
    r = emulate_replace_stream(eng, data, TABLE, THRESHOLD, windows=wins)
    assert (len(wins), r.applied, r.skipped, r.chain, r.ties, len(r.out)) == (154, 42, 23, 72, 0, 192)
    for (step, size) in ((3, 40), (5, 25)):
        q = emulate_replace_stream(eng, data, TABLE, THRESHOLD, windows=strided_windows(len(data), size, step))
        assert q.skipped > 0 and q.chain > 0 and q.ties == 0
    for cut in (1, 50, 153):
        a = emulate_replace_stream(eng, data, TABLE, THRESHOLD, windows=wins[:cut])
        b = emulate_replace_stream(eng, data, TABLE, THRESHOLD, windows=wins[cut:], emitted=a.emitted)
        assert a.out + b.out == r.out and b.emitted == r.emitted == len(data)
        assert (a.applied + b.applied, a.skipped + b.skipped) == (r.applied, r.skipped)


def test_reader_windows_of_the_fixture():
    eng = OracleEngine(fixture_builder(), PATTERNS)
    data = (UNIT * 40).encode()
    for (window, read, n_windows, skipped) in ((24, 8, 140, 40), (32, 16, None, 20), (33, 7, None, 0)):
        r = emulate_replace_stream(eng, data, TABLE, THRESHOLD, overlap=OVERLAP, window=window, read=read)
        assert r.skipped == skipped and r.ties == 0 and r.emitted == len(data)
        assert n_windows is None or len(r.windows) == n_windows
    big = ((UNIT + "the quick brown fox ") * 5000).encode()
    assert len(big) == 380_000
    for (window, n_windows) in ((64 << 10, 6), (100_003, 4)):
        r = emulate_replace_stream(eng, big, TABLE, THRESHOLD, overlap=OVERLAP, window=window)
        assert (len(r.windows), r.skipped, r.ties) == (n_windows, 2, 0)


def test_truncated_tail_is_dropped(needle):
    data = "a needle é".encode()[:-1]  # the input ends inside a character
    r = emulate_replace_stream(needle, data, ["X"], 0.8, overlap=7)
    assert r.out == b"a X " and r.total == len(data) and r.emitted == len(data) - 1
