"""Test helper: whole-token matches of a stream (fac.h fac_stream_open_opts) replayed
over the CPU oracle. The reader is stream_emulation's (test_replace_stream_host.reader_windows is its
loop as a window list). For a window with text T at stream offset `base`:

1. rows = the oracle's raw_rows(T, thr, prefilter);
2. keep those with ref_ok(data[:base + len(T)], base + start, base + end, sides) -- the `regex`-based
   rule of test_boundaries_host.py; with the whole earlier stream as prefix it is the stream rule: the
   start side walks into the text before the window, the end side stops at the window's end;
3. the oracle's apply_rows(Default, NonOverlapping);
4. then start < commit.

Nothing here calls the product."""
import struct

from fuzzy_aho_corasick import FuzzyMatch, FuzzyMatches, Order, Overlap
from test_boundaries_host import ref_ok
from test_replace_stream_host import emulate_replace_stream, reader_windows


def sim_bits(x) -> int:
    return struct.unpack("<I", struct.pack("<f", x))[0]


class StreamEmulation:
    """The windows of `data` and, per window, the raw rows, the rows the rule keeps and the applied
    rows (window-relative), each computed once."""

    def __init__(self, orc, data: bytes, thr: float, overlap: int, window: int, read: int, prefilter: bool, sides: int):
        self.orc, self.data, self.thr, self.prefilter, self.sides = orc, data, thr, prefilter, int(sides)
        self.overlap = overlap
        self.wins = reader_windows(data, overlap, window, read)
        self.raw, self.kept, self.applied = [], [], []
        for base, end, _ in self.wins:
            raw = orc.raw_rows(data[base:end].decode("utf-8"), thr, prefilter)
            kept = [r for r in raw if ref_ok(data[:end], base + r[0], base + r[1], self.sides)]
            self.raw.append(raw)
            self.kept.append(kept)
            self.applied.append(orc.apply_rows(kept, Order.Default, Overlap.NonOverlapping))

    def rows(self):
        """The stream's rows: (start, end, pattern, similarity bits, text) at stream offsets."""
        out = []
        for (base, _, commit), rows in zip(self.wins, self.applied):
            out += [(base + r[0], base + r[1], r[2], sim_bits(r[3]), self.data[base + r[0]:base + r[1]].decode("utf-8"))
                    for r in rows if r[0] < commit]
        return sorted(out)

    def context_drops(self, w: int):
        """Raw rows of window w at window byte 0 that the rule drops with the stream's text before the
        window, and would keep with the window's text as its document."""
        base, end, _ = self.wins[w]
        text = self.data[base:end]
        return [r for r in self.raw[w] if r[0] == 0 and r not in self.kept[w] and ref_ok(text, r[0], r[1], self.sides)]

    def ends_at_window_end(self, w: int):
        base, end, _ = self.wins[w]
        return [r for r in self.raw[w] if r[1] == end - base]

    def searcher(self, wins=None):
        return _WindowSearch(self, wins if wins is not None else self.wins)

    def replace(self, table, wins=None, emitted=0):
        """emulate_replace_stream over a search that does steps 1 to 3 per window."""
        wins = self.wins if wins is None else wins
        return emulate_replace_stream(self.searcher(wins), self.data, table, self.thr, windows=wins, emitted=emitted)


class _WindowSearch:
    """`search` for emulate_replace_stream: called once per window, in window order."""

    def __init__(self, emu: StreamEmulation, wins):
        self.emu, self.wins, self.k = emu, list(wins), 0

    def search(self, text: str, opts):
        emu = self.emu
        base, end, _ = self.wins[self.k]
        self.k += 1
        data = emu.data[base:end]
        assert text.encode("utf-8") == data
        assert (opts.order_, opts.overlap_) == (Order.Default, Overlap.NonOverlapping)
        rows = emu.applied[emu.wins.index((base, end, _))]
        inner = [FuzzyMatch(ins, dele, sub, swp, ed, p, emu.orc.patterns_[p], s, e, sim, data[s:e].decode("utf-8"))
                 for (s, e, p, sim, ins, dele, sub, swp, ed) in rows]
        return FuzzyMatches(text, inner, data)
