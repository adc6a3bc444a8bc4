"""FuzzyAhoCorasickBuilder / FuzzyAhoCorasick: the crate's public surface (builder.rs, query.rs,
prefilter.rs, replacer.rs) over the C ABI of include/fac.h. Every search goes to the GPU."""
from __future__ import annotations

import ctypes
import os
import sys
import time
from typing import Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple, Union

from . import _native

_TIMING = bool(os.environ.get("FAC_TIMING"))  # diagnostics: host-side phase times
from .matches import FuzzyMatch, FuzzyMatches, Segment, TermCount, UnmatchedSegment
from .structs import (Anchor, Boundary, DeviceError, FuzzyLimits, FuzzyPenalties, HaystackTooLarge, Order, Overlap,
                      Pattern, SearchError, SearchOptions, Similarity, UnsupportedConfiguration, f32)


def _default_device() -> int:
    for var in ("FAC_DEVICE", "LOCAL_RANK"):
        if var in os.environ:
            return int(os.environ[var])
    return 0


def _raise(rc: int, err_graphemes: int = 0):
    if rc == _native.FAC_E_HAYSTACK_TOO_LARGE:
        raise HaystackTooLarge(err_graphemes)
    if rc == _native.FAC_E_UNSUPPORTED:
        raise UnsupportedConfiguration(_native.last_error())
    raise DeviceError(rc, _native.last_error())


class FuzzyAhoCorasickBuilder:
    """builder.rs:22-168. Chainable; `build` uploads the automaton to the GPU."""

    def __init__(self):
        self._similarity: Optional[Similarity] = None
        self._limits: Optional[FuzzyLimits] = None
        self._penalties = FuzzyPenalties()
        self._case_insensitive = False
        self._beam_width: Optional[int] = None
        self._auto_beam: Optional[Tuple[int, int]] = None
        self._mappings: List[Tuple[str, str, float]] = []
        self._min_symbol_similarity = 0.0
        self._device = _default_device()

    @classmethod
    def new(cls) -> "FuzzyAhoCorasickBuilder":
        return cls()

    def similarity(self, sim: Similarity) -> "FuzzyAhoCorasickBuilder":
        self._similarity = sim
        return self

    def fuzzy(self, limits: FuzzyLimits) -> "FuzzyAhoCorasickBuilder":
        self._limits = limits.finalize()
        return self

    def penalties(self, p: FuzzyPenalties) -> "FuzzyAhoCorasickBuilder":
        self._penalties = p
        return self

    def case_insensitive(self, value: bool) -> "FuzzyAhoCorasickBuilder":
        self._case_insensitive = bool(value)
        return self

    def beam_width(self, width: int) -> "FuzzyAhoCorasickBuilder":
        self._beam_width = int(width)
        return self

    def auto_beam(self, budget: int, width: int) -> "FuzzyAhoCorasickBuilder":
        self._auto_beam = (int(budget), int(width))
        return self

    def mapping(self, a: str, b: str) -> "FuzzyAhoCorasickBuilder":
        return self.mapping_scored(a, b, 1.0)

    def mapping_scored(self, a: str, b: str, score: float) -> "FuzzyAhoCorasickBuilder":
        self._mappings.append((a, b, f32(score)))
        return self

    def min_symbol_similarity(self, m: float) -> "FuzzyAhoCorasickBuilder":
        self._min_symbol_similarity = f32(m)
        return self

    def device(self, ordinal: int) -> "FuzzyAhoCorasickBuilder":
        """Extension: HIP device that holds this engine's tables."""
        self._device = int(ordinal)
        return self

    def build(self, inputs: Iterable) -> "FuzzyAhoCorasick":
        patterns = [Pattern.from_(x) for x in inputs]
        return FuzzyAhoCorasick(self, patterns)

    def build_replacer(self, pairs: Iterable) -> "FuzzyReplacer":
        pats, repl = [], []
        for p, r in pairs:
            pats.append(Pattern.from_(p))
            repl.append(r if isinstance(r, Wrap) else str(r))
        return FuzzyReplacer(self.build(pats), repl)


class FuzzyAhoCorasick:
    """structs.rs:528-567 + search/query entry points (query.rs:30-202)."""

    def __init__(self, builder: FuzzyAhoCorasickBuilder, patterns: List[Pattern]):
        self.patterns_ = patterns
        self.builder = builder
        self._keep = []  # keep ctypes buffers alive during the call
        cfg = _native.fac_config()
        cfg.case_insensitive = int(builder._case_insensitive)
        cfg.has_limits = int(builder._limits is not None)
        cfg.limits = (builder._limits or FuzzyLimits()).to_c()
        pen = builder._penalties
        cfg.penalty_insertion = pen.insertion
        cfg.penalty_deletion = pen.deletion
        cfg.penalty_substitution = pen.substitution
        cfg.penalty_swap = pen.swap
        cfg.beam_width = builder._beam_width or 0
        if builder._beam_width == 0:
            raise ValueError("beam_width must be >= 1")
        cfg.has_auto_beam = int(builder._auto_beam is not None)
        if builder._auto_beam:
            cfg.auto_beam_budget, cfg.auto_beam_width = builder._auto_beam
        cfg.min_symbol_similarity = builder._min_symbol_similarity
        if builder._similarity is not None:
            tab = (ctypes.c_float * (128 * 128))(*builder._similarity.ascii_table())
            extra = builder._similarity.extra_pairs()
            ab = (ctypes.c_uint32 * (2 * max(1, len(extra))))()
            vals = (ctypes.c_float * max(1, len(extra)))()
            for i, (a, b, s) in enumerate(extra):
                ab[2 * i], ab[2 * i + 1], vals[i] = a, b, s
            cfg.similarity_ascii = tab
            cfg.n_similarity_pairs = len(extra)
            cfg.similarity_pairs = ab
            cfg.similarity_pair_values = vals
            self._keep += [tab, ab, vals]
        cfg.n_mappings = len(builder._mappings)
        if builder._mappings:  # builder.rs:116-132
            maps = (_native.fac_mapping * len(builder._mappings))()
            for i, (a, b, score) in enumerate(builder._mappings):
                ea, eb = a.encode("utf-8"), b.encode("utf-8")
                self._keep += [ea, eb]
                maps[i].a, maps[i].a_len, maps[i].b, maps[i].b_len, maps[i].score = ea, len(ea), eb, len(eb), score
            cfg.mappings = maps
            self._keep.append(maps)
        cfg.device = builder._device
        arr = (_native.fac_pattern * max(1, len(patterns)))()
        enc = []
        for i, p in enumerate(patterns):
            b = p.pattern.encode("utf-8")
            enc.append(b)
            arr[i].utf8 = b
            arr[i].len = len(b)
            arr[i].weight = p.weight
            arr[i].has_limits = int(p.limits is not None)
            arr[i].limits = (p.limits or FuzzyLimits()).to_c()
        handle = ctypes.c_void_p()
        rc = _native.lib.fac_build(arr, len(patterns), ctypes.byref(cfg), ctypes.byref(handle))
        if rc:
            _raise(rc)
        self._h = handle
        self.device = builder._device

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _native.lib is not None:  # the module may already be torn down at exit
            _native.lib.fac_engine_free(h)
            self._h = None

    def drop_prefix_cache(self) -> None:
        """fac_engine_drop_prefix_cache: frees the prefix-cache snapshots the engine keeps from search
        to search (up to FAC_RC_POOL_MB of device memory); the next search builds every key again."""
        _native.lib.fac_engine_drop_prefix_cache(self._h)

    # -- introspection
    def patterns(self) -> List[Pattern]:
        return self.patterns_

    def num_nodes(self) -> int:
        return int(_native.lib.fac_engine_num_nodes(self._h))

    def max_edits_fast(self) -> int:
        return int(_native.lib.fac_engine_max_edits_fast(self._h))

    def grapheme_id(self, grapheme: str) -> int:
        """fac_engine_grapheme_id: the id of one grapheme in the dictionary of an engine with
        multi-character mappings, folded and looked up on the host; 0 = not in it (or no mappings)."""
        raw = grapheme.encode("utf-8")
        return int(_native.lib.fac_engine_grapheme_id(self._h, raw, len(raw)))

    def max_match_graphemes(self) -> int:
        """stream.rs:213-253"""
        return int(_native.lib.fac_max_match_graphemes(self._h))

    # -- raw search (search.rs:187-395)
    def _to_matches(self, haystack: str, data: bytes, rows) -> FuzzyMatches:
        inner = []
        for (s, e, p, sim, ins, dele, sub, swp, ed) in rows:
            inner.append(FuzzyMatch(ins, dele, sub, swp, ed, p, self.patterns_[p], s, e, sim,
                                    data[s:e].decode("utf-8")))
        return FuzzyMatches(haystack, inner, data)

    def search_raw(self, haystack: str, threshold: float, prefilter: bool = False) -> FuzzyMatches:
        data = haystack.encode("utf-8")
        out = ctypes.POINTER(_native.fac_match)()
        n = ctypes.c_uint64()
        eg = ctypes.c_uint64()
        fn = _native.lib.fac_search_prefiltered if prefilter else _native.lib.fac_search_raw
        rc = fn(self._h, data, len(data), f32(threshold), ctypes.byref(out), ctypes.byref(n), ctypes.byref(eg))
        if rc:
            _raise(rc, eg.value)
        return self._to_matches(haystack, data, _native.take_matches(out, n.value))

    def _unique_ids(self):
        """Uniqueness key per pattern for NonOverlappingUnique (matches.rs:118-122): custom ids and
        automatic (index) ids never compare equal."""
        if getattr(self, "_uid", None) is None:
            keys = [(1 << 63) | p.custom_unique_id_ if p.custom_unique_id_ is not None else i
                    for i, p in enumerate(self.patterns_)]
            self._uid = (ctypes.c_uint64 * max(1, len(keys)))(*keys)
        return self._uid

    def _search_ranked(self, haystack: str, threshold: float, order: Order, overlap: Overlap,
                       prefilter: bool = False) -> FuzzyMatches:
        """search_raw + FuzzyMatches::apply, the ranking / overlap resolution on the device
        (fac_matches_apply, matches.rs:7-149) before any Python object is built."""
        data = haystack.encode("utf-8")
        out = ctypes.POINTER(_native.fac_match)()
        n = ctypes.c_uint64()
        eg = ctypes.c_uint64()
        fn = _native.lib.fac_search_prefiltered if prefilter else _native.lib.fac_search_raw
        rc = fn(self._h, data, len(data), f32(threshold), ctypes.byref(out), ctypes.byref(n), ctypes.byref(eg))
        if rc:
            _raise(rc, eg.value)
        count = n.value
        if count and (order != Order.Unsorted or overlap != Overlap.Keep):
            kept = ctypes.c_uint64()
            rc = _native.lib.fac_matches_apply(self._h, out, count, order.value, overlap.value, self._unique_ids(),
                                               ctypes.byref(kept))
            if rc:
                _native.lib.fac_matches_free(out)
                _raise(rc)
            count = kept.value
        return self._to_matches(haystack, data, _native.take_matches(out, count))

    # -- stream.rs
    def search_stream(self, reader, threshold: float, on_match, window: int = 0, _prefilter: bool = False,
                      boundaries: Boundary = Boundary.NONE) -> int:
        """stream.rs:299-328: search a byte stream (anything with .read(n)) in overlapping windows,
        calling `on_match(StreamMatch)` with absolute offsets; returns the bytes read. `boundaries`
        (here and in the other stream calls; non-zero): only matches whose named sides are word
        boundaries of the stream's text reach a window's ranking and overlap resolution; the start
        side looks to the left of the window into the text read before it (fac_stream_open_opts)."""
        st = _Stream(self, threshold, window, prefilter=_prefilter, boundaries=boundaries)
        while True:
            chunk = reader.read(READ_CHUNK)
            for m in st.feed(chunk or b"", eof=not chunk):
                on_match(m)
            if not chunk:
                return st.total()

    def stream_matches(self, reader, threshold: float, window: int = 0, _prefilter: bool = False,
                       boundaries: Boundary = Boundary.NONE):
        """stream.rs:330-352: the same, lazily, as an iterator of StreamMatch."""
        st = _Stream(self, threshold, window, prefilter=_prefilter, boundaries=boundaries)
        while True:
            chunk = reader.read(READ_CHUNK)
            yield from st.feed(chunk or b"", eof=not chunk)
            if not chunk:
                return

    def search_stream_parallel(self, reader, threshold: float, threads: int, on_match,
                               boundaries: Boundary = Boundary.NONE) -> int:
        """stream.rs:378-429. The device path already searches two windows at a time (one HIP
        stream each, fac_stream); `threads` is accepted for API parity."""
        return self.search_stream(reader, threshold, on_match, boundaries=boundaries)

    def replace_stream(self, reader, writer, threshold: float, callback, window: int = 0,
                       _prefilter: bool = False, boundaries: Boundary = Boundary.NONE) -> int:
        """stream.rs:462-503 + ReplaceCursor::emit_window (:645-705): streaming find-and-replace.
        Every owned match (per window: sorted().non_overlapping(), start < commit, ordered by
        (start, end)) is replaced by `callback(m)` (a str; None keeps the matched text) unless it
        starts inside text already written; everything else is copied through. Text before the
        stream's commit point is written as soon as it is committed. Returns the bytes written.
        `callback` may be a ReplacementTable or a list with one entry per pattern (str / bytes, None =
        keep, Wrap = a template): the splice then runs on the device (fac_replace_stream_*). A
        callable is called per match on the host."""
        if not callable(callback):
            table = callback if isinstance(callback, ReplacementTable) else ReplacementTable(self, callback)
            st = _ReplaceStream(self, table, threshold, window, prefilter=_prefilter, boundaries=boundaries)
            while True:
                chunk = reader.read(READ_CHUNK)
                out = st.feed(chunk or b"", eof=not chunk)
                if out:
                    writer.write(out)
                if not chunk:
                    return st.written()
        st = _Stream(self, threshold, window, prefilter=_prefilter, boundaries=boundaries)
        pending = bytearray()  # stream bytes [emitted, read) not yet written
        emitted = written = 0

        def out(b: bytes):
            nonlocal written
            if b:
                writer.write(b)
                written += len(b)

        def emit(ms, upto):
            nonlocal emitted, pending
            for m in sorted(ms, key=lambda m: (m.start, m.end)):
                if m.start < emitted:  # overlaps text an earlier window's match already wrote
                    continue
                out(bytes(pending[: m.start - emitted]))
                repl = callback(m)
                out(m.text.encode("utf-8") if repl is None else str(repl).encode("utf-8"))
                del pending[: m.end - emitted]
                emitted = m.end
            if emitted < upto:  # verbatim up to the commit point
                out(bytes(pending[: upto - emitted]))
                del pending[: upto - emitted]
                emitted = upto

        while True:
            chunk = reader.read(READ_CHUNK)
            pending += chunk or b""
            ms = st.feed(chunk or b"", eof=not chunk)
            if not chunk:
                emit(ms, st.total())
                return written
            emit(ms, max(emitted, st.committed()))

    def replace_stream_parallel(self, reader, writer, threads: int, threshold: float, callback,
                                boundaries: Boundary = Boundary.NONE) -> int:
        """stream.rs:533-638: same output as replace_stream (windows are pipelined on the device);
        `callback` as there."""
        return self.replace_stream(reader, writer, threshold, callback, boundaries=boundaries)

    def apply_on_device(self, matches: FuzzyMatches, order: Order, overlap: Overlap) -> FuzzyMatches:
        """FuzzyMatches::apply of an existing match list through fac_matches_apply (same input
        order in, so Unsorted + NonOverlapping walks the same sequence as the host)."""
        n = len(matches.inner)
        arr = (_native.fac_match * max(1, n))()
        for i, m in enumerate(matches.inner):
            arr[i] = _native.fac_match(m.start, m.end, m.pattern_index, m.similarity, m.insertions, m.deletions,
                                       m.substitutions, m.swaps, m.edits)
        kept = ctypes.c_uint64()
        rc = _native.lib.fac_matches_apply(self._h, arr, n, order.value, overlap.value, self._unique_ids(),
                                           ctypes.byref(kept))
        if rc:
            _raise(rc)
        rows = [(a.start, a.end, a.pattern_index, a.similarity, a.insertions, a.deletions, a.substitutions, a.swaps,
                 a.edits) for a in arr[:kept.value]]
        return self._to_matches(matches.haystack, matches.haystack.encode("utf-8"), rows)

    # -- query.rs
    def search(self, haystack: str, opts: SearchOptions = None, boundaries: Boundary = Boundary.NONE,
               anchors: Anchor = Anchor.NONE) -> FuzzyMatches:
        """`boundaries` (non-zero): only matches whose named sides are word boundaries take part in
        ranking and overlap resolution (DESIGN.md 6a "Whole-token matches"); the haystack then runs
        as a one-document batch, where that filter is on the device. `anchors` (non-zero): only
        matches that touch the named ends of the haystack do (DESIGN.md 6a "Anchored matches"), by
        the same route."""
        opts = opts or SearchOptions()
        if int(boundaries) or int(anchors):
            return self.search_batch([haystack], opts, unicode_mappings=True, boundaries=boundaries, anchors=anchors)[0]
        return self._search_ranked(haystack, opts.threshold_, opts.order_, opts.overlap_)

    def _search_bounded(self, haystack: str, threshold: float, order: Order, overlap: Overlap, prefilter: bool,
                        boundaries, anchors=Anchor.NONE) -> FuzzyMatches:
        """One haystack on the host route: search_raw, FuzzyMatches.retain_boundaries and
        retain_anchors, then apply (the per-document form the batch conveniences fall back to)."""
        if not int(boundaries) and not int(anchors):
            return self._search_ranked(haystack, threshold, order, overlap, prefilter=prefilter)
        ms = self.search_raw(haystack, threshold, prefilter=prefilter).retain_boundaries(boundaries).retain_anchors(anchors)
        if order == Order.Unsorted and overlap == Overlap.Keep:
            return ms
        return self.apply_on_device(ms, order, overlap)

    def _segmented(self, haystack: str, opts: SearchOptions) -> FuzzyMatches:
        order = Order.Default if opts.order_ == Order.Unsorted else opts.order_
        overlap = Overlap.NonOverlapping if opts.overlap_ == Overlap.Keep else opts.overlap_
        return self._search_ranked(haystack, opts.threshold_, order, overlap)

    def replace(self, text: str, opts: SearchOptions, callback) -> str:
        return self._segmented(text, opts).replace(callback)

    def strip_prefix(self, haystack: str, opts: SearchOptions) -> str:
        return self._segmented(haystack, opts).strip_prefix()

    def strip_suffix(self, haystack: str, opts: SearchOptions) -> str:
        return self._segmented(haystack, opts).strip_suffix()

    def split(self, haystack: str, opts: SearchOptions):
        return self._segmented(haystack, opts).split()

    def segment_iter(self, haystack: str, opts: SearchOptions):
        return self._segmented(haystack, opts).segment_iter()

    def segment_text(self, haystack: str, opts: SearchOptions) -> str:
        return self._segmented(haystack, opts).segment_text()

    # -- prefilter.rs:113-155
    def with_prefilter(self) -> "Prefiltered":
        return Prefiltered(self)

    # -- device-resident haystacks (bench / sharding)
    def stage(self, haystack: bytes) -> "StagedHaystack":
        return StagedHaystack(self, haystack)

    # -- many independent haystacks in one device pass (fac_search_batch)
    def search_batch(self, haystacks: Sequence[str], opts: SearchOptions = None,
                     unicode_mappings: bool = False, boundaries: Boundary = Boundary.NONE,
                     anchors: Anchor = Anchor.NONE) -> List[FuzzyMatches]:
        """`[self.search(h, opts) for h in haystacks]` as one call: every haystack is staged, searched
        and ranked as a text of its own (the crate has no such entry point; its answer to many
        documents is one engine shared by threads). Errors name the first offending document
        (`.doc` of the exception). `unicode_mappings` (here and in the other batch calls): an engine
        with multi-character mappings takes non-ASCII haystacks too (StagedBatch.allow_unicode_mappings;
        default off: such a batch raises UnsupportedConfiguration). `boundaries` (here and in the
        other batch calls): only matches whose named sides are word boundaries of their own haystack
        reach ranking and overlap resolution (StagedBatch.require_boundaries)."""
        opts = opts or SearchOptions()
        haystacks = list(haystacks)
        enc = [h.encode("utf-8") for h in haystacks]
        data, offsets = batch_offsets(enc)
        recs, doc_off = StagedBatch(self, data, offsets, unicode_mappings=unicode_mappings,
                                    boundaries=boundaries, anchors=anchors).search_records(opts)
        out = []
        for d, (hay, raw) in enumerate(zip(haystacks, enc)):
            rows = [(int(r["start"]), int(r["end"]), int(r["pattern_index"]), float(r["similarity"]),
                     int(r["insertions"]), int(r["deletions"]), int(r["substitutions"]), int(r["swaps"]),
                     int(r["edits"])) for r in recs[int(doc_off[d]):int(doc_off[d + 1])]]
            out.append(self._to_matches(hay, raw, rows))
        return out

    def lookup_batch(self, texts: Sequence[str], opts: SearchOptions = None, k: int = 1,
                     unicode_mappings: bool = False, boundaries: Boundary = Boundary.NONE) -> List[List[FuzzyMatch]]:
        """Which entries IS each text? Per text the up to `k` matches that cover the whole text, best
        first in the order `opts` names (Unsorted is taken as Default), as one call
        (fac_lookup_batch, StagedBatch.lookup_records): the fuzzy join of a column against the
        dictionary. An empty list: no entry matches the text as a whole."""
        opts = opts or SearchOptions()
        texts = list(texts)
        enc = [t.encode("utf-8") for t in texts]
        data, offsets = batch_offsets(enc)
        recs, found = StagedBatch(self, data, offsets, unicode_mappings=unicode_mappings,
                                  boundaries=boundaries).lookup_records(opts, k)
        out = []
        for d, (text, raw) in enumerate(zip(texts, enc)):
            rows = [(int(r["start"]), int(r["end"]), int(r["pattern_index"]), float(r["similarity"]),
                     int(r["insertions"]), int(r["deletions"]), int(r["substitutions"]), int(r["swaps"]),
                     int(r["edits"])) for r in recs[d, :int(found[d])]]
            out.append(list(self._to_matches(text, raw, rows)))
        return out

    def count_batch(self, texts: Sequence[str], opts: SearchOptions = None, keys=None, n_keys=None,
                    unicode_mappings: bool = False, boundaries: Boundary = Boundary.NONE,
                    anchors: Anchor = Anchor.NONE) -> List[Dict[int, TermCount]]:
        """Which entries does each text mention, and how often? `[self.search(t, opts).term_counts(keys,
        n_keys) for t in texts]` as one call (fac_count_batch, StagedBatch.count_records): per text
        {key: TermCount(count, best_similarity, best_pattern)} in ascending key order, grouped on the
        device. `keys`: one key per pattern (None: key = pattern index)."""
        enc = [t.encode("utf-8") for t in texts]
        data, offsets = batch_offsets(enc)
        terms, doc_off, _ = StagedBatch(self, data, offsets, unicode_mappings=unicode_mappings, boundaries=boundaries,
                                        anchors=anchors).count_records(opts, keys, n_keys)
        return _term_dicts(terms, doc_off)

    def replace_batch(self, texts: Sequence[str], opts: SearchOptions, replacements,
                      unicode_mappings: bool = False, boundaries: Boundary = Boundary.NONE,
                      anchors: Anchor = Anchor.NONE) -> List[str]:
        """`[self.replace(t, opts, lambda m: replacements[m.pattern_index]) for t in texts]` as one
        call (fac_replace_batch): searched, ranked and spliced on the device. `replacements` has one
        entry per pattern, `None` = keep the matched text (the callback's None, matches.rs:180-183).
        A per-match callback cannot run on the device; a per-pattern table is what FuzzyReplacer
        uses (replacer.rs:24). Kept records of equal start are applied in the order search_batch
        returns them (the crate leaves that order open, matches.rs:111)."""
        enc = [t.encode("utf-8") for t in texts]
        data, offsets = batch_offsets(enc)
        table = replacements if isinstance(replacements, ReplacementTable) else ReplacementTable(self, replacements)
        out, off = StagedBatch(self, data, offsets, unicode_mappings=unicode_mappings,
                               boundaries=boundaries, anchors=anchors).replace_bytes(table, opts)
        return [out[int(off[d]):int(off[d + 1])].decode("utf-8") for d in range(len(enc))]

    def extract_batch(self, texts: Sequence[str], opts: SearchOptions, replacements=None,
                      unicode_mappings: bool = False, boundaries: Boundary = Boundary.NONE,
                      anchors: Anchor = Anchor.NONE) -> List[List[str]]:
        """Per text, one string per match of `self.search(t, opts)`, in its order, as one call
        (fac_extract_batch): the matched text, or with `replacements` (one entry per pattern, or a
        ReplacementTable) what replace would put in its place -- the entry, `Wrap` rendered around
        the matched text, the matched text for None."""
        table = replacements
        if replacements is not None and not isinstance(replacements, ReplacementTable):
            table = ReplacementTable(self, replacements)
        return _extract_batch(self, [t.encode("utf-8") for t in texts], opts or SearchOptions(), table, False,
                              unicode_mappings, boundaries, anchors)

    def matched_strings_batch(self, texts: Sequence[str], opts: SearchOptions = None,
                              unicode_mappings: bool = False, boundaries: Boundary = Boundary.NONE,
                              anchors: Anchor = Anchor.NONE) -> List[List[str]]:
        """`[self.search(t, opts).matched_strings() for t in texts]` as one call (matches.rs:513-515)."""
        return self.extract_batch(texts, opts, unicode_mappings=unicode_mappings, boundaries=boundaries, anchors=anchors)

    # -- the other segmentation helpers of a whole batch (fac_render_batch, fac_segment_batch): each is
    # one device call; whitespace is Rust's char::is_whitespace (DESIGN.md 6a "Batched segmentation")
    def strip_prefix_batch(self, texts: Sequence[str], opts: SearchOptions, unicode_mappings: bool = False,
                           boundaries: Boundary = Boundary.NONE, anchors: Anchor = Anchor.NONE) -> List[str]:
        """`[self.strip_prefix(t, opts) for t in texts]` as one call."""
        return _render_batch(self, texts, _native.FAC_RENDER_STRIP_PREFIX, opts, False, unicode_mappings, boundaries, anchors)

    def strip_suffix_batch(self, texts: Sequence[str], opts: SearchOptions, unicode_mappings: bool = False,
                           boundaries: Boundary = Boundary.NONE, anchors: Anchor = Anchor.NONE) -> List[str]:
        """`[self.strip_suffix(t, opts) for t in texts]` as one call."""
        return _render_batch(self, texts, _native.FAC_RENDER_STRIP_SUFFIX, opts, False, unicode_mappings, boundaries, anchors)

    def segment_text_batch(self, texts: Sequence[str], opts: SearchOptions, unicode_mappings: bool = False,
                           boundaries: Boundary = Boundary.NONE, anchors: Anchor = Anchor.NONE) -> List[str]:
        """`[self.segment_text(t, opts) for t in texts]` as one call."""
        return _render_batch(self, texts, _native.FAC_RENDER_SEGMENT_TEXT, opts, False, unicode_mappings, boundaries, anchors)

    def segment_batch(self, texts: Sequence[str], opts: SearchOptions, unicode_mappings: bool = False,
                      boundaries: Boundary = Boundary.NONE, anchors: Anchor = Anchor.NONE) -> List[List[Segment]]:
        """`[list(self.segment_iter(t, opts)) for t in texts]` as one call."""
        return _segment_batch(self, texts, opts, False, unicode_mappings, boundaries, anchors)

    def split_batch(self, texts: Sequence[str], opts: SearchOptions, unicode_mappings: bool = False,
                    boundaries: Boundary = Boundary.NONE, anchors: Anchor = Anchor.NONE) -> List[List[str]]:
        """`[list(self.split(t, opts)) for t in texts]` as one call."""
        return [[s.unmatched().text for s in segs if s.unmatched() is not None]
                for segs in _segment_batch(self, texts, opts, False, unicode_mappings, boundaries, anchors)]


class Prefiltered:
    """prefilter.rs:57-156"""

    def __init__(self, engine: FuzzyAhoCorasick):
        self.engine = engine

    def is_active(self) -> bool:
        return bool(_native.lib.fac_prefilter_active(self.engine._h))

    def search(self, haystack: str, opts: SearchOptions = None) -> FuzzyMatches:
        opts = opts or SearchOptions()
        return self.engine._search_ranked(haystack, opts.threshold_, opts.order_, opts.overlap_, prefilter=True)

    # -- stream.rs over Prefiltered::search: every window's text goes through the bitap pre-filter on
    # the device (fac_stream_open_ex / fac_replace_stream_open_ex); signatures as the engine's
    def search_stream(self, reader, threshold: float, on_match, window: int = 0,
                      boundaries: Boundary = Boundary.NONE) -> int:
        return self.engine.search_stream(reader, threshold, on_match, window, _prefilter=True, boundaries=boundaries)

    def stream_matches(self, reader, threshold: float, window: int = 0, boundaries: Boundary = Boundary.NONE):
        return self.engine.stream_matches(reader, threshold, window, _prefilter=True, boundaries=boundaries)

    def search_stream_parallel(self, reader, threshold: float, threads: int, on_match,
                               boundaries: Boundary = Boundary.NONE) -> int:
        """As the engine's: two windows are in flight on the device; `threads` is accepted for API parity."""
        return self.search_stream(reader, threshold, on_match, boundaries=boundaries)

    def replace_stream(self, reader, writer, threshold: float, callback, window: int = 0,
                       boundaries: Boundary = Boundary.NONE) -> int:
        """A table or list `callback` is spliced on the device; a callable runs over the pre-filtered
        search stream on the host."""
        return self.engine.replace_stream(reader, writer, threshold, callback, window, _prefilter=True,
                                          boundaries=boundaries)

    def replace_stream_parallel(self, reader, writer, threads: int, threshold: float, callback,
                                boundaries: Boundary = Boundary.NONE) -> int:
        return self.replace_stream(reader, writer, threshold, callback, boundaries=boundaries)

    def _batch_parts(self, enc):
        """Indices of the documents one pre-filtered batch takes: all of them where the filter is
        active or the engine has mappings (the batch is opted in, allow_unicode_prefilter and
        allow_unicode_mappings; an engine with mappings has no filter and takes the plain batch call),
        else the ASCII ones (the others go through `search` one by one)."""
        if self.is_active() or self.engine.builder._mappings:
            return list(range(len(enc)))
        return [d for d, raw in enumerate(enc) if raw.isascii()]

    def search_batch(self, haystacks: Sequence[str], opts: SearchOptions = None,
                     boundaries: Boundary = Boundary.NONE, anchors: Anchor = Anchor.NONE) -> List[FuzzyMatches]:
        """`[self.search(h, opts) for h in haystacks]`: the haystacks as one pre-filtered batch
        (fac_search_batch_prefiltered; `_batch_parts`: all of them, or the ASCII ones and the others
        one by one), results in input order. `boundaries` (here and in the other batch calls): as the
        engine's; the documents searched one by one go through FuzzyMatches.retain_boundaries."""
        opts = opts or SearchOptions()
        haystacks = list(haystacks)
        enc = [h.encode("utf-8") for h in haystacks]
        out = [None] * len(haystacks)
        idx = self._batch_parts(enc)
        if idx:
            data, offsets = batch_offsets([enc[d] for d in idx])
            sb = StagedBatch(self.engine, data, offsets, unicode_prefilter=True, unicode_mappings=True,
                             boundaries=boundaries, anchors=anchors)
            recs, doc_off = sb.search_records(opts, prefilter=True)
            for k, d in enumerate(idx):
                rows = [(int(r["start"]), int(r["end"]), int(r["pattern_index"]), float(r["similarity"]),
                         int(r["insertions"]), int(r["deletions"]), int(r["substitutions"]), int(r["swaps"]),
                         int(r["edits"])) for r in recs[int(doc_off[k]):int(doc_off[k + 1])]]
                out[d] = self.engine._to_matches(haystacks[d], enc[d], rows)
        for d, h in enumerate(haystacks):
            if out[d] is None:
                out[d] = self.engine._search_bounded(h, opts.threshold_, opts.order_, opts.overlap_, True, boundaries, anchors)
        return out

    def count_batch(self, texts: Sequence[str], opts: SearchOptions = None, keys=None, n_keys=None,
                    boundaries: Boundary = Boundary.NONE, anchors: Anchor = Anchor.NONE) -> List[Dict[int, TermCount]]:
        """`engine.count_batch` over the pre-filtered search (fac_count_batch_prefiltered), routed as
        `search_batch` routes: the texts of `_batch_parts` as one batch, the others one by one through
        the host's FuzzyMatches.term_counts; results in input order."""
        opts = opts or SearchOptions()
        karr, nk = _key_table(self.engine, keys, n_keys)  # checked once, whichever route the texts take
        texts = list(texts)
        enc = [t.encode("utf-8") for t in texts]
        out = [None] * len(texts)
        idx = self._batch_parts(enc)
        if idx:
            data, offsets = batch_offsets([enc[d] for d in idx])
            sb = StagedBatch(self.engine, data, offsets, unicode_prefilter=True, unicode_mappings=True,
                             boundaries=boundaries, anchors=anchors)
            terms, doc_off, _ = sb.count_records(opts, keys, n_keys, prefilter=True)
            for d, terms_d in zip(idx, _term_dicts(terms, doc_off)):
                out[d] = terms_d
        if len(idx) < len(texts):
            for d, t in enumerate(texts):
                if out[d] is None:
                    out[d] = self.engine._search_bounded(t, opts.threshold_, opts.order_, opts.overlap_, True, boundaries,
                                                         anchors).term_counts(karr, nk if karr is not None else None)
        return out

    def replace_batch(self, texts: Sequence[str], opts: SearchOptions, replacements,
                      boundaries: Boundary = Boundary.NONE, anchors: Anchor = Anchor.NONE) -> List[str]:
        """`engine.replace_batch` over the pre-filtered search: the ASCII texts as one pre-filtered
        batch (fac_replace_batch_prefiltered), the others through `search` and the host splice of
        matches.rs:170-187, results in input order. `replacements`: one entry per pattern (None
        keeps the matched text), or a ReplacementTable built from such a list."""
        texts = list(texts)
        enc = [t.encode("utf-8") for t in texts]
        out = [None] * len(texts)
        idx = self._batch_parts(enc)
        if isinstance(replacements, ReplacementTable):
            table, reps = replacements, replacements.replacements
        else:
            reps = list(replacements)
            table = ReplacementTable(self.engine, reps) if idx else None
        if idx:
            data, offsets = batch_offsets([enc[d] for d in idx])
            sb = StagedBatch(self.engine, data, offsets, unicode_prefilter=True, unicode_mappings=True,
                             boundaries=boundaries, anchors=anchors)
            buf, off = sb.replace_bytes(table, opts, prefilter=True)
            for k, d in enumerate(idx):
                out[d] = buf[int(off[k]):int(off[k + 1])].decode("utf-8")
        order = Order.Default if opts.order_ == Order.Unsorted else opts.order_
        overlap = Overlap.NonOverlapping if opts.overlap_ == Overlap.Keep else opts.overlap_
        for d, t in enumerate(texts):
            if out[d] is None:
                ms = self.engine._search_bounded(t, opts.threshold_, order, overlap, True, boundaries, anchors)
                out[d] = ms.replace(lambda m: _rendered_entry(reps[m.pattern_index], m))
        return out

    def extract_batch(self, texts: Sequence[str], opts: SearchOptions, replacements=None,
                      boundaries: Boundary = Boundary.NONE, anchors: Anchor = Anchor.NONE) -> List[List[str]]:
        """`engine.extract_batch` over the pre-filtered search: the ASCII texts as one pre-filtered
        batch (fac_extract_batch_prefiltered), the others through `search`, results in input order."""
        opts = opts or SearchOptions()
        texts = list(texts)
        enc = [t.encode("utf-8") for t in texts]
        out = [None] * len(texts)
        idx = self._batch_parts(enc)
        if isinstance(replacements, ReplacementTable):
            table, reps = replacements, replacements.replacements
        else:
            reps = None if replacements is None else list(replacements)
            table = ReplacementTable(self.engine, reps) if idx and reps is not None else None
        if idx:
            for d, items in zip(idx, _extract_batch(self.engine, [enc[d] for d in idx], opts, table, True, True,
                                                  boundaries, anchors)):
                out[d] = items
        for d, t in enumerate(texts):
            if out[d] is None:
                out[d] = [_item_text(reps, m) for m in self.engine._search_bounded(
                    t, opts.threshold_, opts.order_, opts.overlap_, True, boundaries, anchors)]
        return out

    def matched_strings_batch(self, texts: Sequence[str], opts: SearchOptions = None,
                              boundaries: Boundary = Boundary.NONE, anchors: Anchor = Anchor.NONE) -> List[List[str]]:
        """`[self.search(t, opts).matched_strings() for t in texts]`, batched as extract_batch is."""
        return self.extract_batch(texts, opts, boundaries=boundaries, anchors=anchors)

    def _segmented(self, haystack: str, opts: SearchOptions, boundaries=Boundary.NONE, anchors=Anchor.NONE) -> FuzzyMatches:
        order = Order.Default if opts.order_ == Order.Unsorted else opts.order_
        overlap = Overlap.NonOverlapping if opts.overlap_ == Overlap.Keep else opts.overlap_
        return self.engine._search_bounded(haystack, opts.threshold_, order, overlap, True, boundaries, anchors)

    def _rendered(self, texts, mode: int, opts: SearchOptions, host, boundaries=Boundary.NONE, anchors=Anchor.NONE) -> List[str]:
        """The ASCII texts as one pre-filtered batch (fac_render_batch_prefiltered), the others
        through `search` and the host method `host`, results in input order."""
        texts = list(texts)
        enc = [t.encode("utf-8") for t in texts]
        out = [None] * len(texts)
        idx = self._batch_parts(enc)
        if idx:
            for d, r in zip(idx, _render_batch(self.engine, [texts[d] for d in idx], mode, opts, True, True, boundaries, anchors)):
                out[d] = r
        for d, t in enumerate(texts):
            if out[d] is None:
                out[d] = host(self._segmented(t, opts, boundaries, anchors))
        return out

    def strip_prefix_batch(self, texts: Sequence[str], opts: SearchOptions, boundaries: Boundary = Boundary.NONE,
                           anchors: Anchor = Anchor.NONE) -> List[str]:
        return self._rendered(texts, _native.FAC_RENDER_STRIP_PREFIX, opts, lambda ms: ms.strip_prefix(), boundaries, anchors)

    def strip_suffix_batch(self, texts: Sequence[str], opts: SearchOptions, boundaries: Boundary = Boundary.NONE,
                           anchors: Anchor = Anchor.NONE) -> List[str]:
        return self._rendered(texts, _native.FAC_RENDER_STRIP_SUFFIX, opts, lambda ms: ms.strip_suffix(), boundaries, anchors)

    def segment_text_batch(self, texts: Sequence[str], opts: SearchOptions, boundaries: Boundary = Boundary.NONE,
                           anchors: Anchor = Anchor.NONE) -> List[str]:
        return self._rendered(texts, _native.FAC_RENDER_SEGMENT_TEXT, opts, lambda ms: ms.segment_text(), boundaries, anchors)

    def segment_batch(self, texts: Sequence[str], opts: SearchOptions,
                      boundaries: Boundary = Boundary.NONE, anchors: Anchor = Anchor.NONE) -> List[List[Segment]]:
        """The ASCII texts as one pre-filtered batch (fac_segment_batch_prefiltered), the others
        through `search` and the host's segment_iter, results in input order."""
        texts = list(texts)
        enc = [t.encode("utf-8") for t in texts]
        out = [None] * len(texts)
        idx = self._batch_parts(enc)
        if idx:
            for d, segs in zip(idx, _segment_batch(self.engine, [texts[d] for d in idx], opts, True, True, boundaries, anchors)):
                out[d] = segs
        for d, t in enumerate(texts):
            if out[d] is None:
                out[d] = list(self._segmented(t, opts, boundaries, anchors).segment_iter())
        return out

    def split_batch(self, texts: Sequence[str], opts: SearchOptions,
                    boundaries: Boundary = Boundary.NONE, anchors: Anchor = Anchor.NONE) -> List[List[str]]:
        return [[s.unmatched().text for s in segs if s.unmatched() is not None]
                for segs in self.segment_batch(texts, opts, boundaries, anchors)]


def _key_table(engine: "FuzzyAhoCorasick", keys, n_keys):
    """(uint32 array or None, size of the key space) of a pattern -> key table for fac_count_batch,
    checked as the library checks it (fac.h "Term counts of a batch"): without a table the key space is
    the pattern count, whether `n_keys` is None, 0 or that count; with one, every key is below
    `n_keys` (None: the greatest key + 1). Every buffer sized by the caller uses the size returned
    here, which is also what the library is given."""
    import numpy as np
    n_pat = len(engine.patterns_)
    if keys is None:
        if n_keys is not None and int(n_keys) not in (0, n_pat):
            raise DeviceError(_native.FAC_E_INVALID, "n_keys must be 0 or the pattern count when keys is None")
        return None, n_pat
    wide = np.asarray(keys, dtype=np.int64)
    if wide.shape != (n_pat,):
        raise ValueError("keys needs one entry per pattern")
    top = int(wide.max()) if len(wide) else -1
    if len(wide) and (int(wide.min()) < 0 or top > 0xFFFFFFFF):
        raise DeviceError(_native.FAC_E_INVALID, "keys must be 32-bit unsigned")
    nk = top + 1 if n_keys is None else int(n_keys)
    if not 0 <= nk <= 0xFFFFFFFF or top >= nk:
        raise DeviceError(_native.FAC_E_INVALID, "a key is not below n_keys (at most 2^32 - 1)")
    return np.ascontiguousarray(wide.astype(np.uint32)), nk


def _term_dicts(terms, doc_off) -> List[Dict[int, TermCount]]:
    """count_records' (terms, doc_offsets) as one {key: TermCount} per document."""
    key, cnt, sim, pat = (terms[f].tolist() for f in ("key", "count", "best_similarity", "best_pattern"))
    off = [int(x) for x in doc_off]
    return [{key[i]: TermCount(cnt[i], sim[i], pat[i]) for i in range(off[d], off[d + 1])} for d in range(len(off) - 1)]


def _as_text(r):
    return bytes(r).decode("utf-8") if isinstance(r, (bytes, bytearray, memoryview)) else r


def _item_text(reps, m) -> str:
    """The item fac_extract_batch gives the match m: its entry's replacement, or the matched text
    where there is no table or the entry is "keep"."""
    r = None if reps is None else _rendered_entry(reps[m.pattern_index], m)
    return m.text if r is None else r


def _extract_batch(engine: "FuzzyAhoCorasick", enc, opts: SearchOptions, table, prefilter: bool,
                   unicode_mappings: bool = False, boundaries=Boundary.NONE, anchors=Anchor.NONE) -> List[List[str]]:
    data, offsets = batch_offsets(enc)
    sb = StagedBatch(engine, data, offsets, unicode_prefilter=prefilter, unicode_mappings=unicode_mappings,
                     boundaries=boundaries, anchors=anchors)
    _, doc_off, text, item_off = sb.extract(table, opts, prefilter=prefilter)
    return [[text[int(item_off[i]):int(item_off[i + 1])].decode("utf-8")
             for i in range(int(doc_off[d]), int(doc_off[d + 1]))] for d in range(len(enc))]


def _render_batch(engine: "FuzzyAhoCorasick", texts, mode: int, opts: SearchOptions, prefilter: bool,
                  unicode_mappings: bool = False, boundaries=Boundary.NONE, anchors=Anchor.NONE) -> List[str]:
    enc = [t.encode("utf-8") for t in texts]
    data, offsets = batch_offsets(enc)
    sb = StagedBatch(engine, data, offsets, unicode_prefilter=prefilter, unicode_mappings=unicode_mappings,
                     boundaries=boundaries, anchors=anchors)
    out, off = sb.render_bytes(mode, opts, prefilter=prefilter)
    return [out[int(off[d]):int(off[d + 1])].decode("utf-8") for d in range(len(enc))]


def _segment_batch(engine: "FuzzyAhoCorasick", texts, opts: SearchOptions, prefilter: bool,
                   unicode_mappings: bool = False, boundaries=Boundary.NONE, anchors=Anchor.NONE) -> List[List[Segment]]:
    enc = [t.encode("utf-8") for t in texts]
    data, offsets = batch_offsets(enc)
    sb = StagedBatch(engine, data, offsets, unicode_prefilter=prefilter, unicode_mappings=unicode_mappings,
                     boundaries=boundaries, anchors=anchors)
    recs, doc_off = sb.segment_records(opts, prefilter=prefilter)
    out = []
    for d, raw in enumerate(enc):
        segs = []
        for r in recs[int(doc_off[d]):int(doc_off[d + 1])]:
            s, e, p = int(r["start"]), int(r["end"]), int(r["pattern_index"])
            text = raw[s:e].decode("utf-8")
            if p == _native.FAC_UNMATCHED:
                segs.append(Segment(unmatched=UnmatchedSegment(s, e, text)))
            else:
                segs.append(Segment(matched=FuzzyMatch(int(r["insertions"]), int(r["deletions"]), int(r["substitutions"]),
                                                       int(r["swaps"]), int(r["edits"]), p, engine.patterns_[p], s, e,
                                                       float(r["similarity"]), text)))
        out.append(segs)
    return out


def prefilter_windows(engine: "FuzzyAhoCorasick", haystack: str, threshold: float):
    """Diagnostics: merged bitap candidate windows (grapheme ranges), or None on fallback."""
    data = haystack.encode("utf-8")
    cap = 2 * len(data) + 16
    buf = (ctypes.c_uint64 * (2 * cap))()
    n = _native.lib.fac_prefilter_windows(engine._h, data, len(data), f32(threshold), buf, cap)
    if n < 0:
        return None
    return [(buf[2 * i], buf[2 * i + 1]) for i in range(n)]


# read() size of the streaming methods. The library cuts windows as the crate's WindowReader does with
# its 64 KiB reads (stream.rs:94, 102-158) whatever the feed size, so a larger read only means fewer
# calls across the C ABI (and lets a feed fill whole batches of windows).
READ_CHUNK = 4 << 20


class StreamMatch:
    """stream.rs:33-59: a match with absolute (stream-wide) byte offsets and its owned text."""
    __slots__ = ("start", "end", "pattern_index", "similarity", "insertions", "deletions", "substitutions",
                 "swaps", "edits", "text")

    def __init__(self, row, text: str):
        (self.start, self.end, self.pattern_index, self.similarity, self.insertions, self.deletions,
         self.substitutions, self.swaps, self.edits) = row
        self.text = text

    def __repr__(self):
        return f"StreamMatch({self.start}..{self.end} p{self.pattern_index} {self.similarity:.4f} {self.text!r})"


class _Stream:
    """fac_stream: WindowReader + per-window search on the GPU (stream.rs:77-297)."""

    def __init__(self, engine: "FuzzyAhoCorasick", threshold: float, window: int = 0, prefilter: bool = False,
                 boundaries: Boundary = Boundary.NONE):
        h = ctypes.c_void_p()
        o = _native.fac_stream_options(f32(threshold), window, int(bool(prefilter)), int(boundaries))
        rc = _native.lib.fac_stream_open_opts(engine._h, ctypes.byref(o), ctypes.byref(h))
        if rc:
            _raise(rc)
        self._h = h
        self.engine = engine

    def feed(self, data: bytes, eof: bool = False) -> List[StreamMatch]:
        out = ctypes.POINTER(_native.fac_match)()
        n = ctypes.c_uint64()
        text = ctypes.POINTER(ctypes.c_uint8)()
        tlen = ctypes.c_uint64()
        rc = _native.lib.fac_stream_feed(self._h, data, len(data), int(eof), ctypes.byref(out), ctypes.byref(n),
                                         ctypes.byref(text), ctypes.byref(tlen))
        if rc:
            _raise(rc)
        raw = ctypes.string_at(text, tlen.value) if tlen.value else b""
        _native.lib.fac_buffer_free(text)
        res, pos = [], 0
        for row in _native.take_matches(out, n.value):
            k = row[1] - row[0]
            res.append(StreamMatch(row, raw[pos:pos + k].decode("utf-8")))
            pos += k
        return res

    def total(self) -> int:
        return int(_native.lib.fac_stream_total(self._h))

    def committed(self) -> int:
        return int(_native.lib.fac_stream_committed(self._h))

    def windows_searched(self) -> int:
        """Start windows of the segments searched for the windows handed out so far."""
        return int(_native.lib.fac_stream_windows_searched(self._h))

    def task_counts(self) -> Tuple[int, int]:
        """(batched, single): the device tasks handed out so far that were searched in one pass, and
        window by window."""
        b, s = ctypes.c_uint64(), ctypes.c_uint64()
        _native.lib.fac_stream_task_counts(self._h, ctypes.byref(b), ctypes.byref(s))
        return int(b.value), int(s.value)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _native.lib is not None:
            _native.lib.fac_stream_close(h)
            self._h = None


class _ReplaceStream:
    """fac_replace_stream: WindowReader + per-window search + the ReplaceCursor splice on the GPU
    (stream.rs:465-517, 645-705) against a ReplacementTable."""

    def __init__(self, engine: "FuzzyAhoCorasick", table: "ReplacementTable", threshold: float, window: int = 0,
                 prefilter: bool = False, boundaries: Boundary = Boundary.NONE):
        h = ctypes.c_void_p()
        o = _native.fac_stream_options(f32(threshold), window, int(bool(prefilter)), int(boundaries))
        rc = _native.lib.fac_replace_stream_open_opts(engine._h, table._h, ctypes.byref(o), ctypes.byref(h))
        if rc:
            _raise(rc)
        self._h = h
        self.engine, self.table = engine, table  # (the table must outlive the stream)

    def feed(self, data: bytes, eof: bool = False) -> bytes:
        """The output completed so far, in stream order."""
        out = ctypes.POINTER(ctypes.c_uint8)()
        n = ctypes.c_uint64()
        rc = _native.lib.fac_replace_stream_feed(self._h, data, len(data), int(eof), ctypes.byref(out), ctypes.byref(n))
        if rc:
            _raise(rc)
        try:
            return ctypes.string_at(out, n.value) if n.value else b""
        finally:
            _native.lib.fac_buffer_free(out)

    def written(self) -> int:
        return int(_native.lib.fac_replace_stream_written(self._h))

    def windows_searched(self) -> int:
        """Start windows of the segments searched for the output handed out so far."""
        return int(_native.lib.fac_replace_stream_windows_searched(self._h))

    def task_counts(self) -> Tuple[int, int]:
        """(batched, single): the device tasks handed out so far that were searched in one pass, and
        window by window."""
        b, s = ctypes.c_uint64(), ctypes.c_uint64()
        _native.lib.fac_replace_stream_task_counts(self._h, ctypes.byref(b), ctypes.byref(s))
        return int(b.value), int(s.value)

    def counts(self) -> Tuple[int, int]:
        """(records replaced, records skipped by the cursor's guard) in the output handed out so far."""
        a, k = ctypes.c_uint64(), ctypes.c_uint64()
        _native.lib.fac_replace_stream_counts(self._h, ctypes.byref(a), ctypes.byref(k))
        return int(a.value), int(k.value)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _native.lib is not None:
            _native.lib.fac_replace_stream_close(h)
            self._h = None


class StagedHaystack:
    """A haystack staged into HBM once (fac_haystack_stage) and searched many times.

    `StagedHaystack.shard(engine, data, n, r)` stages only shard r of n of `data` (its owned bytes
    plus the halo, fac_shard_plan): searching it yields search_raw's records for the shard's start
    windows at global byte offsets."""

    def __init__(self, engine: FuzzyAhoCorasick, data: bytes, _shard=None):
        self.engine = engine
        self.data = data
        h = ctypes.c_void_p()
        eg = ctypes.c_uint64()
        if _shard is None:
            rc = _native.lib.fac_haystack_stage(engine._h, data, len(data), ctypes.byref(h), ctypes.byref(eg))
            self.base, self.owned_bytes, self.open_end, self.plan = 0, len(data), False, None
        else:
            a, b, e, asc, open_end = _shard
            piece = data[a:e]
            rc = _native.lib.fac_haystack_stage_shard(engine._h, piece, len(piece), b - a, int(asc), int(open_end), a,
                                                      ctypes.byref(h), ctypes.byref(eg))
            self.base, self.owned_bytes, self.open_end, self.plan = a, b - a, open_end, _shard
        if rc:
            _raise(rc, eg.value)
        self._h = h
        self.graphemes = int(_native.lib.fac_haystack_graphemes(h))
        self.owned_windows = int(_native.lib.fac_haystack_owned_windows(h))
        self._dev_out = None  # growable device record buffer (search_device)

    @classmethod
    def from_device(cls, engine: FuzzyAhoCorasick, d_utf8: int, length: int, stream=None,
                    reuse: "StagedHaystack" = None) -> "StagedHaystack":
        """fac_haystack_stage_device: search_raw's staging (UTF-8 check, is_ascii, UAX #29 segmentation
        and folding, search.rs:196-203/296-302) of `length` bytes already in HBM at device address
        `d_utf8` (borrowed: keep the buffer alive). `reuse`: a haystack staged this way before, whose
        device buffers are reused (it is restaged in place and returned)."""
        h = ctypes.c_void_p(reuse._h.value if reuse is not None else None)
        eg = ctypes.c_uint64()
        rc = _native.lib.fac_haystack_stage_device(engine._h, ctypes.c_void_p(d_utf8), length, ctypes.c_void_p(stream or 0),
                                                   ctypes.byref(h), ctypes.byref(eg))
        if rc:
            if reuse is not None:  # a failed restage leaves the haystack empty (and searchable)
                reuse.owned_bytes, reuse.graphemes, reuse.owned_windows = 0, 0, 0
            _raise(rc, eg.value)
        obj = reuse
        if obj is None:
            obj = cls.__new__(cls)
            obj.engine, obj.data, obj._h, obj._dev_out = engine, None, h, None
            obj.base, obj.open_end, obj.plan = 0, False, None
        obj.owned_bytes = length
        obj.graphemes = int(_native.lib.fac_haystack_graphemes(obj._h))
        obj.owned_windows = int(_native.lib.fac_haystack_owned_windows(obj._h))
        return obj

    @classmethod
    def shard(cls, engine: FuzzyAhoCorasick, data: bytes, n_shards: int, shard: int, is_ascii: int = -1):
        plan = _native.shard_plan(engine.max_match_graphemes(), data, n_shards, shard, is_ascii)
        return cls(engine, data, _shard=plan)

    @classmethod
    def shard_from_device(cls, engine: FuzzyAhoCorasick, d_utf8: int, plan, stream=None,
                          reuse: "StagedHaystack" = None) -> "StagedHaystack":
        """fac_haystack_stage_shard_device: shard `plan` (a, b, e, global_ascii, open_end from
        _native.shard_plan) whose bytes [a, e) are already in HBM at `d_utf8` (borrowed), staged on the
        device like from_device (the per-step staging of a sharded search_raw). `reuse`: a shard
        staged this way before, restaged in place."""
        a, b, e, asc, open_end = plan
        h = ctypes.c_void_p(reuse._h.value if reuse is not None else None)
        eg = ctypes.c_uint64()
        rc = _native.lib.fac_haystack_stage_shard_device(engine._h, ctypes.c_void_p(d_utf8), e - a, b - a, int(asc),
                                                         int(open_end), a, ctypes.c_void_p(stream or 0),
                                                         ctypes.byref(h), ctypes.byref(eg))
        if rc:
            if reuse is not None:
                reuse.owned_bytes, reuse.graphemes, reuse.owned_windows = 0, 0, 0
            _raise(rc, eg.value)
        obj = reuse
        if obj is None:
            obj = cls.__new__(cls)
            obj.engine, obj.data, obj._h, obj._dev_out = engine, None, h, None
        obj.base, obj.open_end, obj.plan, obj.owned_bytes = a, open_end, plan, b - a
        obj.graphemes = int(_native.lib.fac_haystack_graphemes(obj._h))
        obj.owned_windows = int(_native.lib.fac_haystack_owned_windows(obj._h))
        return obj

    def set_key_partition(self, parts: int, part: int) -> "StagedHaystack":
        """fac_haystack_set_key_partition: later searches cover only the start windows whose first two
        characters hash to `part` of `parts` (a strong-scaling split that keeps whole prefix-cache keys
        on one GPU). parts = 1 restores the whole haystack."""
        rc = _native.lib.fac_haystack_set_key_partition(self.engine._h, self._h, parts, part)
        if rc:
            _raise(rc)
        self.key_partition = (parts, part)
        return self

    def search_device(self, threshold: float, window_begin: int = 0, window_end: int = None, stream=None,
                      auto_beam_prefix: int = 0, torch_device=None):
        """fac_search_staged_ex with the records left in HBM: (uint8 tensor of n * 32 bytes on the
        engine's device, n, fac_stats). The buffer is reused across calls and grown on demand."""
        import torch
        dev = torch_device or torch.device("cuda", self.engine.device)
        if window_end is None:
            window_end = self.graphemes
        while True:
            if self._dev_out is None:
                self._dev_out = torch.empty(max(4096, self.owned_windows // 64) * 32, dtype=torch.uint8, device=dev)
            a = _native.fac_search_args(window_begin, window_end, f32(threshold), ctypes.c_void_p(stream or 0),
                                        auto_beam_prefix, ctypes.c_void_p(self._dev_out.data_ptr()),
                                        self._dev_out.numel() // 32)
            n = ctypes.c_uint64()
            st = _native.fac_stats()
            rc = _native.lib.fac_search_staged_ex(self.engine._h, self._h, ctypes.byref(a), None, ctypes.byref(n),
                                                  ctypes.byref(st))
            if rc == _native.FAC_E_OUTPUT_CAPACITY:
                self._dev_out = torch.empty(int(n.value * 1.25 + 1024) * 32, dtype=torch.uint8, device=dev)
                continue
            if rc:
                _raise(rc)
            return self._dev_out[: n.value * 32], int(n.value), st

    def auto_beam_total(self, threshold: float, window_begin: int = 0, window_end: int = None, stream=None) -> int:
        """fac_auto_beam_total: sum of queue.len() over the windows searched unbeamed."""
        if window_end is None:
            window_end = self.graphemes
        t = ctypes.c_uint64()
        rc = _native.lib.fac_auto_beam_total(self.engine._h, self._h, window_begin, window_end, f32(threshold),
                                             ctypes.c_void_p(stream or 0), ctypes.byref(t))
        if rc:
            _raise(rc)
        return int(t.value)

    def grapheme_starts(self):
        """fac_haystack_grapheme_starts: the byte start of every staged grapheme (the device
        segmentation's result), as a NumPy uint64 array."""
        import numpy as np
        out = np.zeros(max(1, self.graphemes), dtype=np.uint64)
        n = _native.lib.fac_haystack_grapheme_starts(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                                     self.graphemes)
        return out[: min(int(n), self.graphemes)]

    def text_chars(self):
        """fac_haystack_text_chars: the folded first code point of every staged grapheme, as the device
        staging wrote it, as a NumPy uint32 array (empty for an ASCII haystack, which has none)."""
        import numpy as np
        out = np.zeros(max(1, self.graphemes), dtype=np.uint32)
        n = _native.lib.fac_haystack_text_chars(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                                self.graphemes)
        return out[: min(int(n), self.graphemes)]

    def symbol_ids(self, stream=None):
        """fac_haystack_symbol_ids: the bitap pre-filter's symbol id of every staged grapheme
        (prefilter.rs:247-281), computed on the device, as a NumPy uint8 array; None when the engine
        has no filter."""
        import numpy as np
        out = np.zeros(max(1, self.graphemes), dtype=np.uint8)
        n = _native.lib.fac_haystack_symbol_ids(self.engine._h, self._h, ctypes.c_void_p(stream or 0),
                                                ctypes.c_void_p(out.ctypes.data), self.graphemes)
        if n == -1:
            return None
        if n < 0:
            _raise(int(-n))
        return out[: int(n)]

    def grapheme_ids(self, stream=None, engine=None):
        """fac_haystack_grapheme_ids: the id in the grapheme dictionary of `engine` (default: the
        haystack's; 0 = not in it) of every staged grapheme of a Unicode haystack, looked up on the
        device, as a NumPy uint32 array (empty for an ASCII haystack); None when the engine has no
        mappings."""
        import numpy as np
        out = np.zeros(max(1, self.graphemes), dtype=np.uint32)
        n = _native.lib.fac_haystack_grapheme_ids((engine or self.engine)._h, self._h, ctypes.c_void_p(stream or 0),
                                                  ctypes.c_void_p(out.ctypes.data), self.graphemes)
        if n == -1:
            return None
        if n < 0:
            _raise(int(-n))
        return out[: int(n)]

    def stream_window(self, g_begin: int, g_end: int, commit_bytes: int, base: int, threshold: float,
                      prefilter: bool, stream=None):
        """fac_stream_window_staged (stream.rs:262-297 window_matches on a device-resident window):
        NumPy records (MATCH_DTYPE) of the window's owned matches at absolute offsets + fac_stats."""
        out = ctypes.POINTER(_native.fac_match)()
        n = ctypes.c_uint64()
        st = _native.fac_stats()
        rc = _native.lib.fac_stream_window_staged(self.engine._h, self._h, g_begin, g_end, commit_bytes, base,
                                                  f32(threshold), int(prefilter), ctypes.c_void_p(stream or 0),
                                                  ctypes.byref(out), ctypes.byref(n), ctypes.byref(st))
        if rc:
            _raise(rc)
        return _native.take_records(out, n.value), st

    def stream_window_device(self, g_begin: int, g_end: int, commit_bytes: int, base: int, threshold: float,
                             prefilter: bool, out, offset: int = 0, stream=None):
        """fac_stream_window_staged_device: the window's owned records (stream.rs:262-297) written in HBM
        to `out` (a uint8 CUDA tensor of 32-byte records) from record `offset` on, never visiting the
        host; `out` is grown (a new tensor, the records before `offset` copied) when it is too small.
        Returns (out, owned count, fac_stats)."""
        import torch
        n = ctypes.c_uint64()
        st = _native.fac_stats()
        while True:
            cap = out.numel() // _native.REC_BYTES - offset
            ptr = out.data_ptr() + offset * _native.REC_BYTES
            rc = _native.lib.fac_stream_window_staged_device(
                self.engine._h, self._h, g_begin, g_end, commit_bytes, base, f32(threshold), int(prefilter),
                ctypes.c_void_p(stream or 0), ctypes.c_void_p(ptr), max(0, cap), ctypes.byref(n), ctypes.byref(st))
            if rc == _native.FAC_E_OUTPUT_CAPACITY:
                grown = torch.empty(max(2 * out.numel(), (offset + n.value) * _native.REC_BYTES * 2),
                                    dtype=torch.uint8, device=out.device)
                grown[: offset * _native.REC_BYTES].copy_(out[: offset * _native.REC_BYTES])
                out = grown
                continue
            if rc:
                _raise(rc)
            return out, n.value, st

    def stream_windows_device(self, windows, threshold: float, prefilter: bool, out, offset: int = 0, stream=None):
        """fac_stream_windows_staged_device: a batch of stream windows, `windows` = [(g_begin, g_end,
        commit_bytes, base), ...] in stream order, searched together (one pre-filter pass and one search
        launch on an ASCII haystack); their owned records, in window order, written in HBM to `out`
        from record `offset` on (grown like stream_window_device). Returns (out, owned count, fac_stats)."""
        import numpy as np
        import torch
        arr = np.ascontiguousarray(np.asarray(windows, dtype=np.uint64).reshape(-1, 4))
        wp = arr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        n = ctypes.c_uint64()
        st = _native.fac_stats()
        while True:
            cap = out.numel() // _native.REC_BYTES - offset
            ptr = out.data_ptr() + offset * _native.REC_BYTES
            rc = _native.lib.fac_stream_windows_staged_device(
                self.engine._h, self._h, wp, len(arr), f32(threshold), int(prefilter), ctypes.c_void_p(stream or 0),
                ctypes.c_void_p(ptr), max(0, cap), ctypes.byref(n), ctypes.byref(st))
            if rc == _native.FAC_E_OUTPUT_CAPACITY:
                grown = torch.empty(max(2 * out.numel(), (offset + n.value) * _native.REC_BYTES * 2),
                                    dtype=torch.uint8, device=out.device)
                grown[: offset * _native.REC_BYTES].copy_(out[: offset * _native.REC_BYTES])
                out = grown
                continue
            if rc:
                _raise(rc)
            return out, n.value, st

    def replace_windows_device(self, windows, table: "ReplacementTable", threshold: float, prefilter: bool, out,
                               emitted: int = 0, stream=None):
        """fac_replace_windows_staged_device: streaming replace (stream.rs:465-517 + ReplaceCursor::
        emit_window, :645-705) of a run of consecutive stream windows, `windows` as in
        stream_windows_device, spliced on the device from the staged text into `out` (a uint8 CUDA
        tensor). `emitted`: the cursor on entry (what the previous call returned, 0 at the start of a
        stream). Returns (the filled part of `out`, the cursor on return, records applied, records
        skipped, fac_stats). FAC_E_OUTPUT_CAPACITY is raised as DeviceError with `.needed` bytes and
        `.emitted`, the cursor the call left, when `out` is too small (nothing is written, the cursor
        does not move)."""
        import numpy as np
        arr = np.ascontiguousarray(np.asarray(windows, dtype=np.uint64).reshape(-1, 4))
        wp = arr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        em = ctypes.c_uint64(emitted)
        n, na, ns = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        st = _native.fac_stats()
        cap = out.numel() * out.element_size()
        rc = _native.lib.fac_replace_windows_staged_device(
            self.engine._h, self._h, wp, len(arr), table._h, f32(threshold), int(prefilter), ctypes.c_void_p(stream or 0),
            ctypes.byref(em), ctypes.c_void_p(out.data_ptr() if cap else 0), cap, ctypes.byref(n), ctypes.byref(na),
            ctypes.byref(ns), ctypes.byref(st))
        if rc:
            try:
                _raise(rc)
            except DeviceError as ex:
                ex.needed, ex.emitted = int(n.value), int(em.value)
                raise
        return out[: n.value], int(em.value), int(na.value), int(ns.value), st

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _native.lib is not None:
            _native.lib.fac_haystack_free(h)
            self._h = None

    def search_windows(self, threshold: float, window_begin: int = 0, window_end: int = None, stream=None):
        """Raw rows (start, end, pattern, sim, ins, del, sub, swp, edits) + fac_stats."""
        if window_end is None:
            window_end = self.graphemes
        out = ctypes.POINTER(_native.fac_match)()
        n = ctypes.c_uint64()
        st = _native.fac_stats()
        rc = _native.lib.fac_search_staged(self.engine._h, self._h, window_begin, window_end, f32(threshold),
                                           ctypes.c_void_p(stream or 0), ctypes.byref(out), ctypes.byref(n),
                                           ctypes.byref(st))
        if rc:
            _raise(rc)
        return _native.take_matches(out, n.value), st

    def search_windows_records(self, threshold: float, window_begin: int = 0, window_end: int = None,
                               stream=None):
        """search_windows returning a NumPy array of 32-byte match records (MATCH_DTYPE)."""
        if window_end is None:
            window_end = self.graphemes
        out = ctypes.POINTER(_native.fac_match)()
        n = ctypes.c_uint64()
        st = _native.fac_stats()
        t0 = time.perf_counter()
        rc = _native.lib.fac_search_staged(self.engine._h, self._h, window_begin, window_end, f32(threshold),
                                           ctypes.c_void_p(stream or 0), ctypes.byref(out), ctypes.byref(n),
                                           ctypes.byref(st))
        if rc:
            _raise(rc)
        t1 = time.perf_counter()
        rows = _native.take_records(out, n.value)
        if _TIMING:
            print(f"FAC_TIMING native call {1e3 * (t1 - t0):.2f} ms, records to NumPy {1e3 * (time.perf_counter() - t1):.2f} ms",
                  file=sys.stderr)
        return rows, st

    def search_prefiltered_records(self, threshold: float, stream=None):
        out = ctypes.POINTER(_native.fac_match)()
        n = ctypes.c_uint64()
        st = _native.fac_stats()
        rc = _native.lib.fac_search_staged_prefiltered(self.engine._h, self._h, f32(threshold),
                                                       ctypes.c_void_p(stream or 0), ctypes.byref(out),
                                                       ctypes.byref(n), ctypes.byref(st))
        if rc:
            _raise(rc)
        return _native.take_records(out, n.value), st

    def search_prefiltered(self, threshold: float, stream=None):
        """Prefiltered::raw on the device-resident text (prefilter.rs:146-155, 304-374): raw rows
        (best per (start, end, pattern), sorted) + fac_stats (prefilter_ms = bitap + merge)."""
        out = ctypes.POINTER(_native.fac_match)()
        n = ctypes.c_uint64()
        st = _native.fac_stats()
        rc = _native.lib.fac_search_staged_prefiltered(self.engine._h, self._h, f32(threshold),
                                                       ctypes.c_void_p(stream or 0), ctypes.byref(out),
                                                       ctypes.byref(n), ctypes.byref(st))
        if rc:
            _raise(rc)
        return _native.take_matches(out, n.value), st


def batch_offsets(docs) -> Tuple[bytes, List[int]]:
    """(concatenated bytes, offsets) of a list of `bytes` documents: document d is
    data[offsets[d]:offsets[d + 1]] (the layout fac_batch_stage takes). Pure Python."""
    offsets = [0]
    for d in docs:
        if not isinstance(d, (bytes, bytearray, memoryview)):
            raise TypeError(f"batch documents must be bytes, got {type(d).__name__}")
        offsets.append(offsets[-1] + len(d))
    return b"".join(bytes(d) for d in docs), offsets


def _raise_batch(rc: int, doc: int, graphemes: int):
    try:
        _raise(rc, graphemes)
    except SearchError as ex:
        ex.doc = doc  # the first offending document (None: not a per-document error)
        raise


class StagedBatch:
    """A batch of independent documents staged into HBM once (fac_batch_stage) and searched many
    times: document d is data[offsets[d]:offsets[d + 1]], staged as if it were staged alone (UTF-8
    validity, is_ascii and grapheme segmentation per document)."""

    def __init__(self, engine: FuzzyAhoCorasick, data: bytes, offsets, unicode_prefilter: bool = False,
                 unicode_mappings: bool = False, boundaries: Boundary = Boundary.NONE, anchors: Anchor = Anchor.NONE):
        import numpy as np
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        if off.ndim != 1 or len(off) < 1:
            raise ValueError("offsets needs n_docs + 1 entries")
        if int(off[-1]) != len(data) or (len(off) > 1 and int(off.max()) > len(data)):
            # (the library cannot see the length of `data`: keep its reads inside the buffer)
            raise DeviceError(_native.FAC_E_INVALID, "batch offsets must end at len(data) and stay inside it")
        self.engine, self.data, self.n_docs = engine, data, len(off) - 1
        h = ctypes.c_void_p()
        ed = ctypes.c_uint64(0xFFFFFFFFFFFFFFFF)
        eg = ctypes.c_uint64()
        rc = _native.lib.fac_batch_stage(engine._h, data, off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                         self.n_docs, ctypes.byref(h), ctypes.byref(ed), ctypes.byref(eg))
        if rc:
            _raise_batch(rc, None if ed.value == 0xFFFFFFFFFFFFFFFF else ed.value, eg.value)
        self._h = h
        self._dev_out = self._dev_doc = None
        if unicode_prefilter:
            self.allow_unicode_prefilter()
        if unicode_mappings:
            self.allow_unicode_mappings()
        if int(boundaries):
            self.require_boundaries(boundaries)
        if int(anchors):
            self.require_anchors(anchors)

    @classmethod
    def from_device(cls, engine: FuzzyAhoCorasick, d_utf8: int, d_offsets: int, n_docs: int, total_len: int,
                    stream=None, reuse: "StagedBatch" = None, unicode_prefilter: bool = False,
                    unicode_mappings: bool = False, boundaries: Boundary = None, anchors: Anchor = None) -> "StagedBatch":
        """fac_batch_stage_device: the bytes (`d_utf8`, total_len of them) and the n_docs + 1 uint64
        offsets (`d_offsets`) are device addresses, e.g. torch tensors' data_ptr() (borrowed: keep both
        alive). `reuse`: a batch staged this way before, restaged in place and returned (it keeps its
        opt-ins and its require_boundaries mask). `unicode_prefilter`, `unicode_mappings`: opt the batch
        in (allow_unicode_prefilter, allow_unicode_mappings). `boundaries`: require_boundaries (None:
        a reused batch keeps what it had). `anchors`: require_anchors, likewise."""
        h = ctypes.c_void_p(reuse._h.value if reuse is not None else None)
        ed = ctypes.c_uint64(0xFFFFFFFFFFFFFFFF)
        eg = ctypes.c_uint64()
        rc = _native.lib.fac_batch_stage_device(engine._h, ctypes.c_void_p(d_utf8), ctypes.c_void_p(d_offsets), n_docs,
                                                total_len, ctypes.c_void_p(stream or 0), ctypes.byref(h),
                                                ctypes.byref(ed), ctypes.byref(eg))
        if rc:
            if reuse is not None:  # a failed restage leaves the batch empty
                reuse.n_docs = 0
            _raise_batch(rc, None if ed.value == 0xFFFFFFFFFFFFFFFF else ed.value, eg.value)
        obj = reuse
        if obj is None:
            obj = cls.__new__(cls)
            obj.engine, obj.data, obj._h = engine, None, h
            obj._dev_out = obj._dev_doc = None
        obj.n_docs = n_docs
        if unicode_prefilter:
            obj.allow_unicode_prefilter()
        if unicode_mappings:
            obj.allow_unicode_mappings()
        if boundaries is not None:
            obj.require_boundaries(boundaries)
        if anchors is not None:
            obj.require_anchors(anchors)
        return obj

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _native.lib is not None:
            _native.lib.fac_batch_free(h)
            self._h = None

    def allow_unicode_prefilter(self, on: bool = True) -> "StagedBatch":
        """fac_batch_allow_unicode_prefilter: the `prefilter=True` calls take this batch even if it
        holds non-ASCII documents (default off: they raise UnsupportedConfiguration for such a batch).
        An all-ASCII batch is handled the same either way. Returns self."""
        rc = _native.lib.fac_batch_allow_unicode_prefilter(self._h, 1 if on else 0)
        if rc:
            _raise(rc)
        return self

    def allow_unicode_mappings(self, on: bool = True) -> "StagedBatch":
        """fac_batch_allow_unicode_mappings: an engine with multi-character mappings takes this batch
        even if it holds non-ASCII documents (default off: every batch call raises
        UnsupportedConfiguration for such a batch). Returns self."""
        rc = _native.lib.fac_batch_allow_unicode_mappings(self._h, 1 if on else 0)
        if rc:
            _raise(rc)
        return self

    def require_boundaries(self, sides) -> "StagedBatch":
        """fac_batch_require_boundaries: every later call on this batch, plain or pre-filtered, keeps
        only the raw records whose sides `sides` (structs.Boundary; 0 = off) are word boundaries of
        their own document, before ranking and overlap resolution (DESIGN.md 6a "Whole-token
        matches"). Sets a flag and does no work. Returns self."""
        rc = _native.lib.fac_batch_require_boundaries(self._h, int(sides))
        if rc:
            _raise(rc)
        return self

    def require_anchors(self, sides) -> "StagedBatch":
        """fac_batch_require_anchors: every later call on this batch, plain or pre-filtered, keeps only
        the raw records that start at byte 0 of their own document (Anchor.START), end at its end
        (Anchor.END) or both (Anchor.WHOLE; 0 = off), before ranking and overlap resolution
        (DESIGN.md 6a "Anchored matches"). A plain call then searches only the start windows such a
        record can come from. Sets a flag and does no work. Returns self."""
        rc = _native.lib.fac_batch_require_anchors(self._h, int(sides))
        if rc:
            _raise(rc)
        return self

    def lookup_records(self, opts: SearchOptions = None, k: int = 1, out=None, stream=None, stats=None):
        """fac_lookup_batch: (records[n_docs, k], found). Row d holds the first min(k, m_d) of document
        d's whole-string matches (both ends anchored, whatever require_anchors says) in the order
        `opts` names (Unsorted is taken as Default; the overlap mode is not used: such matches all
        cover the document), the other slots `pattern_index == _native.FAC_UNMATCHED` and zeros;
        found[d] (uint32) = min(k, m_d). `out`: a uint8 CUDA tensor of at least n_docs * k * 32 bytes
        to leave the table in HBM: returns (its filled part, found); too small raises DeviceError
        (FAC_E_OUTPUT_CAPACITY) with `.needed` records and writes nothing."""
        import numpy as np
        opts = opts or SearchOptions()
        a = _native.fac_lookup_args()
        a.threshold = f32(opts.threshold_)
        a.order = opts.order_.value
        a.k = int(k)
        a.stream = stream or None
        found = np.zeros(self.n_docs, dtype=np.uint32)
        ptr = ctypes.POINTER(_native.fac_match)()
        total = self.n_docs * int(k)
        if out is not None:
            a.device_out = out.data_ptr()
            a.device_cap = out.numel() // _native.REC_BYTES
        rc = _native.lib.fac_lookup_batch(self.engine._h, self._h, ctypes.byref(a),
                                          None if out is not None else ctypes.byref(ptr),
                                          found.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                          ctypes.byref(stats) if stats is not None else None)
        if rc:
            try:
                _raise(rc)
            except DeviceError as ex:
                ex.needed = total
                raise
        if out is not None:
            return out[: total * _native.REC_BYTES], found
        return _native.take_records(ptr, total).reshape(self.n_docs, int(k)), found

    def grapheme_ids(self, stream=None, engine=None):
        """fac_batch_grapheme_ids: the id in the grapheme dictionary of `engine` (default: the batch's;
        0 = not in it) of every grapheme of the non-ASCII documents, in document order, looked up on the
        device, as a NumPy uint32 array; None when the engine has no mappings."""
        import numpy as np
        eh = (engine or self.engine)._h
        n = _native.lib.fac_batch_grapheme_ids(eh, self._h, ctypes.c_void_p(stream or 0), None, 0)
        if n == -1:
            return None
        if n < 0:
            _raise(int(-n))
        out = np.zeros(max(1, int(n)), dtype=np.uint32)
        n = _native.lib.fac_batch_grapheme_ids(eh, self._h, ctypes.c_void_p(stream or 0),
                                               ctypes.c_void_p(out.ctypes.data), int(n))
        if n < 0:
            _raise(int(-n))
        return out[: int(n)]

    def doc_graphemes(self, d: int) -> Tuple[int, bool]:
        """(grapheme count, is_ascii) of document d."""
        asc = ctypes.c_int32()
        n = _native.lib.fac_batch_doc_graphemes(self._h, d, ctypes.byref(asc))
        return int(n), bool(asc.value)

    def grapheme_starts(self, d: int) -> List[int]:
        """Document-relative byte start of every grapheme of document d."""
        n, _ = self.doc_graphemes(d)
        buf = (ctypes.c_uint64 * max(1, n))()
        k = _native.lib.fac_batch_grapheme_starts(self._h, d, buf, n)
        return list(buf[:min(n, k)])

    def grapheme_starts_into(self, d: int, out):
        """grapheme_starts(d) written into the NumPy uint64 buffer `out` (no Python list): the filled
        prefix of `out`."""
        n = _native.lib.fac_batch_grapheme_starts(self._h, d, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(out))
        return out[: min(int(n), len(out))]

    def text_chars(self, d: int, out=None):
        """fac_batch_text_chars: the folded first code point of every grapheme of document d as a NumPy
        uint32 array (the filled prefix of `out` when given; empty for an ASCII document)."""
        import numpy as np
        if out is None:
            out = np.zeros(max(1, self.doc_graphemes(d)[0]), dtype=np.uint32)
        n = _native.lib.fac_batch_text_chars(self._h, d, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(out))
        return out[: min(int(n), len(out))]

    def _args(self, opts: SearchOptions, stream=None) -> "_native.fac_batch_args":
        a = _native.fac_batch_args()
        a.threshold = f32(opts.threshold_)
        a.order = opts.order_.value
        a.overlap = opts.overlap_.value
        a.unique_ids = self.engine._unique_ids()
        a.stream = stream or None
        return a

    def search_records(self, opts: SearchOptions = None, out=None, stream=None, stats=None, doc_offsets_out=None,
                       prefilter: bool = False):
        """fac_search_batch (`prefilter`: fac_search_batch_prefiltered, every document searched as
        engine.with_prefilter().search would; where the filter runs the batch must be all ASCII or
        opted in, allow_unicode_prefilter):
        (records, doc_offsets). Records (MATCH_DTYPE) are grouped by document,
        offsets relative to the record's own document, each document in FuzzyMatches::apply's order;
        doc_offsets (n_docs + 1) indexes them. `out`: a uint8 CUDA tensor to leave the records in HBM
        (32 bytes each): returns (the tensor's filled part, doc_offsets); FAC_E_OUTPUT_CAPACITY is
        raised as DeviceError with `.needed` records when it is too small. `doc_offsets_out`: an int64
        CUDA tensor of n_docs + 1 entries that also receives the index, in HBM."""
        import numpy as np
        opts = opts or SearchOptions()
        a = self._args(opts, stream)
        doc_off = np.zeros(self.n_docs + 1, dtype=np.uint64)
        n = ctypes.c_uint64()
        ptr = ctypes.POINTER(_native.fac_match)()
        if out is not None:
            a.device_out = out.data_ptr()
            a.device_cap = out.numel() // _native.REC_BYTES
        if doc_offsets_out is not None:
            if doc_offsets_out.numel() < self.n_docs + 1 or doc_offsets_out.element_size() != 8:
                raise ValueError("doc_offsets_out needs n_docs + 1 64-bit entries")
            a.device_doc_offsets = doc_offsets_out.data_ptr()
        fn = _native.lib.fac_search_batch_prefiltered if prefilter else _native.lib.fac_search_batch
        rc = fn(self.engine._h, self._h, ctypes.byref(a), None if out is not None else ctypes.byref(ptr), ctypes.byref(n),
                doc_off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(stats) if stats is not None else None)
        if rc:
            try:
                _raise(rc)
            except DeviceError as ex:
                ex.needed = int(n.value)
                raise
        if out is not None:
            return out[: n.value * _native.REC_BYTES], doc_off
        return _native.take_records(ptr, n.value), doc_off

    def count_records(self, opts: SearchOptions = None, keys=None, n_keys=None, out=None, stream=None, stats=None,
                      doc_offsets_out=None, totals=False, prefilter: bool = False):
        """fac_count_batch (`prefilter`: fac_count_batch_prefiltered): (terms, doc_offsets, totals), the
        per-document term counts of `search_records(opts)` grouped on the device. Terms (TERM_DTYPE:
        key, count, best_similarity, best_pattern) are grouped by document, ascending key inside a
        document; doc_offsets (n_docs + 1) indexes them. `keys`: one key per pattern, folding surface
        forms into entities (None: key = pattern index); `n_keys`: the size of the key space (None:
        the greatest key + 1; without `keys` it is the pattern count, and None, 0 and that count all
        mean it -- the totals always have that many rows). `out`: a uint8 CUDA tensor to leave the terms in
        HBM (16 bytes each): returns its filled part; too small raises DeviceError
        (FAC_E_OUTPUT_CAPACITY) with `.needed` terms, nothing written. `doc_offsets_out`: an int64
        CUDA tensor of n_docs + 1 entries that also receives the index. `totals`: False (None is
        returned), True (an (n_keys, 2) uint64 array of (count, documents) per key), or an int64 CUDA
        tensor of at least n_keys * 2 entries that receives them in HBM and is returned."""
        import numpy as np
        opts = opts or SearchOptions()
        karr, nk = _key_table(self.engine, keys, n_keys)
        a = _native.fac_count_args()
        a.threshold = f32(opts.threshold_)
        a.order = opts.order_.value
        a.overlap = opts.overlap_.value
        a.unique_ids = self.engine._unique_ids()
        a.keys = karr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if karr is not None else None
        a.n_keys = nk
        a.stream = stream or None
        doc_off = np.zeros(self.n_docs + 1, dtype=np.uint64)
        n = ctypes.c_uint64()
        ptr = ctypes.POINTER(_native.fac_term)()
        if out is not None:
            a.device_out = out.data_ptr()
            a.device_cap = out.numel() // _native.TERM_BYTES
        if doc_offsets_out is not None:
            if doc_offsets_out.numel() < self.n_docs + 1 or doc_offsets_out.element_size() != 8:
                raise ValueError("doc_offsets_out needs n_docs + 1 64-bit entries")
            a.device_doc_offsets = doc_offsets_out.data_ptr()
        h_tot = None
        if totals is True:
            h_tot = np.zeros((max(nk, 1), 2), dtype=np.uint64)
        elif totals is not False and totals is not None:
            if totals.numel() < 2 * nk or totals.element_size() != 8:
                raise ValueError("totals needs n_keys * 2 64-bit entries")
            a.device_totals = totals.data_ptr()
        fn = _native.lib.fac_count_batch_prefiltered if prefilter else _native.lib.fac_count_batch
        rc = fn(self.engine._h, self._h, ctypes.byref(a), None if out is not None else ctypes.byref(ptr), ctypes.byref(n),
                doc_off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                ctypes.c_void_p(h_tot.ctypes.data) if h_tot is not None else None,
                ctypes.byref(stats) if stats is not None else None)
        if rc:
            try:
                _raise(rc)
            except DeviceError as ex:
                ex.needed = int(n.value)
                raise
        tot = h_tot[:nk] if h_tot is not None else (totals if a.device_totals else None)
        if out is not None:
            return out[: n.value * _native.TERM_BYTES], doc_off, tot
        return _native.take_terms(ptr, n.value), doc_off, tot

    def term_matrix(self, opts: SearchOptions = None, keys=None, n_keys=None, values: str = "count",
                    prefilter: bool = False):
        """The document-term matrix of the batch as a torch.sparse_csr_tensor of shape (n_docs, n_keys)
        on the engine's device: row d holds document d's terms (count_records), as float32 counts
        (`values="count"`) or each term's best similarity (`values="similarity"`). The terms and their
        index stay in HBM; the tensor is built from them with torch ops only. The term buffer starts at
        max(1024, 2 * n_docs) terms; a batch with more terms runs the whole call (search, apply and
        count) a second time with a buffer of the size the first run reported."""
        import torch
        if values not in ("count", "similarity"):
            raise ValueError('values must be "count" or "similarity"')
        _, nk = _key_table(self.engine, keys, n_keys)
        dev = torch.device("cuda", self.engine.device)
        crow = torch.empty(self.n_docs + 1, dtype=torch.int64, device=dev)
        cap = max(1024, 2 * self.n_docs)
        while True:
            buf = torch.empty(cap * _native.TERM_BYTES, dtype=torch.uint8, device=dev)
            try:
                filled, _, _ = self.count_records(opts, keys, nk, out=buf, doc_offsets_out=crow, prefilter=prefilter)
                break
            except DeviceError as ex:
                if ex.code != _native.FAC_E_OUTPUT_CAPACITY:
                    raise
                cap = ex.needed
        words = filled.view(torch.int32).view(filled.numel() // _native.TERM_BYTES, 4)
        col = words[:, 0].to(torch.int64) & 0xFFFFFFFF
        if values == "count":
            val = (words[:, 1].to(torch.int64) & 0xFFFFFFFF).to(torch.float32)
        else:
            val = words[:, 2].contiguous().view(torch.float32)
        return torch.sparse_csr_tensor(crow, col, val, size=(self.n_docs, nk), device=dev)

    def segment_records(self, opts: SearchOptions = None, out=None, stream=None, stats=None, doc_offsets_out=None,
                        prefilter: bool = False):
        """fac_segment_batch (`prefilter`: fac_segment_batch_prefiltered): (segments, doc_offsets), the
        crate's engine.segment_iter(doc_d, opts) of every document (options normalised as
        `segmented`, query.rs:46-64). Segments (MATCH_DTYPE) are grouped by document, offsets relative
        to the segment's own document, and tile it; a matched segment is the kept record, an unmatched
        one has pattern_index == _native.FAC_UNMATCHED. `out`, `doc_offsets_out` and the DeviceError
        with `.needed` segments are search_records'."""
        import numpy as np
        opts = opts or SearchOptions()
        a = self._args(opts, stream)
        doc_off = np.zeros(self.n_docs + 1, dtype=np.uint64)
        n = ctypes.c_uint64()
        ptr = ctypes.POINTER(_native.fac_match)()
        if out is not None:
            a.device_out = out.data_ptr()
            a.device_cap = out.numel() // _native.REC_BYTES
        if doc_offsets_out is not None:
            if doc_offsets_out.numel() < self.n_docs + 1 or doc_offsets_out.element_size() != 8:
                raise ValueError("doc_offsets_out needs n_docs + 1 64-bit entries")
            a.device_doc_offsets = doc_offsets_out.data_ptr()
        fn = _native.lib.fac_segment_batch_prefiltered if prefilter else _native.lib.fac_segment_batch
        rc = fn(self.engine._h, self._h, ctypes.byref(a), None if out is not None else ctypes.byref(ptr), ctypes.byref(n),
                doc_off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(stats) if stats is not None else None)
        if rc:
            try:
                _raise(rc)
            except DeviceError as ex:
                ex.needed = int(n.value)
                raise
        if out is not None:
            return out[: n.value * _native.REC_BYTES], doc_off
        return _native.take_records(ptr, n.value), doc_off

    def render_bytes(self, mode: int, opts: SearchOptions = None, out=None, offsets_out=None, stream=None, stats=None,
                     prefilter: bool = False):
        """fac_render_batch (`prefilter`: fac_render_batch_prefiltered): (bytes, offsets). Output
        document d is bytes[offsets[d]:offsets[d + 1]], the crate's engine.strip_prefix / strip_suffix /
        segment_text(doc_d, opts) for mode _native.FAC_RENDER_STRIP_PREFIX / _STRIP_SUFFIX /
        _SEGMENT_TEXT. `out`, `offsets_out` and the DeviceError with `.needed` bytes are replace_bytes'."""
        import numpy as np
        opts = opts or SearchOptions()
        a = _native.fac_replace_args()
        a.threshold = f32(opts.threshold_)
        a.order = opts.order_.value
        a.overlap = opts.overlap_.value
        a.unique_ids = self.engine._unique_ids()
        a.stream = stream or None
        offsets = np.zeros(self.n_docs + 1, dtype=np.uint64)
        n = ctypes.c_uint64()
        ptr = ctypes.POINTER(ctypes.c_uint8)()
        if out is not None:
            a.device_out = out.data_ptr()
            a.device_cap = out.numel() * out.element_size()
        if offsets_out is not None:
            if offsets_out.numel() < self.n_docs + 1 or offsets_out.element_size() != 8:
                raise ValueError("offsets_out needs n_docs + 1 64-bit entries")
            a.device_out_offsets = offsets_out.data_ptr()
        fn = _native.lib.fac_render_batch_prefiltered if prefilter else _native.lib.fac_render_batch
        rc = fn(self.engine._h, self._h, int(mode), ctypes.byref(a), None if out is not None else ctypes.byref(ptr),
                ctypes.byref(n), offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                ctypes.byref(stats) if stats is not None else None)
        if rc:
            try:
                _raise(rc)
            except DeviceError as ex:
                ex.needed = int(n.value)
                raise
        if out is not None:
            return out[: n.value], offsets
        try:
            return ctypes.string_at(ptr, n.value), offsets
        finally:
            _native.lib.fac_buffer_free(ptr)

    def prefilter_windows(self, threshold: float, stream=None):
        """Diagnostics (fac_batch_prefilter_windows): the merged bitap windows of every document as
        (document, start, end) triples, document-relative, ascending -- bytes for an ASCII document,
        graphemes for any other (an opted-in batch); None where the reference falls back to the full
        search."""
        cap = 1024
        while True:
            buf = (ctypes.c_uint64 * (3 * cap))()
            n = _native.lib.fac_batch_prefilter_windows(self.engine._h, self._h, f32(threshold),
                                                        ctypes.c_void_p(stream or 0), buf, cap)
            if n == -1:
                return None
            if n < 0:
                _raise(-n)
            if n <= cap:
                return [(int(buf[3 * i]), int(buf[3 * i + 1]), int(buf[3 * i + 2])) for i in range(n)]
            cap = n

    def replace_bytes(self, table: "ReplacementTable", opts: SearchOptions = None, out=None, offsets_out=None,
                      stream=None, stats=None, prefilter: bool = False):
        """fac_replace_batch (`prefilter`: fac_replace_batch_prefiltered): (bytes, offsets). Output document d is bytes[offsets[d]:offsets[d + 1]],
        the crate's engine.replace(doc_d, opts, callback) with callback = the table's entry of the
        match's pattern (options normalised as `segmented`, query.rs:46-64). `out`: a uint8 CUDA
        tensor to leave the bytes in HBM: returns (the tensor's filled part, offsets);
        FAC_E_OUTPUT_CAPACITY is raised as DeviceError with `.needed` bytes when it is too small
        (nothing is written then). `offsets_out`: an int64 CUDA tensor of n_docs + 1 entries that also
        receives the offsets, in HBM. `self.replaced` holds the number of records applied."""
        import numpy as np
        opts = opts or SearchOptions()
        a = _native.fac_replace_args()
        a.threshold = f32(opts.threshold_)
        a.order = opts.order_.value
        a.overlap = opts.overlap_.value
        a.unique_ids = self.engine._unique_ids()
        a.stream = stream or None
        offsets = np.zeros(self.n_docs + 1, dtype=np.uint64)
        n = ctypes.c_uint64()
        nrep = ctypes.c_uint64()
        ptr = ctypes.POINTER(ctypes.c_uint8)()
        if out is not None:
            a.device_out = out.data_ptr()
            a.device_cap = out.numel() * out.element_size()
        if offsets_out is not None:
            if offsets_out.numel() < self.n_docs + 1 or offsets_out.element_size() != 8:
                raise ValueError("offsets_out needs n_docs + 1 64-bit entries")
            a.device_out_offsets = offsets_out.data_ptr()
        fn = _native.lib.fac_replace_batch_prefiltered if prefilter else _native.lib.fac_replace_batch
        rc = fn(self.engine._h, self._h, table._h, ctypes.byref(a), None if out is not None else ctypes.byref(ptr),
                ctypes.byref(n), offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(nrep),
                ctypes.byref(stats) if stats is not None else None)
        if rc:
            try:
                _raise(rc)
            except DeviceError as ex:
                ex.needed = int(n.value)
                raise
        self.replaced = int(nrep.value)
        if out is not None:
            return out[: n.value], offsets
        try:
            return ctypes.string_at(ptr, n.value), offsets
        finally:
            _native.lib.fac_buffer_free(ptr)

    def extract(self, table: "ReplacementTable" = None, opts: SearchOptions = None, records_out=None, text_out=None,
                doc_offsets_out=None, item_offsets_out=None, stream=None, stats=None, prefilter: bool = False):
        """fac_extract_batch (`prefilter`: fac_extract_batch_prefiltered): (records, doc_offsets, text,
        item_offsets). The records are search_records' for the same options; item i, the string of
        record i, is text[item_offsets[i]:item_offsets[i + 1]]: the matched text
        (FuzzyMatches::matched_strings) or, with `table`, what replace would put in its place.
        Document d owns [doc_offsets[d], doc_offsets[d + 1]) of records and items. `records_out` and
        `text_out` (uint8 CUDA tensors, given together) leave records and text in HBM and are returned
        cut to their filled parts; FAC_E_OUTPUT_CAPACITY is raised as DeviceError with `.needed`
        records and `.needed_text` bytes when either is too small (nothing is written then).
        `doc_offsets_out` / `item_offsets_out`: int64 CUDA tensors that receive the two indexes in HBM
        (n_docs + 1 entries; one more than the records `records_out` holds); item_offsets is then
        the filled part of `item_offsets_out` and no copy of it visits the host."""
        import numpy as np
        opts = opts or SearchOptions()
        if (records_out is None) != (text_out is None):
            raise ValueError("records_out and text_out are given together or not at all")
        a = _native.fac_extract_args()
        a.threshold = f32(opts.threshold_)
        a.order = opts.order_.value
        a.overlap = opts.overlap_.value
        a.unique_ids = self.engine._unique_ids()
        a.stream = stream or None
        doc_off = np.zeros(self.n_docs + 1, dtype=np.uint64)
        n, nbytes = ctypes.c_uint64(), ctypes.c_uint64()
        recs = ctypes.POINTER(_native.fac_match)()
        text = ctypes.POINTER(ctypes.c_uint8)()
        ioff = ctypes.POINTER(ctypes.c_uint64)()
        if records_out is not None:
            a.device_records = records_out.data_ptr()
            a.device_record_cap = records_out.numel() // _native.REC_BYTES
            a.device_text = text_out.data_ptr()
            a.device_text_cap = text_out.numel() * text_out.element_size()
        if doc_offsets_out is not None:
            if doc_offsets_out.numel() < self.n_docs + 1 or doc_offsets_out.element_size() != 8:
                raise ValueError("doc_offsets_out needs n_docs + 1 64-bit entries")
            a.device_doc_offsets = doc_offsets_out.data_ptr()
        if item_offsets_out is not None:
            if records_out is None or item_offsets_out.numel() < 1 or item_offsets_out.element_size() != 8:
                raise ValueError("item_offsets_out needs records_out and 64-bit entries, one more than its records")
            a.device_item_offsets = item_offsets_out.data_ptr()
            a.device_record_cap = min(a.device_record_cap, item_offsets_out.numel() - 1)
        fn = _native.lib.fac_extract_batch_prefiltered if prefilter else _native.lib.fac_extract_batch
        dev = records_out is not None
        rc = fn(self.engine._h, self._h, table._h if table is not None else None, ctypes.byref(a),
                None if dev else ctypes.byref(recs), ctypes.byref(n),
                doc_off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), None if dev else ctypes.byref(text),
                ctypes.byref(nbytes), None if item_offsets_out is not None else ctypes.byref(ioff),
                ctypes.byref(stats) if stats is not None else None)
        if rc:
            try:
                _raise(rc)
            except DeviceError as ex:
                ex.needed, ex.needed_text = int(n.value), int(nbytes.value)
                raise
        if item_offsets_out is not None:
            item_off = item_offsets_out[: n.value + 1]
        else:
            try:
                item_off = np.ctypeslib.as_array(ioff, shape=(n.value + 1,)).copy()
            finally:
                _native.lib.fac_buffer_free(ioff)
        if dev:
            return records_out[: n.value * _native.REC_BYTES], doc_off, text_out[: nbytes.value], item_off
        try:
            return _native.take_records(recs, n.value), doc_off, ctypes.string_at(text, nbytes.value), item_off
        finally:
            _native.lib.fac_buffer_free(text)


def replacement_table(replacements) -> Tuple[bytes, List[int], bytes]:
    """(utf8, offsets, keep) of one replacement per pattern, the layout fac_replacements_create
    takes: replacement p is utf8[offsets[p]:offsets[p + 1]]; `None` (keep the matched text) has
    keep[p] == 1 and no bytes. `str` entries are encoded as UTF-8, `bytes` taken as they are (the
    library validates them). Pure Python."""
    parts, offsets, keep = [], [0], bytearray()
    for r in replacements:
        if r is None:
            raw = b""
        elif isinstance(r, str):
            raw = r.encode("utf-8")
        elif isinstance(r, (bytes, bytearray, memoryview)):
            raw = bytes(r)
        else:
            raise TypeError(f"a replacement must be str, bytes or None, got {type(r).__name__}")
        keep.append(1 if r is None else 0)
        parts.append(raw)
        offsets.append(offsets[-1] + len(raw))
    return b"".join(parts), offsets, bytes(keep)


class Wrap(NamedTuple):
    """A template replacement: the match becomes prefix + m.text + suffix, the callback
    `|m| Some(format!("{prefix}{}{suffix}", m.text))` (matches.rs:445-446) -- highlighting, tagging,
    bracketing. `str` or `bytes` halves, each valid UTF-8 on its own."""
    prefix: Union[str, bytes]
    suffix: Union[str, bytes] = ""

    def render(self, text: str) -> str:
        return _as_text(self.prefix) + text + _as_text(self.suffix)


def template_table(replacements) -> Tuple[bytes, List[int], bytes, List[int]]:
    """(utf8, offsets, keep, insert_at), the layout fac_replacements_create_templates takes:
    replacement_table's first three, a `Wrap` entry holding prefix + suffix as its bytes, and
    insert_at[p] = len(prefix) in bytes for a `Wrap`, _native.FAC_NO_INSERT otherwise. Pure Python."""
    flat, insert_at = [], []
    for r in replacements:
        if isinstance(r, Wrap):
            data, off, _ = replacement_table([r.prefix, r.suffix])
            flat.append(data)
            insert_at.append(off[1])
        else:
            flat.append(r)
            insert_at.append(_native.FAC_NO_INSERT)
    return replacement_table(flat) + (insert_at,)


def _rendered_entry(r, m) -> Optional[str]:
    """What the callback of a table entry returns for the match m (None: keep the matched text)."""
    return r.render(m.text) if isinstance(r, Wrap) else _as_text(r)


class ReplacementTable:
    """One replacement per pattern of `engine` (None = keep, `Wrap` = a template around the matched
    text), validated and uploaded once (fac_replacements_create, or
    fac_replacements_create_templates when a `Wrap` is present); freed with the object."""

    def __init__(self, engine: FuzzyAhoCorasick, replacements):
        self.replacements = list(replacements)
        data, offsets, keep, insert_at = template_table(self.replacements)
        self.engine, self.n_patterns = engine, len(keep)
        off = (ctypes.c_uint64 * len(offsets))(*offsets)
        h = ctypes.c_void_p()
        if any(isinstance(r, Wrap) for r in self.replacements):
            ins = (ctypes.c_uint64 * len(insert_at))(*insert_at)
            rc = _native.lib.fac_replacements_create_templates(engine._h, data, off, keep, ins, len(keep), ctypes.byref(h))
        else:
            rc = _native.lib.fac_replacements_create(engine._h, data, off, keep, len(keep), ctypes.byref(h))
        if rc:
            _raise(rc)
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _native.lib is not None:
            _native.lib.fac_replacements_free(h)
            self._h = None


class FuzzyReplacer:
    """replacer.rs:9-52; a replacement may be a `Wrap` (prefix + m.text + suffix)."""

    def __init__(self, engine: FuzzyAhoCorasick, replacements: List[str]):
        self.engine = engine
        self.replacements = replacements

    def _callback(self, m):
        return _rendered_entry(self.replacements[m.pattern_index], m)

    def replace(self, text: str, opts: SearchOptions) -> str:
        return self.engine.replace(text, opts, self._callback)

    def extract_batch(self, texts: Sequence[str], opts: SearchOptions,
                      boundaries: Boundary = Boundary.NONE, anchors: Anchor = Anchor.NONE) -> List[List[str]]:
        """Per text, the replacement of every match `engine.search(t, opts)` finds, as one device pass
        (fac_extract_batch): the canonical form of each mention."""
        return self.engine.extract_batch(texts, opts, self._device_table(), boundaries=boundaries, anchors=anchors)

    def lookup_batch(self, texts: Sequence[str], opts: SearchOptions = None) -> List[Optional[str]]:
        """Per text the canonical form (the replacement) of the best entry that matches the text as a
        whole, or None where no entry does: a column normalised against the dictionary in one device
        pass (engine.lookup_batch with k = 1). A `None` entry stands for the text itself."""
        return [_item_text(self.replacements, ms[0]) if ms else None
                for ms in self.engine.lookup_batch(texts, opts, 1)]

    @staticmethod
    def term_keys(replacements, patterns=None) -> Tuple[List[int], List[str]]:
        """(keys, forms): keys[p] is the index of pattern p's replacement among the distinct
        replacements, in order of first appearance, and forms[k] the canonical form of key k. A `None`
        entry (the matched text stays) stands for its own pattern's text, a `Wrap` for that text
        wrapped; `patterns` (the engine's) is only needed for those."""
        keys, forms, seen = [], [], {}
        for p, r in enumerate(replacements):
            if r is None or isinstance(r, Wrap):
                if patterns is None:
                    raise ValueError("a None or Wrap replacement needs the patterns")
                r = patterns[p].pattern if r is None else r.render(patterns[p].pattern)
            form = _as_text(r)
            if form not in seen:
                seen[form] = len(forms)
                forms.append(form)
            keys.append(seen[form])
        return keys, forms

    def count_batch(self, texts: Sequence[str], opts: SearchOptions = None, unicode_mappings: bool = False,
                    boundaries: Boundary = Boundary.NONE, anchors: Anchor = Anchor.NONE) -> List[Dict[str, int]]:
        """Per text, how often each canonical form (replacement) is mentioned: the matches
        `engine.search(t, opts)` finds, counted per distinct replacement on the device
        (engine.count_batch with `term_keys`)."""
        keys, forms = self.term_keys(self.replacements, self.engine.patterns_)
        return [{forms[k]: t.count for k, t in terms.items()}
                for terms in self.engine.count_batch(texts, opts, keys, len(forms), unicode_mappings=unicode_mappings,
                                                     boundaries=boundaries, anchors=anchors)]

    def _device_table(self) -> "ReplacementTable":
        key = tuple(self.replacements)
        if getattr(self, "_table", None) is None or self._table[0] != key:
            self._table = (key, ReplacementTable(self.engine, self.replacements))
        return self._table[1]

    def replace_batch(self, texts: Sequence[str], opts: SearchOptions, boundaries: Boundary = Boundary.NONE,
                      anchors: Anchor = Anchor.NONE) -> List[str]:
        """`[self.replace(t, opts) for t in texts]` as one device pass (fac_replace_batch)."""
        return self.engine.replace_batch(texts, opts, self._device_table(), boundaries=boundaries, anchors=anchors)

    def replace_stream(self, reader, writer, threshold: float, prefilter: bool = False,
                       boundaries: Boundary = Boundary.NONE) -> int:
        """replacer.rs:35-44, spliced on the device (fac_replace_stream_*); `prefilter`: every window
        is searched through the bitap pre-filter (Prefiltered::search); `boundaries`: as
        engine.search_stream's."""
        return self.engine.replace_stream(reader, writer, threshold, self._device_table(), _prefilter=prefilter,
                                          boundaries=boundaries)
