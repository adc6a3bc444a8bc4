#!/usr/bin/env python3
"""Batch search against the per-document loop.

The texts of workloads.config("c2") and config("c3") are cut into documents at the space nearest
every L bytes and searched three ways in one process, on device-resident bytes, after a warm-up:

  (a) one fac_search_batch call over every document (records left in HBM, Unsorted + Keep),
      timed with device events on the call's stream; run once per prefix-cache rule
      (FAC_BATCH_RC_SEG: windows per segment the cache asks for; 0 = no such condition),
  (b) the per-document loop fac_search_raw(doc) over a fixed sample of documents, host wall clock
      (every call ends synchronised); repeated to get its spread; legs (a) and (b) alternate,
  (c) the same bytes as ONE haystack through fac_search_staged: the boundary-free ceiling, a
      different result set, shown for scale only.

With --replace the legs are instead (DESIGN.md §6a "Batched replace"; the table maps every
pattern to its upper-cased form):

  (r)  one fac_replace_batch call, bytes and offsets left in HBM, device events,
  (a') fac_search_batch with the same normalised options (Default + NonOverlapping) on the same
       batch: (r) - (a') is what the splice costs,
  (b') the per-document loop replacer.replace(doc, opts) over the fixed sample, host wall clock,
  and a hipMemcpyDtoDAsync of the output's size, the copy kernel's yardstick.

With --prefilter the legs are (DESIGN.md §6a "Pre-filtered batches"; workloads c2, c5 and "c5n" =
c5's engine on fresh filler words with no planted match):

  (p)  one fac_search_batch_prefiltered call, records left in HBM, device events; once per
       prefix-cache rule like (a),
  (a)  fac_search_batch on the same batch (the path without the filter),
  (c)  fac_search_staged_prefiltered of the same bytes as ONE haystack: the boundary-free ceiling
       (a different result set; its records go to the host),
  (b)  the per-document loop fac_search_prefiltered(doc) over the fixed sample, host wall clock.

  The legs alternate; "records_equal" compares (p)'s records of the sample with (b)'s.

With --prefilter-unicode the same legs run on batches that hold non-ASCII documents, opted in with
fac_batch_allow_unicode_prefilter (DESIGN.md §6a "Pre-filtered batches of non-ASCII documents"):
"u3" = c5's shape over the C3 script mix (1 000 patterns of 10-16 characters, edits 1, threshold
0.85, case-insensitive, one planted hit per MiB), "u3a" = the same text with every fourth document
replaced by ASCII filler of its length. (a), the plain batch, is the only one-call path such a batch
had before; (b) is what the Python conveniences did.

With --segment the legs are (DESIGN.md §6a "Batched segmentation"):

  (s)  one fac_render_batch call per mode (strip_prefix, strip_suffix, segment_text) and one
       fac_segment_batch call, output and offsets left in HBM, device events,
  (a') fac_search_batch with the same normalised options on the same batch: the cost floor,
  (r)  fac_replace_batch with an all-keep table: the same bytes moved by the splice,
  (b') the per-document loops engine.strip_prefix(doc, opts), strip_suffix, segment_text and
       list(engine.segment_iter(doc, opts)) over the fixed sample, host wall clock.

With --template the legs are (DESIGN.md §6a "Template replacements and extraction"):

  (r)  fac_replace_batch with the plain upper-case table of --replace,
  (t)  the same batch with every entry Wrap("<b>", "</b>"): (t) - (r) is what the three-run pieces
       and the longer output cost, beside a hipMemcpyDtoDAsync of (t)'s output size.

With --extract:

  (x)  fac_extract_batch with a NULL table (matched_strings), records, text and both indexes left
       in HBM,
  (a)  fac_search_batch with the same options and device_out: (x) - (a) is the extraction.

Staging is reported in ms per GiB: the batch stager against fac_haystack_stage_device on the same
bytes. One JSON line per configuration; "gate" is true when (a) beats (b) per document by more than
(b)'s own spread and (a)'s records for the sample equal (b)'s.
"""
import argparse
import ctypes
import json
import os
import sys
import time

os.environ["FAC_DIAGNOSTICS"] = "1"  # the cache-rule knob is a diagnostics knob
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "fuzzy-aho-corasick-rs_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fuzzy_aho_corasick import (FuzzyReplacer, Order, Overlap, ReplacementTable, SearchOptions, StagedBatch,  # noqa: E402
                                StagedHaystack, _native, workloads)
from fuzzy_aho_corasick.structs import f32  # noqa: E402


def cut_documents(data: bytes, L: int) -> np.ndarray:
    """Offsets of the documents: a cut after the space nearest every L bytes."""
    b = np.frombuffer(data, np.uint8)
    sp = np.flatnonzero(b == 0x20)
    tg = np.arange(L, len(data), L)
    i = np.clip(np.searchsorted(sp, tg), 1, len(sp) - 1)
    near = np.where(tg - sp[i - 1] <= sp[i] - tg, sp[i - 1], sp[i]) + 1
    return np.unique(np.concatenate([[0], near, [len(data)]])).astype(np.uint64)


def raw_records(engine, doc: bytes, thr: float):
    out = ctypes.POINTER(_native.fac_match)()
    n = ctypes.c_uint64()
    eg = ctypes.c_uint64()
    rc = _native.lib.fac_search_raw(engine._h, doc, len(doc), f32(thr), ctypes.byref(out), ctypes.byref(n), ctypes.byref(eg))
    if rc:
        raise RuntimeError(_native.last_error())
    return _native.take_records(out, n.value)


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    r = fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b), r


_CACHE = {}


def workload(name, nbytes):
    if (name, nbytes) not in _CACHE:
        w = workloads.config(name, nbytes)
        _CACHE[(name, nbytes)] = (w, workloads.builder_for(w).build(w.patterns))
    return _CACHE[(name, nbytes)]


def run(name, nbytes, L, sample, rounds, rules, profile_only):
    w, engine = workload(name, nbytes)
    data = w.haystack
    off = cut_documents(data, L)
    nd = len(off) - 1
    dev = torch.device("cuda", engine.device)
    t_data = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
    t_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    opts = SearchOptions().threshold(w.threshold)
    out = torch.empty(max(1 << 16, len(data) // 16) * 32, dtype=torch.uint8, device=dev)

    def stage_batch(reuse=None):
        return StagedBatch.from_device(engine, t_data.data_ptr(), t_off.data_ptr(), nd, len(data), stream=sh, reuse=reuse)

    def batch_search(sb):
        nonlocal out
        while True:
            try:
                return sb.search_records(opts, out=out, stream=sh)
            except Exception as ex:  # FAC_E_OUTPUT_CAPACITY: grow and search again
                need = getattr(ex, "needed", 0)
                if not need:
                    raise
                out = torch.empty(int(need * 1.1 + 1024) * 32, dtype=torch.uint8, device=dev)

    if profile_only == "c":  # the one-haystack leg alone
        hay = StagedHaystack.from_device(engine, t_data.data_ptr(), len(data), stream=sh)
        for _ in range(4):
            hay = StagedHaystack.from_device(engine, t_data.data_ptr(), len(data), stream=sh, reuse=hay)
            hay.search_device(w.threshold, stream=sh)
        return None
    sb = stage_batch()
    for rule in rules:  # warm-up: buffers, tables, the output size
        os.environ["FAC_BATCH_RC_SEG"] = str(rule)
        batch_search(sb)
    if profile_only:
        os.environ.pop("FAC_BATCH_RC_SEG")
        for _ in range(3):
            sb = stage_batch(sb)
            batch_search(sb)
        return None
    idx = np.unique(np.linspace(0, nd - 1, min(sample, nd)).astype(np.int64))
    docs = [data[int(off[d]):int(off[d + 1])] for d in idx]
    for d in docs[:50]:
        raw_records(engine, d, w.threshold)
    a_ms = {r: [] for r in rules}
    b_ms = []
    for _ in range(rounds):
        for rule in rules:
            os.environ["FAC_BATCH_RC_SEG"] = str(rule)
            ms, (recs, doc_off) = timed(stream, lambda: batch_search(sb))
            a_ms[rule].append(ms)
        t0 = time.perf_counter()
        per_doc = [raw_records(engine, d, w.threshold) for d in docs]
        b_ms.append(1e3 * (time.perf_counter() - t0))
    os.environ.pop("FAC_BATCH_RC_SEG")
    # (a)'s records of the sample against (b)'s
    host = np.frombuffer(recs.cpu().numpy().tobytes(), dtype=_native.MATCH_DTYPE)
    key = lambda r: sorted(zip(r["start"].tolist(), r["end"].tolist(), r["pattern_index"].tolist(),  # noqa: E731
                               r["similarity"].view(np.uint32).tolist(), r["edits"].tolist()))
    same = all(key(host[int(doc_off[d]):int(doc_off[d + 1])]) == key(p) for d, p in zip(idx, per_doc))
    # staging, and the one-haystack ceiling
    st_b = [timed(stream, lambda: stage_batch(sb))[0] for _ in range(rounds)]
    hay = StagedHaystack.from_device(engine, t_data.data_ptr(), len(data), stream=sh)
    st_h = [timed(stream, lambda: StagedHaystack.from_device(engine, t_data.data_ptr(), len(data), stream=sh, reuse=hay))[0]
            for _ in range(rounds)]
    hay.search_device(w.threshold, stream=sh)
    c_ms = [timed(stream, lambda: hay.search_device(w.threshold, stream=sh))[0] for _ in range(rounds)]
    gib = len(data) / float(1 << 30)
    b_doc = [m / len(docs) for m in b_ms]
    res = {"config": name, "bytes": len(data), "L": L, "docs": nd, "sample": len(docs), "records": int(len(host)),
           "a_ms": {str(r): [round(x, 3) for x in v] for r, v in a_ms.items()},
           "b_sample_ms": [round(x, 2) for x in b_ms], "c_ms": [round(x, 3) for x in c_ms],
           "stage_batch_ms_per_gib": round(min(st_b) / gib, 2), "stage_haystack_ms_per_gib": round(min(st_h) / gib, 2),
           "records_equal": bool(same)}
    best_rule = min(rules, key=lambda r: float(np.median(a_ms[r])))
    a_doc = float(np.median(a_ms[best_rule])) / nd
    res.update({"best_rule": best_rule, "a_us_per_doc": round(1e3 * a_doc, 4),
                "b_us_per_doc": [round(1e3 * x, 2) for x in b_doc], "b_spread_us": round(1e3 * (max(b_doc) - min(b_doc)), 2),
                "a_over_b": round(a_doc / float(np.median(b_doc)), 6),
                "a_over_c": round(float(np.median(a_ms[best_rule])) / float(np.median(c_ms)), 3),
                "gate": bool(same and min(b_doc) - a_doc > max(b_doc) - min(b_doc))})
    return res


def run_replace(name, nbytes, L, sample, rounds, profile_only):
    w, engine = workload(name, nbytes)
    data = w.haystack
    off = cut_documents(data, L)
    nd = len(off) - 1
    dev = torch.device("cuda", engine.device)
    t_data = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
    t_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    opts = SearchOptions().threshold(w.threshold)  # normalised by the replace: Default + NonOverlapping
    opts.order_, opts.overlap_ = Order.Default, Overlap.NonOverlapping
    reps = [(p if isinstance(p, str) else p.pattern).upper() for p in w.patterns]
    table = ReplacementTable(engine, reps)
    replacer = FuzzyReplacer(engine, reps)
    bufs = {"rec": torch.empty(max(1 << 16, len(data) // 16) * 32, dtype=torch.uint8, device=dev),
            "out": torch.empty(len(data) + (1 << 20), dtype=torch.uint8, device=dev)}
    t_out_off = torch.empty(nd + 1, dtype=torch.int64, device=dev)
    sb = StagedBatch.from_device(engine, t_data.data_ptr(), t_off.data_ptr(), nd, len(data), stream=sh)

    def grown(key, unit, call):
        while True:
            try:
                return call(bufs[key])
            except Exception as ex:  # FAC_E_OUTPUT_CAPACITY: grow and run again
                need = getattr(ex, "needed", 0)
                if not need:
                    raise
                bufs[key] = torch.empty(int(need * 1.1 + 1024) * unit, dtype=torch.uint8, device=dev)

    def replace():
        return grown("out", 1, lambda o: sb.replace_bytes(table, opts, out=o, offsets_out=t_out_off, stream=sh))

    def search():
        return grown("rec", 32, lambda o: sb.search_records(opts, out=o, stream=sh))

    for _ in range(2):  # warm-up: buffers, tables, the output sizes
        replace()
        search()
    if profile_only:
        for _ in range(3):
            replace()
        return None
    idx = np.unique(np.linspace(0, nd - 1, min(sample, nd)).astype(np.int64))
    docs = [data[int(off[d]):int(off[d + 1])].decode("utf-8") for d in idx]
    for d in docs[:50]:
        replacer.replace(d, opts)
    r_ms, a_ms, b_ms = [], [], []
    for _ in range(rounds):
        ms, (out, out_off) = timed(stream, replace)
        r_ms.append(ms)
        a_ms.append(timed(stream, search)[0])
        t0 = time.perf_counter()
        per_doc = [replacer.replace(d, opts) for d in docs]
        b_ms.append(1e3 * (time.perf_counter() - t0))
    host = out.cpu().numpy().tobytes()
    same = all(host[int(out_off[d]):int(out_off[d + 1])] == p.encode("utf-8") for d, p in zip(idx, per_doc))
    # the yardstick: a device-to-device copy of the output's size
    copy_ms = None
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        dst = torch.empty(len(host), dtype=torch.uint8, device=dev)
        hip.hipMemcpyDtoDAsync.restype = ctypes.c_int
        rcs = []
        cp = lambda: rcs.append(hip.hipMemcpyDtoDAsync(dst.data_ptr(), out.data_ptr(), len(host), sh))  # noqa: E731
        cp()
        copy_ms = [round(timed(stream, cp)[0], 4) for _ in range(rounds)]
        if any(rcs) or not torch.equal(dst, out[:len(host)]):  # the copy did not run on this stream: no yardstick
            copy_ms = None
    except (OSError, AttributeError):
        pass
    b_doc = [m / len(docs) for m in b_ms]
    r_doc = float(np.median(r_ms)) / nd
    return {"leg": "replace", "config": name, "bytes": len(data), "L": L, "docs": nd, "sample": len(docs),
            "out_bytes": len(host), "replaced": int(sb.replaced),
            "r_ms": [round(x, 3) for x in r_ms], "a_ms": [round(x, 3) for x in a_ms],
            "splice_ms": round(float(np.median(r_ms)) - float(np.median(a_ms)), 3),
            "b_sample_ms": [round(x, 2) for x in b_ms], "dtod_copy_ms": copy_ms,
            "r_us_per_doc": round(1e3 * r_doc, 4), "b_us_per_doc": [round(1e3 * x, 2) for x in b_doc],
            "b_spread_us": round(1e3 * (max(b_doc) - min(b_doc)), 2), "r_over_b": round(r_doc / float(np.median(b_doc)), 6),
            "bytes_equal": bool(same), "gate": bool(same and min(b_doc) - r_doc > max(b_doc) - min(b_doc))}


def run_segment(name, nbytes, L, sample, rounds):
    w, engine = workload(name, nbytes)
    data = w.haystack
    off = cut_documents(data, L)
    nd = len(off) - 1
    dev = torch.device("cuda", engine.device)
    t_data = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
    t_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    opts = SearchOptions().threshold(w.threshold)  # normalised by the calls: Default + NonOverlapping
    opts.order_, opts.overlap_ = Order.Default, Overlap.NonOverlapping
    table = ReplacementTable(engine, [None] * len(w.patterns))  # all keep: the output is the input
    bufs = {"rec": torch.empty(max(1 << 16, len(data) // 16) * 32, dtype=torch.uint8, device=dev),
            "seg": torch.empty(max(1 << 16, len(data) // 8) * 32, dtype=torch.uint8, device=dev),
            "out": torch.empty(2 * len(data) + (1 << 20), dtype=torch.uint8, device=dev)}
    t_out_off = torch.empty(nd + 1, dtype=torch.int64, device=dev)
    sb = StagedBatch.from_device(engine, t_data.data_ptr(), t_off.data_ptr(), nd, len(data), stream=sh)

    def grown(key, unit, call):
        while True:
            try:
                return call(bufs[key])
            except Exception as ex:  # FAC_E_OUTPUT_CAPACITY: grow and run again
                need = getattr(ex, "needed", 0)
                if not need:
                    raise
                bufs[key] = torch.empty(int(need * 1.1 + 1024) * unit, dtype=torch.uint8, device=dev)

    modes = {"strip_prefix": _native.FAC_RENDER_STRIP_PREFIX, "strip_suffix": _native.FAC_RENDER_STRIP_SUFFIX,
             "segment_text": _native.FAC_RENDER_SEGMENT_TEXT}
    legs = {k: (lambda m=m: grown("out", 1, lambda o: sb.render_bytes(m, opts, out=o, offsets_out=t_out_off, stream=sh)))
            for k, m in modes.items()}
    legs["segments"] = lambda: grown("seg", 32, lambda o: sb.segment_records(opts, out=o, doc_offsets_out=t_out_off,
                                                                             stream=sh))
    legs["search"] = lambda: grown("rec", 32, lambda o: sb.search_records(opts, out=o, stream=sh))
    legs["replace_keep"] = lambda: grown("out", 1, lambda o: sb.replace_bytes(table, opts, out=o, offsets_out=t_out_off,
                                                                              stream=sh))
    loops = {"strip_prefix": lambda d: engine.strip_prefix(d, opts), "strip_suffix": lambda d: engine.strip_suffix(d, opts),
             "segment_text": lambda d: engine.segment_text(d, opts),
             "segments": lambda d: list(engine.segment_iter(d, opts))}
    for _ in range(2):  # warm-up: buffers, tables, the output sizes
        for fn in legs.values():
            fn()
    idx = np.unique(np.linspace(0, nd - 1, min(sample, nd)).astype(np.int64))
    docs = [data[int(off[d]):int(off[d + 1])].decode("utf-8") for d in idx]
    for d in docs[:50]:
        loops["segment_text"](d)
    ms = {k: [] for k in legs}
    b_ms = {k: [] for k in loops}
    sizes, same = {}, {}
    for rnd in range(rounds):
        for k, fn in legs.items():  # the legs alternate
            t, (out, out_off) = timed(stream, fn)
            ms[k].append(t)
            sizes[k] = int(out.numel()) // (32 if k in ("segments", "search") else 1)
        for k, fn in loops.items():
            t0 = time.perf_counter()
            per_doc = [fn(d) for d in docs]
            b_ms[k].append(1e3 * (time.perf_counter() - t0))
            if rnd == 0:  # the batch's answer for the sample against the loop's
                out, out_off = legs[k]()
                if k == "segments":
                    host = np.frombuffer(out.cpu().numpy().tobytes(), dtype=_native.MATCH_DTYPE)
                    same[k] = all([(int(r["start"]), int(r["end"])) for r in host[int(out_off[d]):int(out_off[d + 1])]] ==
                                  [(sg.matched().start, sg.matched().end) if sg.matched() is not None else
                                   (sg.unmatched().start, sg.unmatched().end) for sg in p] for d, p in zip(idx, per_doc))
                else:
                    host = out.cpu().numpy().tobytes()
                    same[k] = all(host[int(out_off[d]):int(out_off[d + 1])] == p.encode("utf-8")
                                  for d, p in zip(idx, per_doc))
    med = lambda v: float(np.median(v))  # noqa: E731
    spread = lambda v: max(v) - min(v)  # noqa: E731
    res = {"leg": "segment", "config": name, "bytes": len(data), "L": L, "docs": nd, "sample": len(docs), "sizes": sizes,
           "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
           "b_sample_ms": {k: [round(x, 2) for x in v] for k, v in b_ms.items()}, "equal": same}
    for k in loops:
        res[k + "_us_per_doc"] = round(1e3 * med(ms[k]) / nd, 4)
        res[k + "_loop_us_per_doc"] = round(1e3 * med(b_ms[k]) / len(docs), 2)
        res[k + "_over_search"] = round(med(ms[k]) / med(ms["search"]), 4)
        res[k + "_minus_replace_keep_ms"] = round(med(ms[k]) - med(ms["replace_keep"]), 3)
    res["spread_ms"] = {k: round(spread(v), 3) for k, v in ms.items()}
    return res


def dtod_copy_ms(stream, sh, src, nbytes, rounds):
    """The byte movers' yardstick: hipMemcpyDtoDAsync of nbytes on the stream, or None."""
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        hip.hipMemcpyDtoDAsync.restype = ctypes.c_int
        dst = torch.empty(nbytes, dtype=torch.uint8, device=src.device)
        rcs = []
        cp = lambda: rcs.append(hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), nbytes, sh))  # noqa: E731
        cp()
        ms = [round(timed(stream, cp)[0], 4) for _ in range(rounds)]
        return None if any(rcs) or not torch.equal(dst, src[:nbytes]) else ms
    except (OSError, AttributeError):
        return None


def run_template_extract(name, nbytes, L, rounds, leg, profile_only):
    """--template: (r) fac_replace_batch with the plain upper-case table against (t) the same batch
    with every entry Wrap("<b>", "</b>"). --extract: (x) fac_extract_batch with a NULL table against
    (a) fac_search_batch with the same options, both with their results left in HBM."""
    from fuzzy_aho_corasick import Wrap
    w, engine = workload(name, nbytes)
    data = w.haystack
    off = cut_documents(data, L)
    nd = len(off) - 1
    dev = torch.device("cuda", engine.device)
    t_data = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
    t_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    opts = SearchOptions().threshold(w.threshold)
    if leg == "template":
        opts.order_, opts.overlap_ = Order.Default, Overlap.NonOverlapping
    plain = ReplacementTable(engine, [(p if isinstance(p, str) else p.pattern).upper() for p in w.patterns])
    wrapped = ReplacementTable(engine, [Wrap("<b>", "</b>")] * len(w.patterns))
    bufs = {"rec": torch.empty(max(1 << 16, len(data) // 16) * 32, dtype=torch.uint8, device=dev),
            "out": torch.empty(len(data) + (1 << 20), dtype=torch.uint8, device=dev)}
    t_doc_off = torch.empty(nd + 1, dtype=torch.int64, device=dev)
    sb = StagedBatch.from_device(engine, t_data.data_ptr(), t_off.data_ptr(), nd, len(data), stream=sh)

    def grown(call, unit):
        """unit: what the error's `.needed` counts, "out" bytes or "rec" records (`.needed_text`: bytes)"""
        while True:
            try:
                return call()
            except Exception as ex:  # FAC_E_OUTPUT_CAPACITY: grow and run again
                need = {"out": getattr(ex, "needed_text", 0), "rec": 0}
                need[unit] = max(need[unit], getattr(ex, "needed", 0))
                if not any(need.values()):
                    raise
                if need["out"] > bufs["out"].numel():
                    bufs["out"] = torch.empty(int(need["out"] * 1.1 + 1024), dtype=torch.uint8, device=dev)
                if need["rec"] > bufs["rec"].numel() // 32:
                    bufs["rec"] = torch.empty(int(need["rec"] * 1.1 + 1024) * 32, dtype=torch.uint8, device=dev)
                    bufs["ioff"] = torch.empty(bufs["rec"].numel() // 32 + 1, dtype=torch.int64, device=dev)

    bufs["ioff"] = torch.empty(bufs["rec"].numel() // 32 + 1, dtype=torch.int64, device=dev)

    bufs["ioff"] = torch.empty(bufs["rec"].numel() // 32 + 1, dtype=torch.int64, device=dev)
    if leg == "template":
        legs = {"r": lambda: grown(lambda: sb.replace_bytes(plain, opts, out=bufs["out"], offsets_out=t_doc_off,
                                                            stream=sh), "out"),
                "t": lambda: grown(lambda: sb.replace_bytes(wrapped, opts, out=bufs["out"], offsets_out=t_doc_off,
                                                            stream=sh), "out")}
    else:
        legs = {"x": lambda: grown(lambda: sb.extract(None, opts, records_out=bufs["rec"], text_out=bufs["out"],
                                                      doc_offsets_out=t_doc_off, item_offsets_out=bufs["ioff"],
                                                      stream=sh), "rec"),
                "a": lambda: grown(lambda: sb.search_records(opts, out=bufs["rec"], doc_offsets_out=t_doc_off, stream=sh),
                                   "rec")}
    for _ in range(2):  # warm-up: buffers, tables, the output sizes
        for fn in legs.values():
            fn()
    first = "t" if leg == "template" else "x"
    if profile_only:
        for _ in range(3):
            legs[first]()
        return None
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():  # the legs alternate
            t, res = timed(stream, fn)
            ms[k].append(t)
            if k == first:
                out_bytes = int((res[0] if leg == "template" else res[2]).numel())
                items = int(sb.replaced) if leg == "template" else int(res[0].numel()) // 32
    med = lambda v: float(np.median(v))  # noqa: E731
    other = "r" if leg == "template" else "a"
    return {"leg": leg, "config": name, "bytes": len(data), "L": L, "docs": nd, "out_bytes": out_bytes, "items": items,
            "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
            "spread_ms": {k: round(max(v) - min(v), 3) for k, v in ms.items()},
            first + "_minus_" + other + "_ms": round(med(ms[first]) - med(ms[other]), 3),
            "dtod_copy_ms": dtod_copy_ms(stream, sh, bufs["out"], out_bytes, rounds)}


def unicode_workload(nbytes):
    """c5's shape over the C3 scripts (profiles/bench_prefilter_stream.py's text)."""
    if ("u3", nbytes) not in _CACHE:
        from fuzzy_aho_corasick import FuzzyAhoCorasickBuilder, FuzzyLimits
        pats = workloads._words(workloads.XorShift(5).numpy(), workloads.SCRIPTS_C3, 1000, 10, 16, True)
        hay = workloads._haystack(workloads.XorShift(1005).numpy(), workloads.SCRIPTS_C3, pats, nbytes, 1, 1 << 20)
        w = workloads.Workload("u3", pats, hay, 1, 0, True, 0.85, True)
        engine = FuzzyAhoCorasickBuilder().fuzzy(FuzzyLimits().edits(1)).case_insensitive(True).build(pats)
        assert engine.with_prefilter().is_active() and not hay.isascii()
        _CACHE[("u3", nbytes)] = (w, engine)
    return _CACHE[("u3", nbytes)]


def ascii_quarter(data: bytes, off: np.ndarray) -> bytes:
    """`data` with every fourth document replaced by fresh ASCII filler words of its byte length."""
    rng = workloads.XorShift(0xA5C1).numpy()
    filler = np.frombuffer(workloads._fresh_filler(rng, [workloads.ASCII_LOWER], len(data), 2, 12)[:len(data)], np.uint8)
    lens = np.diff(off.astype(np.int64))
    take = np.repeat(np.arange(len(lens)) % 4 == 0, lens)
    out = np.frombuffer(data, np.uint8).copy()
    out[take] = filler[take]
    return out.tobytes()


def prefilter_workload(name, nbytes):
    """c2 / c5 as workloads.config; c5n: c5's patterns and threshold over fresh filler words alone;
    u3 / u3a: unicode_workload (u3a's documents are replaced once they are cut, run_prefilter)."""
    if name in ("u3", "u3a"):
        return unicode_workload(nbytes)
    if name != "c5n":
        return workload(name, nbytes)
    if (name, nbytes) not in _CACHE:
        w5, engine = workload("c5", 1 << 20)
        rng = workloads.XorShift(0xC5F1).numpy()
        text = workloads._fresh_filler(rng, [workloads.ASCII_LOWER], nbytes, 2, 12)[:nbytes]
        w = workloads.Workload("c5n", w5.patterns, text, w5.edits, w5.beam, w5.case_insensitive, w5.threshold, True)
        _CACHE[(name, nbytes)] = (w, engine)
    return _CACHE[(name, nbytes)]


def run_prefilter(name, nbytes, L, sample, rounds, rules, profile_only):
    w, engine = prefilter_workload(name, nbytes)
    data = w.haystack
    off = cut_documents(data, L)  # (after a space: a grapheme boundary, the texts hold no combining marks)
    if name == "u3a":
        data = ascii_quarter(data, off)
    nd = len(off) - 1
    dev = torch.device("cuda", engine.device)
    t_data = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
    t_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    opts = SearchOptions().threshold(w.threshold)
    bufs = {"out": torch.empty(max(1 << 16, len(data) // 16) * 32, dtype=torch.uint8, device=dev)}
    sb = StagedBatch.from_device(engine, t_data.data_ptr(), t_off.data_ptr(), nd, len(data), stream=sh,
                                 unicode_prefilter=name in ("u3", "u3a"))
    stats = _native.fac_stats()

    def batch_search(prefilter):
        while True:
            try:
                return sb.search_records(opts, out=bufs["out"], stream=sh, prefilter=prefilter,
                                         stats=stats if prefilter else None)
            except Exception as ex:  # FAC_E_OUTPUT_CAPACITY: grow and search again
                need = getattr(ex, "needed", 0)
                if not need:
                    raise
                bufs["out"] = torch.empty(int(need * 1.1 + 1024) * 32, dtype=torch.uint8, device=dev)

    def pf_records(doc):
        out = ctypes.POINTER(_native.fac_match)()
        n = ctypes.c_uint64()
        eg = ctypes.c_uint64()
        rc = _native.lib.fac_search_prefiltered(engine._h, doc, len(doc), f32(w.threshold), ctypes.byref(out),
                                                ctypes.byref(n), ctypes.byref(eg))
        if rc:
            raise RuntimeError(_native.last_error())
        return _native.take_records(out, n.value)

    for rule in rules:  # warm-up: buffers, tables, the output size
        os.environ["FAC_BATCH_RC_SEG"] = str(rule)
        batch_search(True)
    os.environ.pop("FAC_BATCH_RC_SEG")
    batch_search(False)
    if profile_only:
        for _ in range(3):
            batch_search(True)
        return None
    hay = StagedHaystack.from_device(engine, t_data.data_ptr(), len(data), stream=sh)
    hay.search_prefiltered_records(w.threshold, stream=sh)
    idx = np.unique(np.linspace(0, nd - 1, min(sample, nd)).astype(np.int64))
    docs = [data[int(off[d]):int(off[d + 1])] for d in idx]
    for d in docs[:50]:
        pf_records(d)
    p_ms = {r: [] for r in rules}
    pf_ms, a_ms, b_ms, c_ms = [], [], [], []
    for _ in range(rounds):
        for rule in rules:
            os.environ["FAC_BATCH_RC_SEG"] = str(rule)
            stats.prefilter_ms = 0.0
            stats.windows = 0
            ms, (recs, doc_off) = timed(stream, lambda: batch_search(True))
            p_ms[rule].append(ms)
        pf_ms.append(stats.prefilter_ms)
        windows = int(stats.windows)
        os.environ.pop("FAC_BATCH_RC_SEG")
        a_ms.append(timed(stream, lambda: batch_search(False))[0])
        c_ms.append(timed(stream, lambda: hay.search_prefiltered_records(w.threshold, stream=sh))[0])
        t0 = time.perf_counter()
        per_doc = [pf_records(d) for d in docs]
        b_ms.append(1e3 * (time.perf_counter() - t0))
    os.environ["FAC_BATCH_RC_SEG"] = str(rules[-1])
    recs, doc_off = batch_search(True)
    os.environ.pop("FAC_BATCH_RC_SEG")
    host = np.frombuffer(recs.cpu().numpy().tobytes(), dtype=_native.MATCH_DTYPE)
    key = lambda r: sorted(zip(r["start"].tolist(), r["end"].tolist(), r["pattern_index"].tolist(),  # noqa: E731
                               r["similarity"].view(np.uint32).tolist(), r["edits"].tolist()))
    same = all(key(host[int(doc_off[d]):int(doc_off[d + 1])]) == key(p) for d, p in zip(idx, per_doc))
    best_rule = min(rules, key=lambda r: float(np.median(p_ms[r])))
    med = lambda v: float(np.median(v))  # noqa: E731
    p_best = med(p_ms[best_rule])
    b_doc = [m / len(docs) for m in b_ms]
    return {"leg": "prefilter", "config": name, "bytes": len(data), "L": L, "docs": nd, "sample": len(docs),
            "records": int(len(host)), "start_windows": windows,
            "p_ms": {str(r): [round(x, 3) for x in v] for r, v in p_ms.items()}, "best_rule": best_rule,
            "p_prefilter_ms": [round(x, 3) for x in pf_ms], "a_ms": [round(x, 3) for x in a_ms],
            "c_ms": [round(x, 3) for x in c_ms], "b_sample_ms": [round(x, 2) for x in b_ms],
            "p_us_per_doc": round(1e3 * p_best / nd, 4), "b_us_per_doc": [round(1e3 * x, 2) for x in b_doc],
            "p_over_a": round(p_best / med(a_ms), 4), "p_over_c": round(p_best / med(c_ms), 4),
            "p_spread_ms": round(max(p_ms[best_rule]) - min(p_ms[best_rule]), 3),
            "a_spread_ms": round(max(a_ms) - min(a_ms), 3), "c_spread_ms": round(max(c_ms) - min(c_ms), 3),
            "records_equal": bool(same),
            "faster_than_a": bool(same and min(a_ms) - max(p_ms[best_rule]) > 0),
            "faster_than_b": bool(same and min(b_doc) - max(p_ms[best_rule]) / nd > 0)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--c2-bytes", type=int, default=64 << 20)
    ap.add_argument("--c3-bytes", type=int, default=16 << 20)
    ap.add_argument("--lengths", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--configs", nargs="+", default=["c2", "c3"])
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rules", type=int, nargs="+", default=[0, 1024],
                    help="prefix-cache rules to time for leg (a): windows per segment asked for")
    ap.add_argument("--profile-only", nargs="?", const="a", choices=["a", "c"], default=None,
                    help="a few calls of leg (a) (default) or (c) and nothing else (for rocprofv3)")
    ap.add_argument("--replace", action="store_true",
                    help="time fac_replace_batch against fac_search_batch and the per-document replace loop")
    ap.add_argument("--prefilter", action="store_true",
                    help="time fac_search_batch_prefiltered against the plain batch, the one-haystack pre-filtered "
                         "search and the per-document Prefiltered loop (configs c2, c5, c5n; --pf-bytes each)")
    ap.add_argument("--prefilter-unicode", action="store_true",
                    help="the --prefilter legs on opted-in batches of the C3 script mix (configs u3, u3a)")
    ap.add_argument("--pf-bytes", type=int, default=64 << 20)
    ap.add_argument("--segment", action="store_true",
                    help="time fac_render_batch (each mode) and fac_segment_batch against fac_search_batch, the "
                         "all-keep fac_replace_batch and the per-document loops")
    ap.add_argument("--template", action="store_true",
                    help="time fac_replace_batch with a table of Wrap entries against the plain table")
    ap.add_argument("--extract", action="store_true",
                    help="time fac_extract_batch (NULL table) against fac_search_batch with the same options")
    args = ap.parse_args()
    if args.prefilter or args.prefilter_unicode:
        default = ["u3", "u3a"] if args.prefilter_unicode else ["c2", "c5", "c5n"]
        for name in (args.configs if args.configs != ["c2", "c3"] else default):
            for L in args.lengths:
                res = run_prefilter(name, args.pf_bytes, L, args.sample, args.rounds, args.rules, args.profile_only)
                if res is not None:
                    print(json.dumps(res), flush=True)
        return
    for name in args.configs:
        for L in args.lengths:
            if args.template or args.extract:
                res = run_template_extract(name, args.c2_bytes if name == "c2" else args.c3_bytes, L, args.rounds,
                                           "template" if args.template else "extract", args.profile_only)
                if res is not None:
                    print(json.dumps(res), flush=True)
                continue
            if args.segment:
                res = run_segment(name, args.c2_bytes if name == "c2" else args.c3_bytes, L, args.sample, args.rounds)
                print(json.dumps(res), flush=True)
                continue
            if args.replace:
                res = run_replace(name, args.c2_bytes if name == "c2" else args.c3_bytes, L, args.sample, args.rounds,
                                  args.profile_only)
                if res is not None:
                    print(json.dumps(res), flush=True)
                continue
            res = run(name, args.c2_bytes if name == "c2" else args.c3_bytes, L, args.sample, args.rounds, args.rules,
                      args.profile_only)
            if res is not None:
                print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
