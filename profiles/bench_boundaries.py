#!/usr/bin/env python3
"""Whole-token matches of a batch: what the device filter costs (DESIGN.md 6a "Whole-token matches").

The documents are bench_batch.py's: the texts of workloads.config("c2") and config("c3") cut at the
space nearest every L bytes, device-resident, after a warm-up. Three legs, the first two alternating:

  (w) one fac_replace_batch call on the batch flagged FAC_BOUNDARY_WHOLE, bytes and offsets left in
      HBM, timed with device events on the call's stream,
  (r) the same call with the flag off: the cost floor (a different result set),
  (h) the only route there was before: per document of a fixed sample, search_raw (Unsorted + Keep,
      records to the host), FuzzyMatches.retain_boundaries, apply, replace; host wall clock.

Reported: (w) - (r) beside the spread of (r) over its own repeats, (w) per document against (h) per
document, and how many raw records the filter dropped. One JSON line per configuration. The filter
kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats` run of --profile-only;
"filter_bytes" is what it must move: 32 B read per raw record, 32 B written per kept one, plus the
neighbour bytes (at least one byte per side looked at).
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "fuzzy-aho-corasick-rs_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_batch import cut_documents, timed, workload  # noqa: E402
from fuzzy_aho_corasick import Boundary, Order, Overlap, ReplacementTable, SearchOptions, StagedBatch  # noqa: E402
from fuzzy_aho_corasick.engine import _rendered_entry  # noqa: E402


def run(name, nbytes, L, sample, rounds, profile_only):
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
    raw_opts = SearchOptions().threshold(w.threshold)
    reps = [(p if isinstance(p, str) else p.pattern).upper() for p in w.patterns]
    table = ReplacementTable(engine, reps)
    bufs = {"out": torch.empty(len(data) + (1 << 20), dtype=torch.uint8, device=dev),
            "rec": torch.empty(max(1 << 16, len(data) // 16) * 32, dtype=torch.uint8, device=dev)}
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

    def replace(sides):
        sb.require_boundaries(sides)
        return grown("out", 1, lambda o: sb.replace_bytes(table, opts, out=o, offsets_out=t_out_off, stream=sh))

    def raw_count(sides):
        sb.require_boundaries(sides)
        return int(grown("rec", 32, lambda o: sb.search_records(raw_opts, out=o, stream=sh))[0].numel()) // 32

    for _ in range(2):  # warm-up: buffers, tables, the class table, the output sizes
        replace(Boundary.WHOLE)
        replace(Boundary.NONE)
    if profile_only:
        for _ in range(3):
            replace(Boundary.WHOLE)
        return None
    n_raw, n_kept = raw_count(Boundary.NONE), raw_count(Boundary.WHOLE)
    n_start, n_end = raw_count(Boundary.START), raw_count(Boundary.END)

    def host_route(doc):
        ms = engine.search_raw(doc, w.threshold).retain_boundaries(Boundary.WHOLE)
        return engine.apply_on_device(ms, opts.order_, opts.overlap_).replace(lambda m: _rendered_entry(reps[m.pattern_index], m))

    idx = np.unique(np.linspace(0, nd - 1, min(sample, nd)).astype(np.int64))
    docs = [data[int(off[d]):int(off[d + 1])].decode("utf-8") for d in idx]
    for d in docs[:50]:
        host_route(d)
    w_ms, r_ms, h_ms = [], [], []
    for rnd in range(rounds):  # the legs alternate
        ms, (out, out_off) = timed(stream, lambda: replace(Boundary.WHOLE))
        w_ms.append(ms)
        if rnd == 0:
            host, host_off, replaced_w = out.cpu().numpy().tobytes(), out_off.copy(), int(sb.replaced)
        r_ms.append(timed(stream, lambda: replace(Boundary.NONE))[0])
        replaced_r = int(sb.replaced)
        if rnd < 3:  # the host route is slow and steady: three repeats
            t0 = time.perf_counter()
            per_doc = [host_route(d) for d in docs]
            h_ms.append(1e3 * (time.perf_counter() - t0))
    same = all(host[int(host_off[d]):int(host_off[d + 1])] == p.encode("utf-8") for d, p in zip(idx, per_doc))
    med = lambda v: float(np.median(v))  # noqa: E731
    w_doc, h_doc = med(w_ms) / nd, med(h_ms) / len(docs)
    delta, r_spread = med(w_ms) - med(r_ms), max(r_ms) - min(r_ms)
    # the sides looked at: END for every raw record, START for the ones whose end side passed
    sides_read = n_raw + n_end
    return {"config": name, "bytes": len(data), "L": L, "docs": nd, "sample": len(docs),
            "raw_records": n_raw, "kept_whole": n_kept, "dropped": n_raw - n_kept, "kept_start_only": n_start,
            "kept_end_only": n_end, "replaced_w": replaced_w, "replaced_r": replaced_r,
            "w_ms": [round(x, 3) for x in w_ms], "r_ms": [round(x, 3) for x in r_ms],
            "h_sample_ms": [round(x, 2) for x in h_ms],
            "w_minus_r_ms": round(delta, 3), "r_spread_ms": round(r_spread, 3), "w_spread_ms": round(max(w_ms) - min(w_ms), 3),
            "inside_r_spread": bool(abs(delta) <= r_spread),
            "w_us_per_doc": round(1e3 * w_doc, 4), "h_us_per_doc": round(1e3 * h_doc, 2), "w_over_h": round(w_doc / h_doc, 6),
            "filter_bytes": 32 * n_raw + 32 * n_kept + sides_read, "bytes_equal": bool(same)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--c2-bytes", type=int, default=64 << 20)
    ap.add_argument("--c3-bytes", type=int, default=16 << 20)
    ap.add_argument("--lengths", type=int, nargs="+", default=[64])
    ap.add_argument("--configs", nargs="+", default=["c2", "c3"])
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--profile-only", action="store_true", help="a few calls of leg (w) and nothing else (for rocprofv3)")
    args = ap.parse_args()
    for name in args.configs:
        for L in args.lengths:
            res = run(name, args.c2_bytes if name == "c2" else args.c3_bytes, L, args.sample, max(5, args.rounds),
                      args.profile_only)
            if res is None:
                continue
            line = json.dumps(res)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
