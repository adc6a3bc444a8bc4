#!/usr/bin/env python3
"""Anchored matches of a batch: what the window restriction buys (DESIGN.md 6a "Anchored matches").

The documents are bench_boundaries.py's: the texts of workloads.config("c2") and config("c3") cut at
the space nearest every L bytes, device-resident, after a warm-up. Four legs, alternating, five
rounds, medians and spreads (max - min) reported:

  (l) StagedBatch.lookup_records(k=1), the table left in HBM, timed with device events on the
      call's stream,
  (a) search_records on the batch flagged Anchor.WHOLE (Default + Keep), records left in HBM, device
      events,
  (u) the same call with the flag off: every start window searched (a different result set); the
      expectation is that (a) is not slower than (u) beyond (u)'s own spread,
  (p) the only route there was before: the unflagged search_records with Unsorted + Keep, records to
      the host, then the host filter `start == 0 and end == len(doc)` and the host ranking (best
      similarity first per document); host wall clock, the device call included.

Also reported: the start windows each device leg searched (fac_stats.windows) and whether the three
routes name the same best entry for every document. One JSON line per configuration.
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
from fuzzy_aho_corasick import Anchor, Order, Overlap, SearchOptions, StagedBatch, _native  # noqa: E402


def run(name, nbytes, L, rounds):
    w, engine = workload(name, nbytes)
    data = w.haystack
    off = cut_documents(data, L)
    nd = len(off) - 1
    lens = np.diff(off.astype(np.int64))
    dev = torch.device("cuda", engine.device)
    t_data = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
    t_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    ranked = SearchOptions().threshold(w.threshold)
    ranked.order_, ranked.overlap_ = Order.Default, Overlap.Keep
    raw_opts = SearchOptions().threshold(w.threshold)
    bufs = {"rec": torch.empty(max(1 << 16, len(data) // 16) * 32, dtype=torch.uint8, device=dev)}
    table = torch.empty(nd * 32, dtype=torch.uint8, device=dev)
    sb = StagedBatch.from_device(engine, t_data.data_ptr(), t_off.data_ptr(), nd, len(data), stream=sh)
    windows = {}

    def grown(call):
        while True:
            try:
                return call(bufs["rec"])
            except Exception as ex:  # FAC_E_OUTPUT_CAPACITY: grow and run again
                need = getattr(ex, "needed", 0)
                if not need:
                    raise
                bufs["rec"] = torch.empty(int(need * 1.1 + 1024) * 32, dtype=torch.uint8, device=dev)

    def lookup():
        st = _native.fac_stats()
        r = sb.lookup_records(ranked, 1, out=table, stream=sh, stats=st)
        windows["l"] = int(st.windows)
        return r

    def searched(sides, key):
        st = _native.fac_stats()
        sb.require_anchors(sides)
        r = grown(lambda o: sb.search_records(ranked, out=o, stream=sh, stats=st))
        windows[key] = int(st.windows)
        return r

    def parent_route():
        """Unflagged Unsorted + Keep to the host, the host filter, the host ranking: per document the
        best whole-document record's pattern, or FAC_UNMATCHED."""
        sb.require_anchors(Anchor.NONE)
        recs, doc_off = sb.search_records(raw_opts, stream=sh)
        doc = np.repeat(np.arange(nd), np.diff(doc_off.astype(np.int64)))
        keep = (recs["start"] == 0) & (recs["end"].astype(np.int64) == lens[doc])
        recs, doc = recs[keep], doc[keep]
        # best first: similarity descending, then pattern index
        order = np.lexsort((recs["pattern_index"], -recs["similarity"].astype(np.float64), doc))
        recs, doc = recs[order], doc[order]
        first = np.ones(len(doc), dtype=bool)
        first[1:] = doc[1:] != doc[:-1]
        best = np.full(nd, _native.FAC_UNMATCHED, dtype=np.uint32)
        best[doc[first]] = recs["pattern_index"][first]
        return best, int(keep.sum())

    for _ in range(2):  # warm-up: buffers, tables, the output sizes
        lookup()
        searched(Anchor.WHOLE, "a")
        searched(Anchor.NONE, "u")
        parent_route()
    l_ms, a_ms, u_ms, p_ms = [], [], [], []
    for _ in range(rounds):  # the legs alternate
        ms, (tab, found) = timed(stream, lookup)
        l_ms.append(ms)
        ms, (arec, aoff) = timed(stream, lambda: searched(Anchor.WHOLE, "a"))
        a_ms.append(ms)
        u_ms.append(timed(stream, lambda: searched(Anchor.NONE, "u"))[0])
        t0 = time.perf_counter()
        best_p, n_whole = parent_route()
        p_ms.append(1e3 * (time.perf_counter() - t0))
    tab = np.frombuffer(tab.cpu().numpy().tobytes(), dtype=_native.MATCH_DTYPE)
    arec = np.frombuffer(arec.cpu().numpy().tobytes(), dtype=_native.MATCH_DTYPE)
    best_l = tab["pattern_index"].astype(np.uint32)
    best_a = np.full(nd, _native.FAC_UNMATCHED, dtype=np.uint32)
    has = np.diff(aoff.astype(np.int64)) > 0
    best_a[has] = arec["pattern_index"][aoff[:-1].astype(np.int64)[has]]
    # (the parent route's tie-break is similarity then pattern index; documents whose two best entries
    # tie in similarity may name another entry than Order.Default, which breaks ties by its own key)
    sim_l = tab["similarity"]
    med = lambda v: float(np.median(v))  # noqa: E731
    spread = lambda v: float(max(v) - min(v))  # noqa: E731
    return {"config": name, "bytes": len(data), "L": L, "docs": nd, "whole_records": n_whole,
            "docs_found": int((found > 0).sum()), "windows_lookup": windows["l"], "windows_flagged": windows["a"],
            "windows_unflagged": windows["u"],
            "lookup_ms": [round(x, 3) for x in l_ms], "flagged_ms": [round(x, 3) for x in a_ms],
            "unflagged_ms": [round(x, 3) for x in u_ms], "parent_route_ms": [round(x, 2) for x in p_ms],
            "lookup_med_ms": round(med(l_ms), 3), "lookup_spread_ms": round(spread(l_ms), 3),
            "flagged_med_ms": round(med(a_ms), 3), "flagged_spread_ms": round(spread(a_ms), 3),
            "unflagged_med_ms": round(med(u_ms), 3), "unflagged_spread_ms": round(spread(u_ms), 3),
            "parent_route_med_ms": round(med(p_ms), 2), "parent_route_spread_ms": round(spread(p_ms), 2),
            "flagged_minus_unflagged_ms": round(med(a_ms) - med(u_ms), 3),
            "flagged_not_slower": bool(med(a_ms) <= med(u_ms) + spread(u_ms)),
            "unflagged_over_flagged": round(med(u_ms) / med(a_ms), 2), "parent_over_lookup": round(med(p_ms) / med(l_ms), 2),
            "lookup_equals_flagged": bool((best_l == best_a).all()),
            "found_equal_parent": bool(((best_l != _native.FAC_UNMATCHED) == (best_p != _native.FAC_UNMATCHED)).all()),
            "best_equal_parent": int((best_l == best_p).sum()), "best_similarity_min": float(sim_l[found > 0].min()) if (found > 0).any() else None}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--c2-bytes", type=int, default=64 << 20)
    ap.add_argument("--c3-bytes", type=int, default=16 << 20)
    ap.add_argument("--lengths", type=int, nargs="+", default=[64])
    ap.add_argument("--configs", nargs="+", default=["c2", "c3"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    for name in args.configs:
        for L in args.lengths:
            res = run(name, args.c2_bytes if name == "c2" else args.c3_bytes, L, max(5, args.rounds))
            line = json.dumps(res)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
