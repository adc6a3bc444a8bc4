#!/usr/bin/env python3
"""Per-document term counts of a batch: the device group-by against the host route (DESIGN.md 6a
"Term counts").

The documents are bench_boundaries.py's: the texts of workloads.config("c2") and config("c3") cut at
the space nearest every L bytes, device-resident, after a warm-up. Default + NonOverlapping, keys =
pattern index. The legs alternate, five rounds, medians and spreads (max - min) reported:

  (d) StagedBatch.count_records, the terms and their index left in HBM, no totals; device events on
      the call's stream,
  (t) the same with the corpus totals, also left in HBM; device events,
  (h) count_records with the terms brought to the host; host wall clock,
  (r) the host route there was before: search_records with the records to the host, then a NumPy
      lexsort + reduceat group-by into the same terms; host wall clock, the device call included,
  (p) leg (r) in a second process that loads another build of the library (--parent-lib, e.g. the
      parent commit's: the route uses only calls that build has), one round of it after every round
      of the legs above.

Also reported: records and terms per call, and whether the host route's terms equal the device's.
One JSON line per configuration.
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "fuzzy-aho-corasick-rs_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_batch import cut_documents, timed, workload  # noqa: E402
from fuzzy_aho_corasick import Order, Overlap, SearchOptions, StagedBatch, _native  # noqa: E402


def group_on_host(recs, doc_off, nd):
    """The terms of search_records' result by NumPy: (terms as a TERM_DTYPE-shaped tuple of arrays, index)."""
    doc = np.repeat(np.arange(nd, dtype=np.int64), np.diff(doc_off.astype(np.int64)))
    pat = recs["pattern_index"].astype(np.int64)
    bits = recs["similarity"].view(np.uint32)
    word = np.where(bits >> 31, ~bits, bits | np.uint32(0x80000000)).astype(np.int64)  # total_cmp as an unsigned compare
    order = np.lexsort((-pat, word, pat, doc))  # per (document, key): the best record last
    doc, pat, sim = doc[order], pat[order], recs["similarity"][order]
    n = len(doc)
    if n == 0:
        return (pat, pat, sim, pat), np.zeros(nd + 1, dtype=np.int64)
    head = np.ones(n, dtype=bool)
    head[1:] = (doc[1:] != doc[:-1]) | (pat[1:] != pat[:-1])
    starts = np.flatnonzero(head)
    count = np.add.reduceat(np.ones(n, dtype=np.int64), starts)
    last = np.append(starts[1:], n) - 1
    index = np.zeros(nd + 1, dtype=np.int64)
    np.cumsum(np.bincount(doc[starts], minlength=nd), out=index[1:])
    return (pat[starts], count, sim[last], pat[last]), index


class Setup:
    def __init__(self, name, nbytes, L):
        w, engine = workload(name, nbytes)
        self.data = w.haystack
        off = cut_documents(self.data, L)
        self.nd = len(off) - 1
        self.dev = torch.device("cuda", engine.device)
        self.t_data = torch.from_numpy(np.frombuffer(self.data, np.uint8).copy()).to(self.dev)
        self.t_off = torch.from_numpy(off.view(np.int64).copy()).to(self.dev)
        self.stream = torch.cuda.current_stream(self.dev)
        self.sh = self.stream.cuda_stream
        self.opts = SearchOptions().threshold(w.threshold)
        self.opts.order_, self.opts.overlap_ = Order.Default, Overlap.NonOverlapping
        self.n_pat = len(engine.patterns_)
        self.sb = StagedBatch.from_device(engine, self.t_data.data_ptr(), self.t_off.data_ptr(), self.nd, len(self.data),
                                          stream=self.sh)

    def host_route(self):
        recs, doc_off = self.sb.search_records(self.opts, stream=self.sh)
        terms, index = group_on_host(recs, doc_off, self.nd)
        return terms, index, len(recs)


def child():
    """Leg (p): `cfg name nbytes L` stages and warms up, `go` runs one round of the host route and
    prints its milliseconds, `quit` ends."""
    s = None
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        if cmd[0] == "cfg":
            s = Setup(cmd[1], int(cmd[2]), int(cmd[3]))
            for _ in range(2):
                s.host_route()
            print("ready", flush=True)
        elif cmd[0] == "go":
            t0 = time.perf_counter()
            s.host_route()
            print(1e3 * (time.perf_counter() - t0), flush=True)


def run(name, nbytes, L, rounds, other):
    s = Setup(name, nbytes, L)
    sb, opts, sh, nd = s.sb, s.opts, s.sh, s.nd
    bufs = {"terms": torch.empty(max(1 << 16, 2 * nd) * 16, dtype=torch.uint8, device=s.dev)}
    d_index = torch.empty(nd + 1, dtype=torch.int64, device=s.dev)
    d_totals = torch.empty((s.n_pat, 2), dtype=torch.int64, device=s.dev)

    def device_leg(totals):
        while True:
            try:
                return sb.count_records(opts, out=bufs["terms"], stream=sh, doc_offsets_out=d_index,
                                        totals=d_totals if totals else False)
            except Exception as ex:  # FAC_E_OUTPUT_CAPACITY: grow and run again
                need = getattr(ex, "needed", 0)
                if not need:
                    raise
                bufs["terms"] = torch.empty(int(need * 1.1 + 1024) * 16, dtype=torch.uint8, device=s.dev)

    if other:
        other.stdin.write(f"cfg {name} {nbytes} {L}\n")
        other.stdin.flush()
        assert other.stdout.readline().strip() == "ready"
    for _ in range(2):  # warm-up: buffers, tables, the output sizes
        device_leg(False)
        device_leg(True)
        sb.count_records(opts, stream=sh)
        s.host_route()
    d_ms, t_ms, h_ms, r_ms, p_ms = [], [], [], [], []
    for _ in range(rounds):  # the legs alternate
        ms, (filled, _, _) = timed(s.stream, lambda: device_leg(False))
        d_ms.append(ms)
        t_ms.append(timed(s.stream, lambda: device_leg(True))[0])
        t0 = time.perf_counter()
        terms, index, _ = sb.count_records(opts, stream=sh)
        h_ms.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        (r_key, r_count, r_sim, r_pat), r_index, n_recs = s.host_route()
        r_ms.append(1e3 * (time.perf_counter() - t0))
        if other:
            other.stdin.write("go\n")
            other.stdin.flush()
            p_ms.append(float(other.stdout.readline()))
    left = np.frombuffer(filled.cpu().numpy().tobytes(), dtype=_native.TERM_DTYPE)
    equal = bool(len(terms) == len(r_key) and (terms["key"] == r_key).all() and (terms["count"] == r_count).all()
                 and (terms["best_similarity"].view(np.uint32) == r_sim.view(np.uint32)).all()
                 and (terms["best_pattern"] == r_pat).all() and (index.astype(np.int64) == r_index).all()
                 and left.tobytes() == terms.tobytes())
    tot = d_totals.cpu().numpy().view(np.uint64)
    med = lambda v: float(np.median(v)) if v else None  # noqa: E731
    spread = lambda v: float(max(v) - min(v)) if v else None  # noqa: E731
    r3 = lambda x: None if x is None else round(x, 3)  # noqa: E731
    res = {"config": name, "bytes": len(s.data), "L": L, "docs": nd, "records": n_recs, "terms": int(len(terms)),
           "docs_with_terms": int((np.diff(index.astype(np.int64)) > 0).sum()), "keys": s.n_pat,
           "totals_count_sum": int(tot[:, 0].sum()), "host_route_equals_device": equal,
           "device_ms": [round(x, 3) for x in d_ms], "device_totals_ms": [round(x, 3) for x in t_ms],
           "to_host_ms": [round(x, 3) for x in h_ms], "host_route_ms": [round(x, 3) for x in r_ms],
           "host_route_other_lib_ms": [round(x, 3) for x in p_ms]}
    for key, v in (("device", d_ms), ("device_totals", t_ms), ("to_host", h_ms), ("host_route", r_ms),
                   ("host_route_other_lib", p_ms)):
        res[key + "_med_ms"], res[key + "_spread_ms"] = r3(med(v)), r3(spread(v))
    res["host_route_over_to_host"] = round(med(r_ms) / med(h_ms), 2)
    res["device_beats_host_route"] = bool(med(h_ms) < med(r_ms))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--c2-bytes", type=int, default=64 << 20)
    ap.add_argument("--c3-bytes", type=int, default=16 << 20)
    ap.add_argument("--lengths", type=int, nargs="+", default=[64])
    ap.add_argument("--configs", nargs="+", default=["c2", "c3"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--commit", default=None, help="what this library was built from (recorded in the output)")
    ap.add_argument("--parent-lib", default=None, help="another build of libfac.so for leg (p)")
    ap.add_argument("--parent-commit", default=None, help="what --parent-lib was built from (recorded in the output)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child()
    other = None
    if args.parent_lib:
        env = dict(os.environ, FAC_LIB=os.path.abspath(args.parent_lib))
        other = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child"], env=env, stdin=subprocess.PIPE,
                                 stdout=subprocess.PIPE, text=True)
    try:
        for name in args.configs:
            for L in args.lengths:
                res = run(name, args.c2_bytes if name == "c2" else args.c3_bytes, L, max(5, args.rounds), other)
                res["commit"], res["parent_commit"] = args.commit, args.parent_commit
                line = json.dumps(res)
                print(line, flush=True)
                if args.out:
                    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                    with open(args.out, "a") as f:
                        f.write(line + "\n")
    finally:
        if other:
            try:
                other.stdin.write("quit\n")
                other.stdin.flush()
            except OSError:
                pass
            other.wait(timeout=60)


if __name__ == "__main__":
    main()
