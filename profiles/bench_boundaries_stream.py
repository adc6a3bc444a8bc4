#!/usr/bin/env python3
"""Whole-token matches in streams: what the mask costs (DESIGN.md 6a "Whole-token matches", the rule
for a stream), at the default 256 KiB window and 32 MiB tasks.

  texts   c2   workloads.config("c2"): ASCII, 1 000 patterns, edits 1 (the ASCII union path)
          c3   workloads.config("c3"): the Unicode scripts, 10 000 patterns, edits 2, case-insensitive
               (the window-documents path)
  legs    search_stream and replace_stream against a table (every pattern replaced by its upper case)

Three comparisons, one JSON line each per text and leg, printed and appended to
profiles/boundaries/bench_stream.jsonl; every time is a median of --runs (5) runs, the two sides of a
comparison alternating run by run after one warm-up run each:

  unflagged   this build with the mask 0 against --base-tree PATH, a built checkout of the parent commit
              (its library and its package, a worker process of its own). The mask-0 path does nothing
              new, so the expectation is no difference beyond the parent's own run-to-run spread
              ("inside_base_spread"). Left out without --base-tree.
  flagged     Boundary.WHOLE against the mask 0, both this build (a different result set: "rows" and
              "output" differ).
  host        the route the mask replaces, on --sample windows of the text: per window search_raw
              (records to the host), FuzzyMatches.retain_boundaries, apply(Default, NonOverlapping);
              host wall clock per window, and that times the number of windows beside the flagged
              stream's time. (That route has no left context: it is the cost that is compared, not
              the result.)

The clock is the host's around whole calls; a call returns after its last task was collected.

    python profiles/bench_boundaries_stream.py [--c2-mib 64] [--c3-mib 16] [--runs 5] [--base-tree PATH]
"""
import argparse
import hashlib
import io
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "profiles", "boundaries", "bench_stream.jsonl")
WINDOW = 256 * 1024


class Digest:
    def __init__(self):
        self.h, self.n = hashlib.sha256(), 0

    def write(self, b):
        self.h.update(b)
        self.n += len(b)


def worker(tree, sizes):
    """Serve `text leg sides` requests on stdin, one JSON answer a line on stdout. `tree`: the
    checkout whose package and library this process loads."""
    sys.path.insert(0, os.path.join(tree, "fuzzy-aho-corasick-rs_amd"))
    import fuzzy_aho_corasick as F
    from fuzzy_aho_corasick import workloads as W
    state = {}
    for line in sys.stdin:
        which, leg, sides = line.split()
        sides = int(sides)
        if which not in state:
            state.clear()  # one text at a time
            w = W.config(which, sizes[which] << 20)
            eng = W.builder_for(w).build(w.patterns)
            reps = [(p if isinstance(p, str) else p.pattern).upper() for p in w.patterns]
            state[which] = (w, eng, F.ReplacementTable(eng, reps))
        w, eng, table = state[which]
        data = w.haystack
        kw = {"boundaries": F.Boundary(sides)} if sides else {}  # (the parent's calls have no such keyword)
        d = Digest()
        rows = 0
        t0 = time.perf_counter()
        if leg == "search":
            def on_match(m):
                nonlocal rows
                rows += 1
                d.write(b"%d %d %d;" % (m.start, m.end, m.pattern_index))
            eng.search_stream(io.BytesIO(data), w.threshold, on_match, **kw)
        elif leg == "replace":
            eng.replace_stream(io.BytesIO(data), d, w.threshold, table, **kw)
        else:  # host: the sampled windows through search_raw, retain_boundaries, apply
            n_win = max(1, len(data) // WINDOW)
            sample = int(leg.split(":")[1])
            per = []
            for k in range(sample):
                a = (k * n_win // sample) * WINDOW
                while a and data[a] & 0xC0 == 0x80:
                    a += 1
                b = min(len(data), a + WINDOW)
                while b < len(data) and data[b] & 0xC0 == 0x80:
                    b -= 1
                doc = data[a:b].decode("utf-8")
                t1 = time.perf_counter()
                ms = eng.search_raw(doc, w.threshold).retain_boundaries(F.Boundary(sides))
                rows += len(eng.apply_on_device(ms, F.Order.Default, F.Overlap.NonOverlapping).inner)
                per.append(time.perf_counter() - t1)
            print(json.dumps({"s": statistics.median(per), "windows": n_win, "rows": rows, "bytes": len(data)}), flush=True)
            continue
        dt = time.perf_counter() - t0
        print(json.dumps({"s": dt, "bytes": len(data), "rows": rows, "out": d.n, "sha": d.h.hexdigest()}), flush=True)


def summary(ts, nbytes):
    med = statistics.median(ts)
    return {"seconds": [round(t, 4) for t in ts], "median_s": round(med, 4), "min_s": round(min(ts), 4),
            "max_s": round(max(ts), 4), "gb_per_s": round(nbytes / med / 1e9, 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--c2-mib", type=int, default=64)
    ap.add_argument("--c3-mib", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sample", type=int, default=8, help="windows of the host route")
    ap.add_argument("--texts", nargs="+", default=["c2", "c3"], choices=["c2", "c3"])
    ap.add_argument("--base-tree", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--label", default="", help="written into every line")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    sizes = {"c2": args.c2_mib, "c3": args.c3_mib}
    if args.worker:
        return worker(args.worker, sizes)
    env = dict(os.environ)
    for k in ("FAC_LIB", "FAC_DIAGNOSTICS", "FAC_STREAM_BATCH_BYTES", "FAC_STREAM_READ_BYTES"):
        env.pop(k, None)
    trees = {"head": REPO}
    if args.base_tree:
        trees["base"] = os.path.abspath(args.base_tree)
    procs = {k: subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", t, "--c2-mib", str(args.c2_mib),
                                  "--c3-mib", str(args.c3_mib)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True,
                                 env=env) for k, t in trees.items()}

    def ask(side, which, leg, sides):
        p = procs[side]
        p.stdin.write("%s %s %d\n" % (which, leg, sides))
        p.stdin.flush()
        line = p.stdout.readline()
        if not line:
            sys.exit("the %s worker ended (exit status %s)" % (side, p.wait()))
        return json.loads(line)

    def emit(res):
        res["label"] = args.label
        line = json.dumps(res)
        print(line, flush=True)
        with open(OUT, "a") as f:
            f.write(line + "\n")

    def compare(which, leg, a, b):
        """Sides a and b = (worker, mask), alternating; b over a."""
        times, last = {0: [], 1: []}, {}
        for it in range(args.runs + 1):  # (run 0 warms both sides up and is not reported)
            for i, (side, sides) in enumerate((a, b)):
                last[i] = ask(side, which, leg, sides)
                if it:
                    times[i].append(last[i]["s"])
        n = last[1]["bytes"]
        sa, sb = summary(times[0], n), summary(times[1], n)
        return last, sa, sb

    try:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        for which in args.texts:
            flagged_s = {}
            for leg in ("search", "replace"):
                if "base" in procs:
                    last, base, head = compare(which, leg, ("base", 0), ("head", 0))
                    delta = head["median_s"] - base["median_s"]
                    emit({"compare": "unflagged", "text": which, "leg": leg, "bytes": last[1]["bytes"], "runs": args.runs,
                          "base": base, "head": head, "head_over_base": round(head["median_s"] / base["median_s"], 4),
                          "head_minus_base_s": round(delta, 4), "base_spread_s": round(base["max_s"] - base["min_s"], 4),
                          "inside_base_spread": bool(abs(delta) <= base["max_s"] - base["min_s"]),
                          "outputs_equal": (last[0]["out"], last[0]["sha"]) == (last[1]["out"], last[1]["sha"])})
                last, off, on = compare(which, leg, ("head", 0), ("head", 3))
                flagged_s[leg] = on["median_s"]
                emit({"compare": "flagged", "text": which, "leg": leg, "bytes": last[1]["bytes"], "runs": args.runs,
                      "unflagged": off, "flagged": on, "flagged_over_unflagged": round(on["median_s"] / off["median_s"], 4),
                      "flagged_minus_unflagged_s": round(on["median_s"] - off["median_s"], 4),
                      "unflagged_spread_s": round(off["max_s"] - off["min_s"], 4),
                      "rows": [last[0]["rows"], last[1]["rows"]], "output": [last[0]["out"], last[1]["out"]]})
            h = [ask("head", which, "host:%d" % args.sample, 3) for _ in range(3)]
            per = statistics.median(x["s"] for x in h)
            emit({"compare": "host", "text": which, "bytes": h[0]["bytes"], "sample_windows": args.sample,
                  "windows": h[0]["windows"], "host_ms_per_window": round(1e3 * per, 3),
                  "host_s_all_windows": round(per * h[0]["windows"], 3), "flagged_search_stream_s": flagged_s["search"],
                  "host_over_flagged": round(per * h[0]["windows"] / flagged_s["search"], 2)})
    finally:
        for p in procs.values():
            p.stdin.close()
            p.wait()


if __name__ == "__main__":
    main()
