"""Streaming replace, device splice against the host splice, on the workload of the crate's
examples/replace_bench.rs: "the quick brown fox jumps over the lazy dog " x 12, then "needle " or
"neeedle " in turn; edits(1), case-insensitive, threshold 0.85, every match replaced by "N".

  device  FuzzyReplacer.replace_stream: fac_replace_stream_* (search, plan and copy kernels on the GPU,
          the output copied back per task)
  host    engine.replace_stream(..., lambda m: "N"): fac_stream_* for the matches, then one Python
          iteration per match over a bytearray (the only path before the device stream existed)

Both write into a sink that keeps the chunks, in the same process, alternating, after a warm-up run
of each; the clock is the host's around whole calls (a call returns after its last task was
collected, so the device is idle). One JSON line per size: the times of every alternation, their
medians and ranges, and whether the two outputs were equal byte for byte.

    python profiles/bench_replace_stream.py [--sizes 32 256] [--alternations 5] [--only device|host]

--only runs one side alone (for a kernel trace: rocprofv3 --kernel-trace --stats -- python ... --only device).
"""
import argparse
import hashlib
import io
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fuzzy-aho-corasick-rs_amd"))

from fuzzy_aho_corasick import FuzzyAhoCorasickBuilder, FuzzyLimits  # noqa: E402
from fuzzy_aho_corasick.engine import FuzzyReplacer  # noqa: E402

THRESHOLD = 0.85


def workload(mib: int) -> bytes:
    filler = "the quick brown fox jumps over the lazy dog " * 12
    pair = (filler + "needle " + filler + "neeedle ").encode()
    n = mib << 20
    return (pair * (n // len(pair) + 1))[:n]


class Sink:
    def __init__(self):
        self.chunks, self.n = [], 0

    def write(self, b):
        self.chunks.append(bytes(b))
        self.n += len(b)

    def digest(self):
        h = hashlib.sha256()
        for c in self.chunks:
            h.update(c)
        return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[32, 256], help="input sizes in MiB")
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--only", choices=["device", "host"], default=None)
    args = ap.parse_args()
    eng = FuzzyAhoCorasickBuilder().fuzzy(FuzzyLimits().edits(1)).case_insensitive(True).device(0).build(["needle"])
    replacer = FuzzyReplacer(eng, ["N"])
    sides = {
        "device": lambda r, w: replacer.replace_stream(r, w, THRESHOLD),
        "host": lambda r, w: eng.replace_stream(r, w, THRESHOLD, lambda m: "N"),
    }
    names = [args.only] if args.only else ["device", "host"]
    for mib in args.sizes:
        data = workload(mib)
        times = {k: [] for k in names}
        digests = {}
        for it in range(args.alternations + 1):  # (run 0 warms both sides up and is not reported)
            for k in names:
                sink = Sink()
                t0 = time.perf_counter()
                n = sides[k](io.BytesIO(data), sink)
                dt = time.perf_counter() - t0
                assert n == sink.n
                if it == 0:
                    digests[k] = (sink.n, sink.digest())
                else:
                    times[k].append(dt)
        res = {"input_mib": mib, "alternations": args.alternations,
               "output_bytes": digests[names[0]][0],
               "outputs_equal": len(set(digests.values())) == 1 if len(names) == 2 else None}
        for k in names:
            res[k] = {"seconds": [round(t, 4) for t in times[k]], "median_s": round(statistics.median(times[k]), 4),
                      "min_s": round(min(times[k]), 4), "max_s": round(max(times[k]), 4),
                      "mib_per_s": round(mib / statistics.median(times[k]), 1)}
        print(json.dumps(res), flush=True)
        if res["outputs_equal"] is False:
            sys.exit("the device and the host splice disagree")


if __name__ == "__main__":
    main()
