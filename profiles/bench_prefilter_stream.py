"""The bitap pre-filter on Unicode text and in the streaming API: three legs, one JSON line each,
appended to profiles/prefilter_stream/bench.jsonl (and printed).

  (a) staged_unicode   search_prefiltered of a device-resident non-ASCII haystack of sparse hits: 64 MiB
                       from workloads.py's generator over the C3 scripts (1 000 patterns of 10-16
                       characters, edits 1, case-insensitive, threshold 0.85, one planted hit per MiB).
                       Every step restages the resident bytes (fac_haystack_stage_device, as bench.py's
                       C3 step does) and searches them, so a step pays what a fresh text pays. Uses
                       only entry points that exist without the streaming work, so the same script
                       measures an older checkout (--pkg).
  (b) stream_ascii     search_stream over an in-memory reader of 1 GiB of sparse ASCII text (the C5
                       generator), pre-filter off and on, alternating.
  (c) stream_unicode   the same for the text of (a).

The texts of (b) and (c) are 64 MiB from the generator repeated to the size asked for. The clock is
the host's around whole calls; every call ends after its last device work was collected. One warm-up
call of each side, then --runs timed ones (alternating where a leg has two sides).

    python profiles/bench_prefilter_stream.py [--legs a b c] [--runs 3] [--stream-mib 1024] [--pkg DIR]
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "profiles", "prefilter_stream", "bench.jsonl")
THRESHOLD = 0.85
UNIT = 64 << 20


def summary(ts):
    return {"seconds": [round(t, 4) for t in ts], "median_s": round(statistics.median(ts), 4),
            "min_s": round(min(ts), 4), "max_s": round(max(ts), 4)}


def emit(res, label):
    res = dict(res, label=label)
    line = json.dumps(res, ensure_ascii=False)
    print(line, flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def texts(W, which):
    """(patterns, 64 MiB of text): the C5 workload, or its shape over the C3 scripts."""
    if which == "ascii":
        wl = W.config("c5", UNIT)
        return wl.patterns, wl.haystack
    rng = W.XorShift(5).numpy()
    pats = W._words(rng, W.SCRIPTS_C3, 1000, 10, 16, True)
    hay = W._haystack(W.XorShift(1005).numpy(), W.SCRIPTS_C3, pats, UNIT, 1, 1 << 20)
    assert not hay.isascii()
    return pats, hay


def engine_for(F, pats):
    eng = F.FuzzyAhoCorasickBuilder().fuzzy(F.FuzzyLimits().edits(1)).case_insensitive(True).device(0).build(pats)
    assert eng.with_prefilter().is_active()
    return eng


def leg_staged(F, W, runs, label):
    import torch
    from fuzzy_aho_corasick.engine import StagedHaystack
    pats, hay = texts(W, "unicode")
    eng = engine_for(F, pats)
    buf = torch.frombuffer(bytearray(hay), dtype=torch.uint8).cuda()
    st, stage_t, search_t, n = None, [], [], 0
    for it in range(runs + 1):  # (run 0 warms up and is not reported)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = StagedHaystack.from_device(eng, buf.data_ptr(), buf.numel(), reuse=st)
        t1 = time.perf_counter()
        rows, _ = st.search_prefiltered_records(THRESHOLD)
        t2 = time.perf_counter()
        n = len(rows)
        if it:
            stage_t.append(t1 - t0)
            search_t.append(t2 - t1)
    med = statistics.median(search_t)
    emit({"leg": "staged_unicode", "bytes": len(hay), "graphemes": st.graphemes, "patterns": len(pats), "records": n,
          "runs": runs, "restage": summary(stage_t), "search_prefiltered": summary(search_t),
          "gchars_per_s": round(st.graphemes / med / 1e9, 3)}, label)


def leg_stream(F, W, which, mib, runs, label):
    pats, unit = texts(W, which)
    eng = engine_for(F, pats)
    reps = max(1, (mib << 20) // len(unit))
    data = unit * reps
    chars = (len(unit) if which == "ascii" else len(unit.decode("utf-8"))) * reps
    sides = {"off": eng}
    if hasattr(F.Prefiltered, "search_stream"):
        sides["on"] = eng.with_prefilter()
    times, counts = {k: [] for k in sides}, {}
    for it in range(runs + 1):
        for k, e in sides.items():
            got = []
            t0 = time.perf_counter()
            total = e.search_stream(io.BytesIO(data), THRESHOLD, got.append)
            dt = time.perf_counter() - t0
            assert total == len(data)
            counts[k] = len(got)
            if it:
                times[k].append(dt)
    res = {"leg": "stream_" + which, "bytes": len(data), "chars": chars, "patterns": len(pats), "runs": runs,
           "matches": counts}
    for k in sides:
        res["prefilter_" + k] = dict(summary(times[k]), gchars_per_s=round(chars / statistics.median(times[k]) / 1e9, 3))
    emit(res, label)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", nargs="+", default=["a", "b", "c"], choices=["a", "b", "c"])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--stream-mib", type=int, default=1024)
    ap.add_argument("--pkg", default=os.path.join(REPO, "fuzzy-aho-corasick-rs_amd"),
                    help="directory holding the fuzzy_aho_corasick package to measure (default: this checkout's)")
    ap.add_argument("--label", default="head", help="written into every line: the commit measured")
    args = ap.parse_args()
    sys.path.insert(0, args.pkg)
    import fuzzy_aho_corasick as F
    from fuzzy_aho_corasick import workloads as W
    for leg in args.legs:
        if leg == "a":
            leg_staged(F, W, args.runs, args.label)
        else:
            leg_stream(F, W, "ascii" if leg == "b" else "unicode", args.stream_mib, args.runs, args.label)


if __name__ == "__main__":
    main()
