"""Streams over text that is not ASCII: a task searched as one batch of window documents
(stream_windows_docs) against the same task searched window by window, at the default 256 KiB window
and 32 MiB tasks.

  texts   unicode  workloads.py's generator over the C3 scripts (1 000 patterns of 10-16 characters,
                   edits 1, case-insensitive, threshold 0.85, one planted hit per MiB): 64 MiB repeated
          ascii1   the C5 generator's sparse ASCII text, 64 MiB repeated, with one 'é' per MiB
  legs    search_stream and FuzzyReplacer.replace_stream (every match replaced by "N"), each with the
          pre-filter off and on

Two sides alternate run by run, each a worker process of its own that stays up for the whole session
(so both hold their text and their warmed-up engine, and only one of them works at a time):

  head    this checkout's library
  base    --base-lib PATH: another build of the library (the parent commit's), loaded through FAC_LIB;
          without it, this checkout's library with the path turned off (FAC_STREAM_WINDOW_DOCS=0)

The clock is the host's around whole calls; a call returns after its last task was collected. One
warm-up run of each side and leg, then --runs timed ones. One JSON line per text and leg, printed and
appended to profiles/stream_unicode/bench.jsonl: every time, medians and ranges, and whether the two
sides returned the same matches / output bytes.

    python profiles/bench_stream_unicode.py [--mib 256] [--runs 5] [--base-lib PATH] [--texts unicode ascii1]
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
OUT = os.path.join(REPO, "profiles", "stream_unicode", "bench.jsonl")
THRESHOLD = 0.85
UNIT = 64 << 20
LEGS = [("search", False), ("search", True), ("replace", False), ("replace", True)]


def text_of(W, which):
    if which == "unicode":
        rng = W.XorShift(5).numpy()
        pats = W._words(rng, W.SCRIPTS_C3, 1000, 10, 16, True)
        hay = W._haystack(W.XorShift(1005).numpy(), W.SCRIPTS_C3, pats, UNIT, 1, 1 << 20)
        assert not hay.isascii()
        return pats, hay
    wl = W.config("c5", UNIT)
    hay = bytearray(wl.haystack)
    for mib in range(UNIT >> 20):  # one two-byte character per MiB, in place of two bytes of a filler word
        p = (mib << 20) + (1 << 19)
        while not (hay[p:p + 2].isalpha() and hay[p - 1:p].isalpha() and hay[p + 2:p + 3].isalpha()):
            p += 1
        hay[p:p + 2] = "é".encode()
    hay = bytes(hay)
    hay.decode("utf-8")
    return wl.patterns, hay


class Digest:
    def __init__(self):
        self.h, self.n = hashlib.sha256(), 0

    def write(self, b):
        self.h.update(b)
        self.n += len(b)


def worker(mib):
    """Serve `text leg prefilter` requests on stdin, one JSON answer a line on stdout."""
    sys.path.insert(0, os.path.join(REPO, "fuzzy-aho-corasick-rs_amd"))
    import fuzzy_aho_corasick as F
    from fuzzy_aho_corasick import workloads as W
    from fuzzy_aho_corasick.engine import FuzzyReplacer
    state = {}
    for line in sys.stdin:
        which, leg, pre = line.split()
        pre = pre == "1"
        if which not in state:
            state.clear()  # one text at a time
            pats, unit = text_of(W, which)
            eng = F.FuzzyAhoCorasickBuilder().fuzzy(F.FuzzyLimits().edits(1)).case_insensitive(True).device(0).build(pats)
            assert eng.with_prefilter().is_active()
            state[which] = (eng, FuzzyReplacer(eng, ["N"] * len(pats)), unit * max(1, (mib << 20) // len(unit)),
                            len(unit.decode("utf-8")) * max(1, (mib << 20) // len(unit)))
        eng, rep, data, chars = state[which]
        d = Digest()
        t0 = time.perf_counter()
        if leg == "search":
            total = (eng.with_prefilter() if pre else eng).search_stream(
                io.BytesIO(data), THRESHOLD, lambda m: d.write(b"%d %d %d;" % (m.start, m.end, m.pattern_index)))
        else:
            total = rep.replace_stream(io.BytesIO(data), d, THRESHOLD, prefilter=pre)
        dt = time.perf_counter() - t0
        print(json.dumps({"s": dt, "total": total, "bytes": len(data), "chars": chars, "out": d.n, "sha": d.h.hexdigest()}),
              flush=True)


def summary(ts, chars):
    med = statistics.median(ts)
    return {"seconds": [round(t, 4) for t in ts], "median_s": round(med, 4), "min_s": round(min(ts), 4),
            "max_s": round(max(ts), 4), "gchars_per_s": round(chars / med / 1e9, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--base-lib", default=None, help="the library of the base side (the parent commit's build)")
    ap.add_argument("--texts", nargs="+", default=["unicode", "ascii1"], choices=["unicode", "ascii1"])
    ap.add_argument("--label", default="", help="written into every line")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.mib)
    envs = {"head": dict(os.environ), "base": dict(os.environ)}
    envs["head"].pop("FAC_STREAM_WINDOW_DOCS", None)
    if args.base_lib:
        envs["base"]["FAC_LIB"] = os.path.abspath(args.base_lib)
        base = "library " + os.path.basename(args.base_lib)
    else:
        envs["base"].update(FAC_DIAGNOSTICS="1", FAC_STREAM_WINDOW_DOCS="0")
        base = "this library, FAC_STREAM_WINDOW_DOCS=0"
    procs = {k: subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--mib", str(args.mib)],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=envs[k])
             for k in ("base", "head")}

    def ask(side, which, leg, pre):
        p = procs[side]
        p.stdin.write("%s %s %d\n" % (which, leg, int(pre)))
        p.stdin.flush()
        line = p.stdout.readline()
        if not line:
            sys.exit("the %s worker ended (exit status %s)" % (side, p.wait()))
        return json.loads(line)

    try:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        for which in args.texts:
            for leg, pre in LEGS:
                times, last = {"base": [], "head": []}, {}
                for it in range(args.runs + 1):  # (run 0 warms both sides up and is not reported)
                    for side in ("base", "head"):
                        last[side] = ask(side, which, leg, pre)
                        if it:
                            times[side].append(last[side]["s"])
                h = last["head"]
                res = {"text": which, "leg": leg, "prefilter": pre, "bytes": h["bytes"], "chars": h["chars"],
                       "runs": args.runs, "base_is": base, "label": args.label, "output": h["out"],
                       "outputs_equal": (last["base"]["out"], last["base"]["sha"]) == (h["out"], h["sha"]),
                       "base": summary(times["base"], h["chars"]), "head": summary(times["head"], h["chars"])}
                res["head_over_base"] = round(res["head"]["median_s"] / res["base"]["median_s"], 3)
                line = json.dumps(res)
                print(line, flush=True)
                with open(OUT, "a") as f:
                    f.write(line + "\n")
    finally:
        for p in procs.values():
            p.stdin.close()
            p.wait()


if __name__ == "__main__":
    main()
