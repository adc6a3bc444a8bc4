"""Direct calls on different haystacks: profiles/carry_over/measure.py's
protocol over --n (at least eight) distinct haystacks and a list of knob settings. One C3 engine per
setting; --n + 1 haystacks of --mib MiB held in HBM, all of the bench's 50 000-word vocabulary with
their own word orders and plants (or, with --vocab 0, of fresh random words). After one untimed call
on the last haystack the bench's step (device staging, search, records D2H) is timed on the others in
turn, --cycles times: no call of the first cycle searches a haystack an earlier call has seen. The
same calls are then replayed untimed on a new engine with FAC_RC_DEBUG=launch for each call's direct
decision (unknown_pm, floor_pm, why) and its carried share. One JSON line per timed call, one summary
line per setting.

  python profiles/direct/measure_direct.py --settings default,no_direct,pm0,pm5,pm20,pm50,pm100,cgrid4,cgrid8

FAC_LIB=<the parent commit's library> --settings parent measures the parent. --hay-dir keeps the
generated haystacks, so a second run (the other library) reads them back."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REPO, "fuzzy-aho-corasick-rs_amd"), os.path.join(os.path.dirname(HERE), "carry_over")]

import measure as carry  # noqa: E402  (profiles/carry_over/measure.py: the haystacks, the stderr capture)

SETTINGS = {
    "parent": {},
    "default": {},
    "no_direct": {"FAC_RC_NO_DIRECT": "1"},
    "no_carry": {"FAC_RC_NO_CARRY": "1"},
    "cgrid4": {"FAC_RC_NO_DIRECT": "1", "FAC_RC_CGRID2": "4"},
    "cgrid8": {"FAC_RC_NO_DIRECT": "1", "FAC_RC_CGRID2": "8"},
}
for pm in (0, 5, 10, 20, 50, 100):
    SETTINGS[f"pm{pm}"] = {"FAC_RC_DIRECT_PM": str(pm)}


def haystacks(W, wl, nbytes, vocab, n, hay_dir):
    out, vocab_b = [], None
    for i in range(n):
        path = os.path.join(hay_dir, f"c3_v{vocab}_{nbytes}_{i}.bin") if hay_dir else None
        if path and os.path.exists(path):
            out.append(np.fromfile(path, dtype=np.uint8).tobytes())
            continue
        if vocab:
            if vocab_b is None:  # the bench's: drawn first from its haystack seed
                rng = W.XorShift(3 + 1000).numpy()
                vocab_b = [w.encode("utf-8") for w in W._words(rng, W.SCRIPTS_C3, vocab, 2, 12, distinct=False)]
            hay = carry.vocabulary_haystack(W, wl.patterns, vocab_b, nbytes, 7000 + i)
        else:
            hay = W.config("c3", nbytes, seed=3, hay_seed=7000 + i, vocab=None).haystack
        if path:
            os.makedirs(hay_dir, exist_ok=True)
            np.frombuffer(hay, dtype=np.uint8).tofile(path)
        out.append(hay)
    return out


def direct_of(err):
    line = [ln for ln in err.splitlines() if ln.startswith("FAC_RC windows=") and "| carry" in ln]
    if not line:
        return None
    part = line[-1].split("| carry", 1)[1]
    m = re.search(r"direct=([01]) unknown_pm=(-?\d+) floor_pm=(-?\d+)(?: why=(\w+))?", part)
    lv = re.findall(r"k=(\d+) carried=(\d+) built=(\d+)", part)
    c, b = sum(int(x[1]) for x in lv), sum(int(x[2]) for x in lv)
    s = re.search(r"dir_keys=(\d+) dir_slots=(\d+) reset=(\w+)", part)
    return {"direct": int(m.group(1)) if m else None, "unknown_pm": int(m.group(2)) if m else None,
            "floor_pm": int(m.group(3)) if m else None, "why": m.group(4) if m else None,
            "carried_share": round(c / (c + b), 4) if c + b else None,
            "dir_keys": int(s.group(1)) if s else None, "dir_bytes": int(s.group(2)) * 32 if s else None,
            "reset": s.group(3) if s else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=float, default=256.0)
    ap.add_argument("--vocab", type=int, default=50_000)
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--cycles", type=int, default=2)
    ap.add_argument("--settings", default="default,no_direct")
    ap.add_argument("--hay-dir", default=None)
    args = ap.parse_args()
    os.environ["FAC_DIAGNOSTICS"] = "1"  # read once by the library
    import torch
    from fuzzy_aho_corasick import workloads as W
    from fuzzy_aho_corasick.engine import StagedHaystack

    nbytes = int(args.mib * (1 << 20))
    wl = W.config("c3", 1 << 16, seed=3, hay_seed=1003)  # the bench's C3 patterns and settings
    hays = haystacks(W, wl, nbytes, args.vocab, args.n + 1, args.hay_dir)
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream().cuda_stream
    dev = [torch.from_numpy(np.frombuffer(h, dtype=np.uint8).copy()).to("cuda") for h in hays]
    lib = os.path.basename(os.environ.get("FAC_LIB", "libfac.so"))
    order = [args.n] + list(range(args.n)) * args.cycles

    def run(timed):
        engine = W.builder_for(wl).device(0).build(wl.patterns)
        staged, recs = None, []
        for n, i in enumerate(order):
            torch.cuda.synchronize()
            t = time.perf_counter()
            staged = StagedHaystack.from_device(engine, dev[i].data_ptr(), len(hays[i]), stream, reuse=staged)
            if timed:
                rows, st = staged.search_windows_records(wl.threshold, stream=stream)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t) * 1e3
                recs.append({"call": n, "haystack": i, "ms": round(ms, 3), "records": len(rows),
                             "cache_ms": round(st.cache_ms, 3), "lane_ms": round(st.lane_ms, 3),
                             "kernel_ms": round(st.kernel_ms, 3)})
                del rows
            else:
                with carry.Stderr() as cap:
                    rows, st = staged.search_windows_records(wl.threshold, stream=stream)
                    del rows
                recs.append(direct_of(cap.text))
        return recs

    for name in args.settings.split(","):
        env = SETTINGS[name]
        os.environ.update(env)
        timed = run(True)
        os.environ["FAC_RC_DEBUG"] = "launch"
        info = run(False)
        del os.environ["FAC_RC_DEBUG"]
        for k in env:
            del os.environ[k]
        for rec, d in zip(timed, info):
            rec.update({"setting": name, "lib": lib, "vocab": args.vocab or "fresh", "mib": args.mib})
            rec.update(d or {})
            print(json.dumps(rec), flush=True)
        cyc = [[r["ms"] for r in timed[1 + c * args.n: 1 + (c + 1) * args.n]] for c in range(args.cycles)]
        print(json.dumps({"summary": True, "setting": name, "lib": lib, "vocab": args.vocab or "fresh",
                          "first_call_ms": timed[0]["ms"],
                          "cycle_mean_ms": [round(sum(c) / len(c), 3) for c in cyc],
                          "cycle_min_ms": [min(c) for c in cyc], "cycle_max_ms": [max(c) for c in cyc],
                          "direct_calls": sum(1 for d in info if d and d["direct"])}), flush=True)


if __name__ == "__main__":
    main()
