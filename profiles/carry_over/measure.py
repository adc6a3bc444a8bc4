"""Carry-over between different haystacks: the figure the engine's snapshot
store is judged on. One C3 engine; three haystacks of --mib MiB held in HBM, all of the bench's
50 000-word vocabulary (the vocabulary `bench.py` draws for C3) with their own word orders and planted
patterns, or, with --vocab 0, of fresh random words. After one untimed call on a fourth haystack the
bench's step (device staging, search, records D2H) is timed on the three in turn, --cycles times: no
call of the first cycle searches a haystack an earlier call has seen. Then the same calls are replayed
untimed on an emptied store with FAC_RC_DEBUG=launch, for each call's `carried` / `built` per level and
the store's size. Prints one JSON line per timed call and a summary line.

  python profiles/carry_over/measure.py [--vocab 0] [--hay-dir DIR] > profiles/carry_over/<name>.jsonl

FAC_LIB=<the parent commit's library> measures the parent (no store: the replay reports nothing).
--hay-dir keeps the generated haystacks, so a second run (the other library) reads them back."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(REPO, "fuzzy-aho-corasick-rs_amd")]


def vocabulary_haystack(W, patterns, vocab_b, nbytes, seed, edits=2, plant_every=4096):
    """workloads._haystack's vocabulary branch with the vocabulary given: words drawn with replacement,
    a mutated pattern planted every `plant_every` bytes."""
    rng = W.XorShift(seed).numpy()
    flat = [c for al in W.SCRIPTS_C3 for c in al]
    mean = sum(len(b) for b in vocab_b) / len(vocab_b) + 1
    nw = max(1, int(plant_every / mean))
    chunks, total = [], 0
    while total < nbytes:
        idx = rng.integers(0, len(vocab_b), size=nw)
        p = patterns[int(rng.integers(0, len(patterns)))]
        planted = W._mutate(rng, p, int(rng.integers(0, edits + 1)), flat).encode("utf-8")
        piece = b" ".join(vocab_b[i] for i in idx) + b" " + planted + b" "
        chunks.append(piece)
        total += len(piece)
    data = b"".join(chunks)
    cut = min(nbytes, len(data))
    while cut > 0 and (data[cut - 1] & 0xC0) == 0x80:
        cut -= 1
    if cut > 0 and data[cut - 1] >= 0xC0:
        cut -= 1
    return data[:cut]


def haystacks(W, wl, nbytes, vocab, hay_dir):
    """Four haystacks: [0..2] timed, [3] the untimed first call's."""
    out = []
    vocab_b = None
    for i in range(4):
        path = os.path.join(hay_dir, f"c3_v{vocab}_{nbytes}_{i}.bin") if hay_dir else None
        if path and os.path.exists(path):
            out.append(np.fromfile(path, dtype=np.uint8).tobytes())
            continue
        if vocab:
            if vocab_b is None:  # the bench's: drawn first from its haystack seed
                rng = W.XorShift(3 + 1000).numpy()
                vocab_b = [w.encode("utf-8") for w in W._words(rng, W.SCRIPTS_C3, vocab, 2, 12, distinct=False)]
            hay = vocabulary_haystack(W, wl.patterns, vocab_b, nbytes, 7000 + i)
        else:
            hay = W.config("c3", nbytes, seed=3, hay_seed=7000 + i, vocab=None).haystack
        if path:
            os.makedirs(hay_dir, exist_ok=True)
            np.frombuffer(hay, dtype=np.uint8).tofile(path)
        out.append(hay)
    return out


class Stderr:
    """The process's stderr (the library writes to fd 2) into a file for a while."""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode("utf-8", "replace")
        self.tmp.close()


def carry_of(err):
    line = [ln for ln in err.splitlines() if ln.startswith("FAC_RC windows=") and "| carry" in ln]
    if not line:
        return None
    part = line[-1].split("| carry", 1)[1]
    m = re.search(r"store pool_words=(\d+) dir_keys=(\d+) dir_slots=(\d+) reset=(\w+)", part)
    return {"levels": {k: {"carried": int(c), "built": int(b)}
                       for k, c, b in re.findall(r"k=(\d+) carried=(\d+) built=(\d+)", part)},
            "pool_words": int(m.group(1)), "dir_keys": int(m.group(2)), "dir_bytes": int(m.group(3)) * 32,
            "reset": m.group(4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=float, default=256.0)
    ap.add_argument("--vocab", type=int, default=50_000)
    ap.add_argument("--cycles", type=int, default=2)
    ap.add_argument("--hay-dir", default=None)
    args = ap.parse_args()
    os.environ["FAC_DIAGNOSTICS"] = "1"  # read once by the library: the replay's FAC_RC_DEBUG needs it
    import torch
    from fuzzy_aho_corasick import _native, workloads as W
    from fuzzy_aho_corasick.engine import StagedHaystack

    nbytes = int(args.mib * (1 << 20))
    wl = W.config("c3", 1 << 16, seed=3, hay_seed=1003)  # the bench's C3 patterns and settings
    hays = haystacks(W, wl, nbytes, args.vocab, args.hay_dir)
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream().cuda_stream
    dev = [torch.from_numpy(np.frombuffer(h, dtype=np.uint8).copy()).to("cuda") for h in hays]
    lib = os.path.basename(os.environ.get("FAC_LIB", "libfac.so"))

    def run(engine, timed):
        staged, recs = None, []
        for n, i in enumerate([3] + [0, 1, 2] * args.cycles):
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
                with Stderr() as cap:
                    rows, st = staged.search_windows_records(wl.threshold, stream=stream)
                    del rows
                recs.append(carry_of(cap.text))
        return recs

    engine = W.builder_for(wl).device(0).build(wl.patterns)
    timed = run(engine, True)
    carry = [None] * len(timed)
    if hasattr(_native.lib, "fac_engine_drop_prefix_cache"):
        engine.drop_prefix_cache()
        os.environ["FAC_RC_DEBUG"] = "launch"
        carry = run(engine, False)
        del os.environ["FAC_RC_DEBUG"]
    for rec, c in zip(timed, carry):
        rec.update({"lib": lib, "vocab": args.vocab or "fresh", "mib": args.mib, "carry": c})
        print(json.dumps(rec), flush=True)
    first = [r["ms"] for r in timed[1:4]]
    later = [r["ms"] for r in timed[4:]]
    summary = {"summary": True, "lib": lib, "vocab": args.vocab or "fresh", "mib": args.mib,
               "first_call_ms": timed[0]["ms"], "first_cycle_ms": first, "first_cycle_mean_ms": round(sum(first) / 3, 3),
               "later_cycles_mean_ms": round(sum(later) / len(later), 3) if later else None}
    if carry[-1]:
        tot = lambda c: (sum(v["carried"] for v in c["levels"].values()), sum(v["built"] for v in c["levels"].values()))  # noqa: E731
        shares = [tot(c) for c in carry[1:4]]
        summary["first_cycle_carried_share"] = [round(a / max(1, a + b), 4) for a, b in shares]
        summary["store_pool_bytes"] = carry[-1]["pool_words"] * 16
        summary["store_dir_bytes"] = carry[-1]["dir_bytes"]
        summary["resets"] = [c["reset"] for c in carry]
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
