#!/usr/bin/env python3
"""Engines with multi-character mappings on non-ASCII text (DESIGN.md §6a "Batches of non-ASCII
documents for mapping engines", §6b "Grapheme ids of mapping engines").

  --leg a   The first search of a freshly staged Unicode haystack (--mib MiB of words and filler
            that hold both sides of the rules) by an engine with mappings, against the second search
            of the same windows: the difference is what the grapheme ids cost (ensure_gids: built by
            the first search after a staging, kept for the next). Only --windows start windows are
            searched, so the search itself stays small beside it. Host wall clock around
            synchronised calls: the step is synchronous in every build, and in builds that fold on
            the host it is host time that no device event sees. Run once per library
            (FAC_LIB=<another build's libfac.so>) to compare builds; "ids_d2h_bytes" is what a build
            that folds on the host copies back for it (the text and 8 bytes per grapheme).

  --leg b   A column of --names short names, one in five not ASCII, normalised with replace_batch on
            a "ß/ss, æ/ae, œ/oe" engine, three ways, alternating, --runs times each:
              one_call   one opted-in batch (StagedBatch(..., unicode_mappings=True).replace_bytes),
              split      the ASCII names as one batch, the others one by one through engine.replace
                         (what the pre-filtered conveniences do, and the only route before the opt-in),
              loop       engine.replace per name over a fixed sample, scaled to the column.
            Needs a build with fac_batch_allow_unicode_mappings.

One JSON line per leg goes to --out (appended) and to stdout."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "fuzzy-aho-corasick-rs_amd"))

import torch  # noqa: E402

from fuzzy_aho_corasick import (FuzzyAhoCorasickBuilder as B, FuzzyLimits as L, ReplacementTable,  # noqa: E402
                                SearchOptions as O, StagedBatch, StagedHaystack, _native, batch_offsets)

RULES = [("ß", "ss"), ("æ", "ae"), ("œ", "oe")]
VOCAB = ["encyclopædia", "straße", "cœur", "café", "Ωμέγα", "alexandr", "phone", "strasse", "oeuvre", "encyclopaedia"]
FILLER = ["æ", "ae", "ß", "ss", "œ", "é", "é", "ω", "o", " ", "x", "ks", "Æ", "\r\n", "a", "e", "n", "r", "t"]
THR = 0.8


class Rng:  # the tests' xorshift
    def __init__(self, s):
        self.s = s

    def next(self):
        x = self.s
        x ^= (x << 13) & 0xFFFFFFFFFFFFFFFF
        x ^= x >> 7
        x ^= (x << 17) & 0xFFFFFFFFFFFFFFFF
        self.s = x
        return x


def builder():
    b = B().fuzzy(L().edits(1)).case_insensitive(True)
    for a, c in RULES:
        b = b.mapping(a, c)
    return b


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def leg_a(args):
    eng = builder().build(VOCAB)
    rng = Rng(0x5EED_A001)
    block = []
    size = 0
    while size < (1 << 20):  # one MiB of units, repeated: the ids do not care, staging neither
        u = VOCAB[rng.next() % len(VOCAB)] + " " if rng.next() % 7 == 0 else FILLER[rng.next() % len(FILLER)]
        block.append(u)
        size += len(u.encode("utf-8"))
    data = ("".join(block).encode("utf-8")) * args.mib
    runs = []
    for _ in range(args.runs):
        t_stage, sh = wall(lambda: StagedHaystack(eng, data))
        t_first, (_, n1, _) = wall(lambda: sh.search_device(THR, 0, args.windows))
        t_second, (_, n2, _) = wall(lambda: sh.search_device(THR, 0, args.windows))
        assert n1 == n2
        runs.append({"stage_ms": round(t_stage, 2), "first_ms": round(t_first, 2), "second_ms": round(t_second, 2),
                     "ids_ms": round(t_first - t_second, 2), "records": n1})
        graphemes = sh.graphemes
        del sh
    return {"leg": "a", "lib": os.path.basename(_native.LIB_PATH), "bytes": len(data), "graphemes": graphemes,
            "windows": args.windows, "ids_d2h_bytes": len(data) + 8 * graphemes, "ids_h2d_bytes": 4 * graphemes, "runs": runs}


FIRST = ["anna", "jürgen", "rené", "zoë", "max", "marie", "hans", "léa", "otto", "emma", "søren", "ida"]
LAST_ASCII = ["strauss", "weiss", "gross", "jaeger", "oehler", "maier", "schmidt", "kraemer", "voss", "oeztuerk", "fischer",
              "meissner", "schloesser", "baeck"]
LAST_UNI = ["strauß", "weiß", "groß", "jæger", "œhler", "müller", "kræmer", "voß", "meißner", "schlœsser", "bæck", "çelik"]
CANON = ["strauss", "weiss", "gross", "jaeger", "oehler", "kraemer", "voss", "meissner", "schloesser", "baeck", "maier", "schmidt"]


def names(n):
    rng = Rng(0x5EED_A002)
    out = []
    for i in range(n):
        if i % 5 == 4:  # one in five is not ASCII
            out.append(FIRST[rng.next() % len(FIRST)] + " " + LAST_UNI[rng.next() % len(LAST_UNI)])
        else:
            f = FIRST[rng.next() % len(FIRST)]
            out.append((f if f.isascii() else "eva") + " " + LAST_ASCII[rng.next() % len(LAST_ASCII)])
    return out


def leg_b(args):
    eng = builder().build(CANON)
    reps = [c.upper() for c in CANON]
    table = ReplacementTable(eng, reps)
    opts = O().threshold(THR)
    col = names(args.names)
    enc = [t.encode("utf-8") for t in col]
    uni = sum(not e.isascii() for e in enc)
    callback = lambda m: reps[m.pattern_index]  # noqa: E731

    def one_call():
        data, offsets = batch_offsets(enc)
        out, off = StagedBatch(eng, data, offsets, unicode_mappings=True).replace_bytes(table, opts)
        return [out[int(off[d]):int(off[d + 1])] for d in range(len(enc))]

    def split():
        idx = [d for d, e in enumerate(enc) if e.isascii()]
        data, offsets = batch_offsets([enc[d] for d in idx])
        out, off = StagedBatch(eng, data, offsets).replace_bytes(table, opts)
        res = [None] * len(enc)
        for k, d in enumerate(idx):
            res[d] = out[int(off[k]):int(off[k + 1])]
        for d, t in enumerate(col):
            if res[d] is None:
                res[d] = eng.replace(t, opts, callback).encode("utf-8")
        return res

    sample = list(range(0, len(col), max(1, len(col) // args.sample)))

    def loop():
        return [eng.replace(col[d], opts, callback).encode("utf-8") for d in sample]

    one_call(), loop()  # warm-up
    t = {"one_call": [], "split": [], "loop": []}
    for _ in range(args.runs):
        ms, a = wall(one_call)
        t["one_call"].append(round(ms, 2))
        ms, s = wall(split)
        t["split"].append(round(ms, 2))
        ms, lo = wall(loop)
        t["loop"].append(round(ms * len(col) / len(sample), 2))
        assert a == s and [a[d] for d in sample] == lo
    changed = sum(x != y for x, y in zip(a, enc))
    best = {k: min(v) for k, v in t.items()}
    return {"leg": "b", "lib": os.path.basename(_native.LIB_PATH), "names": len(col), "non_ascii": uni, "changed": changed,
            "sample": len(sample), "ms": t, "loop_us_per_name": round(best["loop"] * 1e3 / len(col), 1),
            "split_over_one_call": round(best["split"] / best["one_call"], 2),
            "loop_over_one_call": round(best["loop"] / best["one_call"], 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", choices=["a", "b"], required=True)
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--names", type=int, default=100_000)
    ap.add_argument("--sample", type=int, default=5000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mappings", "bench_mappings.jsonl"))
    args = ap.parse_args()
    res = leg_a(args) if args.leg == "a" else leg_b(args)
    line = json.dumps(res, ensure_ascii=False)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
