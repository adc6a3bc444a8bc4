"""What the HBM rungs cost (DESIGN.md §5 "HBM rungs"). Three searches, each run once to warm up and
then timed: 5000 CJK patterns (every window on the smallest HBM rung), the edits-8 deep frontier
(every LDS rung up to (4096, 4096) and (0, 8192), then an HBM rung: one FAC_PROF line per launch)
and, for comparison, the edits-5 deep frontier of test_frontier_beyond_2048_states, which ends on an
LDS rung. Prints one JSON line per case: fac_stats and the FAC_HBM launches; with the
phase-profiling library (`make -C fuzzy-aho-corasick-rs_amd/csrc prof`, FAC_LIB=.../libfac_prof.so)
also the FAC_PROF lines, whose `clear=` / `window_total=` cycles give the table clear's share.

  python profiles/hbm_frontier/measure.py > profiles/hbm_frontier/<name>.jsonl"""
import json
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(REPO, "fuzzy-aho-corasick-rs_amd")]

PATS = ["a" * 12, "ab" * 6, "b" * 12, "ba" * 6]
HAY = "ab" * 20 + "a" * 20 + "b" * 20
CJK = [chr(0x4E00 + i) + "東京" for i in range(5000)]
H2 = "".join(chr(0x4E00 + (i * 37) % 5000) + ("東京" if i % 3 else "東亰") + "。" for i in range(60))
CASES = {"cjk5000_edits1": (1, CJK, H2, 0.6), "deep_edits8": (8, PATS, HAY, 0.3), "deep_edits5_lds": (5, PATS, HAY, 0.3)}


def child(name):
    os.environ["FAC_DIAGNOSTICS"] = "1"
    from fuzzy_aho_corasick import FuzzyAhoCorasickBuilder as B, FuzzyLimits as L
    edits, pats, hay, thr = CASES[name]
    staged = B().fuzzy(L().edits(edits)).build(pats).stage(hay.encode("utf-8"))
    staged.search_windows(thr)
    os.environ["FAC_RC_DEBUG"] = "1"
    sys.stderr.write("MEASURED\n")
    sys.stderr.flush()
    got, st = staged.search_windows(thr)
    print(json.dumps({"rows": len(got), "kernel_ms": st.kernel_ms, "kernel_launches": st.kernel_launches,
                      "retries": st.retries, "windows": st.windows, "states_popped": st.states_popped}))


def main():
    for name in CASES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), name], capture_output=True, text=True, timeout=300)
        if p.returncode:
            print(json.dumps({"case": name, "error": p.returncode, "stderr": p.stderr[-400:]}), flush=True)
            sys.exit(1)
        rec = {"case": name, "lib": os.path.basename(os.environ.get("FAC_LIB", "libfac.so"))}
        rec.update(json.loads(p.stdout.strip().splitlines()[-1]))
        err = p.stderr.split("MEASURED\n", 1)[-1]
        rec["hbm_launches"] = [dict(zip(("vcap", "qcap", "windows", "slots"), map(int, m)))
                               for m in re.findall(r"FAC_HBM rung=(\d+),(\d+) windows=(\d+) slots=(\d+)", err)]
        prof = []
        # prologue = the table clear, the (absent) snapshot load and the fence that waits for the clear's
        # stores; clear = issuing the stores alone
        for m in re.finditer(r"FAC_PROF main variant=(\d+),(\d+) .*?window_total=(\d+) batches=(\d+) .*?main_popped=(\d+) "
                             r"prologue=(\d+) .*?prologue: clear=(\d+) load=(\d+)", err):
            v, q, total, batches, popped, prologue, clear, load = map(int, m.groups())
            prof.append({"vcap": v, "qcap": q, "window_cycles": total, "batches": batches, "popped": popped,
                         "prologue_cycles": prologue, "clear_issue_cycles": clear,
                         "prologue_share": round(prologue / total, 4) if total else None})
        if prof:
            rec["phases"] = prof
        if rec["kernel_ms"]:
            rec["states_per_second"] = rec["states_popped"] / (rec["kernel_ms"] * 1e-3)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    child(sys.argv[1]) if len(sys.argv) > 1 else main()
