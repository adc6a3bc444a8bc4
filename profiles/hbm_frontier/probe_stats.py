"""fac_stats of engines that fit the LDS rungs, and what the deep-frontier searches do, for one build
of the library (run it on the commit before the HBM rungs and on the commit with them):

  python profiles/hbm_frontier/probe_stats.py stats_<name>.json     (written next to this file)

Keys of the output: variant_unbeamed / variant_beamed: test_every_frontier_variant's two engines;
wide_beam: the same text, edits 1, beam_width 3000 (no table rung holds the beam: the dedup-free first
pass takes it); c3_slice, c3_slice_vcap256 / 512: test_frontier_spill_beamed's C3 slice, default and
with FAC_BEAM_VCAP set; edits5 / edits5_beam512: test_frontier_beyond_2048_states; edits6..8:
test_frontier_capacity_is_loud's inputs at those edit counts. Per case: retries, launches
(kernel_launches), rows, ok (rows equal the CPU oracle's), kernel_ms, popped, windows; or the error."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "fuzzy-aho-corasick-rs_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
os.environ["FAC_DIAGNOSTICS"] = "1"

from fuzzy_aho_corasick import FuzzyAhoCorasickBuilder as B, FuzzyLimits as L, workloads  # noqa: E402
from fuzzy_aho_corasick.structs import DeviceError  # noqa: E402
from oracle_harness import OracleEngine  # noqa: E402
from test_gpu_parity import Rng  # noqa: E402

out = {}


def run(name, b, pats, hay, thr):
    try:
        got, st = b.build(pats).stage(hay.encode("utf-8")).search_windows(thr)
        want = OracleEngine(b, pats).raw_rows(hay, thr)
        out[name] = dict(retries=st.retries, launches=st.kernel_launches, rows=len(got), ok=sorted(got) == sorted(want),
                         kernel_ms=st.kernel_ms, popped=st.states_popped, windows=st.windows)
    except DeviceError as e:
        out[name] = dict(error=e.code, text=str(e))
    except Exception as e:  # noqa: BLE001
        out[name] = dict(exc=type(e).__name__, text=str(e))
    print(name, out[name], flush=True)


rng = Rng(0xabcdef)
words = ["needle", "haystack", "fuzzy", "automaton", "école", "Москва"]
text = " ".join(words[rng.next() % 6][: 3 + rng.next() % 6] + "xyzé"[rng.next() % 4] for _ in range(600))
run("variant_unbeamed", B().fuzzy(L().edits(2)), words, text, 0.6)
run("variant_beamed", B().fuzzy(L().edits(2)).beam_width(8).case_insensitive(True), words, text, 0.6)
run("wide_beam", B().fuzzy(L().edits(1)).beam_width(3000), words, text, 0.6)
for bv in ("256", "512"):
    os.environ["FAC_BEAM_VCAP"] = bv
    w = workloads.config("c3", 24 << 10, 3)
    run("c3_slice_vcap" + bv, workloads.builder_for(w), w.patterns, w.haystack.decode("utf-8"), w.threshold)
del os.environ["FAC_BEAM_VCAP"]
w = workloads.config("c3", 24 << 10, 3)
run("c3_slice", workloads.builder_for(w), w.patterns, w.haystack.decode("utf-8"), w.threshold)

pats = ["a" * 12, "ab" * 6, "b" * 12, "ba" * 6]
hay = "ab" * 20 + "a" * 20 + "b" * 20
run("edits5", B().fuzzy(L().edits(5)), pats, hay, 0.3)
run("edits5_beam512", B().fuzzy(L().edits(5)).beam_width(512), pats, hay, 0.3)
for e in (6, 7, 8):
    run(f"edits{e}", B().fuzzy(L().edits(e)), pats, hay, 0.3)

with open(os.path.join(HERE, sys.argv[1]), "w") as f:
    json.dump(out, f, indent=1)
