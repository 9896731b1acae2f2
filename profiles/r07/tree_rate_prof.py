"""The 1080p 8-bit DecisionPicture step for a profiler: `tree`, `residual` or `default` as the first argument, the number of steps as the second (default 10; the
launches are issued one by one, not replayed from the graph, so that every kernel shows under its own name).
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/r07/tree_rate_prof.py tree
  rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d OUT -- python profiles/r07/tree_rate_prof.py tree 1      (counters in a run of their own)
from the repository root; tree_rate_figures.txt holds the result."""
import os, sys
sys.path.insert(0, os.getcwd())
from turingcodec_amd.havoc import Havoc
from turingcodec_amd.decisions import DecisionPicture
mode = sys.argv[1]
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
hv = Havoc(stream="new")
dp = DecisionPicture(hv, 1920, 1080, 8, 32, seed=5, intra=False, **{"tree": {"tree_rates": True}, "residual": {"residual_rates": True}, "default": {}}[mode])
dp.use_graphs = False
for _ in range(steps):
    dp.step()
P = dp.rqt_plan
print("luma candidates per transform size:", {s: g["m"] for s, g in P["sizes"].items()})
if mode == "tree":
    print("chroma candidates per transform size:", {s: g["m"] for s, g in P["csizes"].items()}, "trees per (unit size, depth):", {k: len(t["jobs"]) for k, t in P["tree_jobs"].items()})
    r, t = dp.rqt_results, dp.rqt_tree_results
    print("units", len(r), "untried", int((r["tried_zero"] == 0).sum()), "depth 0", int(((r["depth"] == 0) & (r["tried_zero"] == 1)).sum()), "depth 1", int((r["depth"] == 1).sum()),
          "depth-1 trees coded in chroma only", int(((t["mask_one"] != 0) & ((t["mask_one"] & 15) == 0)).sum()))
