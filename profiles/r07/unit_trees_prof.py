"""The 1080p 8-bit DecisionPicture step with unit_trees=True for a profiler, its launches issued one by one, so that k_tree_rate<6, 1>, k_unit_pred_select and the
rqt_decide_units launch (k_rqt_decide<3>) show as kernels of their own.  The number of steps as the first argument (default 4).
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/r07/unit_trees_prof.py 4
  rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d OUT -- python profiles/r07/unit_trees_prof.py 1      (counters in a run of their own)
from the repository root; unit_trees_figures.txt holds the result."""
import os, sys
sys.path.insert(0, os.getcwd())
from turingcodec_amd.havoc import Havoc
from turingcodec_amd.decisions import DecisionPicture
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 4
hv = Havoc(stream="new")
dp = DecisionPicture(hv, 1920, 1080, 8, 32, seed=5, intra=False, tree_rates=True, pu_modes=True, cu_close=True, cqt=True, unit_trees=True)
dp.use_graphs = False
for _ in range(steps):
    dp.step()
U = dp.unit_plan
print("searched units", len(dp.pus), "| tree_rate jobs", {k: len(t["jobs"]) for k, t in U["tree_jobs"].items()}, "| luma candidates", {s: g["m"] for s, g in U["sizes"].items()},
      "| chroma candidates", {s: g["m"] for s, g in U["csizes"].items()})
