"""The 1080p 8-bit DecisionPicture step with commit=True for a profiler, its launches issued one by one, so that k_cqt_commit and the fill before it show as launches
of their own.  The number of steps as the first argument (default 4).
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/r07/cqt_commit_prof.py 4
  rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d OUT -- python profiles/r07/cqt_commit_prof.py 1      (counters in a run of their own)
from the repository root; cqt_commit_figures.txt holds the result."""
import os, sys
sys.path.insert(0, os.getcwd())
from turingcodec_amd.havoc import Havoc
from turingcodec_amd.decisions import DecisionPicture
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 4
hv = Havoc(stream="new")
dp = DecisionPicture(hv, 1920, 1080, 8, 32, seed=5, intra=False, tree_rates=True, pu_modes=True, cu_close=True, cqt=True, unit_trees=True, commit=True)
dp.use_graphs = False
for _ in range(steps):
    dp.step()
cells = dp.cqt_commit_results()["cells"]
print("searched units", len(dp.pus), "| committed units", len(set(cells["unit"].ravel().tolist()) - {-1}), "| cells", cells.size, "without a unit", int((cells["unit"] < 0).sum()))
