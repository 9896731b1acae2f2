"""The 1080p 8-bit DecisionPicture step with commit=True and finish=True for a profiler, its launches issued one by one, so that k_cqt_block_cells and the three stages
behind it show as launches of their own beside the legacy tail's (k_block_cells_blank + k_block_cells, derive_bs, deblocking, padding: earlier in every step).  The
number of steps as the first argument (default 4).
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/r07/cqt_finish_prof.py 4
  rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d OUT -- python profiles/r07/cqt_finish_prof.py 1      (counters in a run of their own)
from the repository root; cqt_finish_figures.txt holds the result."""
import os, sys
sys.path.insert(0, os.getcwd())
import numpy as np
from turingcodec_amd.havoc import Havoc
from turingcodec_amd.decisions import DecisionPicture
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 4
hv = Havoc(stream="new")
dp = DecisionPicture(hv, 1920, 1080, 8, 32, seed=5, intra=False, tree_rates=True, pu_modes=True, cu_close=True, cqt=True, unit_trees=True, commit=True, finish=True)
dp.use_graphs = False
for _ in range(steps):
    dp.step()
r = dp.cqt_finish_results()
print("4x4 cells", r["cells"].size, "| coded", int((r["cells"]["flags"] & 2 != 0).sum()), "| not filtered", int((r["cells"]["flags"] & 4 != 0).sum()),
      "| regions", r["bs"].size, "with a strength", int((r["bs"] != 0).sum()), "| legacy regions with a strength", int((hv.down(dp.d_bs, np.uint8) != 0).sum()))
