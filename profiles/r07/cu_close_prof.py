"""The 1080p 8-bit DecisionPicture step with tree_rates, pu_modes and cu_close for a profiler: the number of steps as the first argument (default 4; the launches are
issued one by one, not replayed from the graph, so that every kernel shows under its own name).
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/r07/cu_close_prof.py 4
  rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d OUT -- python profiles/r07/cu_close_prof.py 1      (counters in a run of their own)
from the repository root; cu_close_figures.txt holds the result."""
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
from turingcodec_amd.havoc import Havoc
from turingcodec_amd.decisions import DecisionPicture
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 4
hv = Havoc(stream="new")
dp = DecisionPicture(hv, 1920, 1080, 8, 32, seed=5, intra=False, tree_rates=True, pu_modes=True, cu_close=True)
dp.use_graphs = False
for _ in range(steps):
    dp.step()
d = dp.cu_decisions
print("tree units", len(dp.units), "per size 8 / 16 / 32:", np.bincount(dp.units["log2_size"], minlength=6)[[3, 4, 5]].tolist(), "with a searched unit of their size",
      int((d["searched"] >= 0).sum()), "outcomes refused / coded / no residual / skipped:", np.bincount(d["records"]["outcome"] + 1, minlength=4).tolist())
