"""The 1080p 8-bit DecisionPicture step for a profiler: `pu` or `default` as the first argument, the number of steps as the second (default 10; the launches are issued
one by one, not replayed from the graph, so that every kernel shows under its own name).
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/r07/pu_rate_prof.py pu
  rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d OUT -- python profiles/r07/pu_rate_prof.py pu 1      (counters in a run of their own)
from the repository root; pu_rate_figures.txt holds the result."""
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
from turingcodec_amd.havoc import Havoc
from turingcodec_amd.decisions import DecisionPicture
mode = sys.argv[1]
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
hv = Havoc(stream="new")
dp = DecisionPicture(hv, 1920, 1080, 8, 32, seed=5, intra=False, **{"pu": {"pu_modes": True}, "default": {}}[mode])
dp.use_graphs = False
for _ in range(steps):
    dp.step()
if mode == "pu":
    d = dp.pu_decisions
    print("units", len(dp.pus), "per size 8 / 16 / 32 / 64:", np.bincount(dp.pus["w"], minlength=65)[[8, 16, 32, 64]].tolist(), "candidates", dp.pu_plan["M"],
          "modes L0 / L1 / bi:", np.bincount(d["mode"], minlength=3).tolist())
