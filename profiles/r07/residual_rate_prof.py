"""The 1080p 8-bit DecisionPicture step for a profiler: `rated` or `default` as the first argument, the number of timed steps as the second (default 10; the launches
are issued one by one, not replayed from the graph, so that every kernel shows under its own name).
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/r07/residual_rate_prof.py rated
  rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d OUT -- python profiles/r07/residual_rate_prof.py rated 1      (counters in a run of their own)
from the repository root; residual_rate_figures.txt holds the result."""
import os, sys
sys.path.insert(0, os.getcwd())
from turingcodec_amd.havoc import Havoc
from turingcodec_amd.decisions import DecisionPicture
rated = sys.argv[1] == "rated"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
hv = Havoc(stream="new")
dp = DecisionPicture(hv, 1920, 1080, 8, 32, seed=5, intra=False, residual_rates=rated)
dp.use_graphs = False
for _ in range(steps):
    dp.step()
P = dp.rqt_plan
print("candidates per transform size:", {s: g["m"] for s, g in P["sizes"].items()}, "rate jobs:", {s: len(g["rate_jobs"]) for s, g in P["sizes"].items()} if rated else "-")
