"""havoc_mi355x_cqt_decide at 1080p (30 x 17 = 510 CTUs of 85 nodes) for a profiler, on synthetic candidates at every node (tests/cqt_tools.make_case: single units and
splits both win at every depth, so the walk visits most of each tree), with WPP and without; and the 1080p 8-bit DecisionPicture step with cqt=True, its launches
issued one by one, so that the picture route's launch shows too.  The number of calls of each as the first argument (default 4).
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/r07/cqt_prof.py 4
  rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d OUT -- python profiles/r07/cqt_prof.py 1      (counters in a run of their own)
from the repository root; cqt_figures.txt holds the result."""
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import cqt_tools as Q
from turingcodec_amd.havoc import Havoc
from turingcodec_amd.decisions import DecisionPicture
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 4
hv = Havoc(stream="new")
case = Q.make_case(seed=5, width=1920, height=1080, ctb_log2=6, min_cb_log2=3, flags=Q.WPP)
for flags in (Q.WPP, 0):        # in the trace: the first `calls` launches of k_cqt_decide are WPP's, the next `calls` the raster chain's
    for _ in range(calls):
        got = hv.cqt_decide(1920, 1080, 6, 3, flags, case["cu_syntax"], case["node_cu"], case["choice"])
    n = got["nodes"]
    print("flags", flags, "CTUs", len(got["ctus"]), "decided", int(got["ctus"]["decided"].sum()), "coding units", int(got["ctus"]["n_cus"].sum()), "nodes visited",
          int((n["choice"] != 0).sum()), "flags priced (full + split)", int(((n["flags"] & 2 != 0) * ((n["cost_full"] >= 0) + 1 * (n["cost_split"] >= 0))).sum()))
if "--picture" in sys.argv:
    dp = DecisionPicture(hv, 1920, 1080, 8, 32, seed=5, intra=False, tree_rates=True, pu_modes=True, cu_close=True, cqt=True)
    dp.use_graphs = False
    for _ in range(calls):
        dp.step()
    d = dp.cqt_decisions
    print("picture: CTUs", len(d["ctus"]), "decided", int(d["ctus"]["decided"].sum()), "coding units", int(d["ctus"]["n_cus"].sum()), "gave up", d["gave_up"])
