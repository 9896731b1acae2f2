"""Two 1080p 8-bit DecisionPicture steps for a profiler, their launches issued one by one: picture A with commit, finish and motion=(8, 0, 16) -- k_cqt_motion_store --
and picture B with the same options, motion=(4, 0, 8), col = A's store and merge_lists=5 -- k_temporal_candidates and k_cqt_merge_lists in one trace.  The number of
steps as the first argument (default 4).
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/r07/merge_list_prof.py 4
  rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d OUT -- python profiles/r07/merge_list_prof.py 1      (counters in a run of their own)
from the repository root; merge_list_figures.txt holds the result."""
import os, sys
sys.path.insert(0, os.getcwd())
import numpy as np
from turingcodec_amd.havoc import Havoc
from turingcodec_amd.decisions import DecisionPicture
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 4
hv = Havoc(stream="new")
full = dict(intra=False, tree_rates=True, pu_modes=True, cu_close=True, cqt=True, unit_trees=True, commit=True, finish=True)
a = DecisionPicture(hv, 1920, 1080, 8, 32, seed=5, motion=(8, 0, 16), **full)
b = DecisionPicture(hv, 1920, 1080, 8, 32, seed=6, motion=(4, 0, 8), merge_lists=5,
                    col=dict(store=a.cqt_store, col_poc=8, cur_poc=4, target_poc=(0, 8), all_backwards=0, collocated_from_l0=1), **full)
a.use_graphs = b.use_graphs = False
for _ in range(steps):
    a.step()
    b.step()
m, c = b.cqt_merge_results(), b.temporal_candidates()
final = m["n_cand"] == 5
print("units", len(b.pus), "| final", int(final.sum()), "| match per index", [int((m["match"][final] == k).sum()) for k in range(5)], "none", int((m["match"][final] < 0).sum()),
      "| n_real histogram", np.bincount(m["n_real"][final], minlength=6).tolist(), "| units with a temporal candidate", int(c["available"].any(axis=1)[final].sum()))
