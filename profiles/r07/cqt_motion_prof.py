"""Two 1080p 8-bit DecisionPicture steps for a profiler, their launches issued one by one: picture A with commit, finish and motion=(8, 0, 16) -- k_cqt_motion_store
shows as a launch of its own beside k_cqt_block_cells, which reads the same committed cells -- and picture B, the default step with col = A's store --
k_temporal_candidates.  The number of steps as the first argument (default 4).
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/r07/cqt_motion_prof.py 4
  rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d OUT -- python profiles/r07/cqt_motion_prof.py 1      (counters in a run of their own)
from the repository root; cqt_motion_figures.txt holds the result."""
import os, sys
sys.path.insert(0, os.getcwd())
import numpy as np
from turingcodec_amd.havoc import Havoc
from turingcodec_amd.decisions import DecisionPicture
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 4
hv = Havoc(stream="new")
a = DecisionPicture(hv, 1920, 1080, 8, 32, seed=5, intra=False, tree_rates=True, pu_modes=True, cu_close=True, cqt=True, unit_trees=True, commit=True, finish=True,
                    motion=(8, 0, 16))
b = DecisionPicture(hv, 1920, 1080, 8, 32, seed=6, intra=False, col=dict(store=a.cqt_store, col_poc=8, cur_poc=4, target_poc=(0, 8), all_backwards=0, collocated_from_l0=1))
a.use_graphs = b.use_graphs = False
for _ in range(steps):
    a.step()
    b.step()
s, c = a.cqt_motion_results(), b.temporal_candidates()
print("store entries", s.size, "| with list 0", int(s["pred_flag"][..., 0].sum()), "| with list 1", int(s["pred_flag"][..., 1].sum()), "| units", len(b.pus),
      "| candidates", c.size, "available", int(c["available"].sum()), "from the bottom-right cell", int((c["source"] == 1).sum()), "from the centre", int((c["source"] == 2).sum()))
