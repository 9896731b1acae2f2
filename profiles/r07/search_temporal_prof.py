"""Two 1080p 8-bit DecisionPicture pictures for a profiler, their launches issued one by one, both the default step with col = a synthetic store with motion in every
entry: one without temporal_mvp (k_search_rows<1, false>; k_temporal_candidates behind everything) and one with it (k_temporal_candidates first, then
k_search_rows<1, true>).  The number of steps as the first argument (default 4).  Then, where the test tooling is at hand, how many of the picture's derivations
consumed their candidate (the walk over the CPU oracle with the downloaded records, tests/search_temporal_tools.py).
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/r07/search_temporal_prof.py 4
from the repository root; search_temporal_figures.txt holds the result."""
import os, sys
sys.path.insert(0, os.getcwd())
import numpy as np
from turingcodec_amd.havoc import Havoc
from turingcodec_amd import havoc as hmod
from turingcodec_amd.decisions import DecisionPicture
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 4
hv = Havoc(stream="new")
s = np.zeros((68, 120), hmod.COL_CELL_DT)
rng = np.random.default_rng(1)
s["pred_flag"], s["mv"], s["ref_poc"] = 1, rng.integers(-64, 65, (68, 120, 2, 2)), (0, 16)
col = dict(store=hv.up(s.view(np.uint8).reshape(-1)), col_poc=8, cur_poc=4, target_poc=(0, 8), all_backwards=0, collocated_from_l0=1)
off = DecisionPicture(hv, 1920, 1080, 8, 32, seed=5, intra=False, col=col)
on = DecisionPicture(hv, 1920, 1080, 8, 32, seed=5, intra=False, col=col, temporal_mvp=True)
off.use_graphs = on.use_graphs = False
for _ in range(steps):
    r_off = off.step()[0]
    r_on = on.step()[0]
c = on.temporal_candidates()
print("units", len(on.pus), "| derivations", c.size, "| candidates available", int(c["available"].sum()), "| search records that differ",
      int(sum(a.tobytes() != b.tobytes() for a, b in zip(r_on, r_off))), "of", len(r_on), flush=True)
try:
    sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
    import search_temporal_tools as T
except Exception as e:
    print("derivations that consumed the candidate: not counted (%s)" % e)
else:
    case = dict(W=on.W, H=on.H, bd=8, planes=on.host_planes, stride=on.stride, pus=np.ascontiguousarray(on.pus), ctu_first=np.ascontiguousarray(on.ctu_first, np.int32),
                cx=on.cx, cy=on.cy, params=on.params, mvp_rate=on.mvp_rate)
    res, field, bi, rep = T.Client("oracle").walk(case, c, report=True)
    free = rep[..., 0]
    print("derivations that consumed the candidate", int(((c["available"] != 0) & (free >= 0)).sum()), "of", free.size, "| first slot", int((free == 0).sum()),
          "second slot", int((free == 1).sum()), "not consulted", int((free == -1).sum()), "| device results equal that walk:", T.same_records(r_on, res))
