"""One-picture step time of DecisionPicture at 1080p 8-bit: by default; with tree_rates + pu_modes + cu_close + cqt + unit_trees + commit + finish + motion + col
(`col`); and with merge_lists=5 on top of that (`merge`) -- median of 10 steps after 3 warm-up steps; every step's time is printed, so that the series can be written
down.  The modes run in the order given, so `col merge col merge col merge` alternates them three times over in one process.  A tree without an option (the parent
commit) is timed on what it has: run its own cqt_motion_step_time.py alternately with this script on the same box to set the default step beside the parent's, and take
the parent's run-to-run spread from its repeated runs.
python profiles/r07/merge_list_step_time.py [mode ...]  (from the repository root; modes: default col merge; merge_list_figures.txt holds the result)"""
import inspect, os, sys, time, statistics
sys.path.insert(0, os.getcwd())
import numpy as np
from turingcodec_amd.havoc import Havoc
from turingcodec_amd import havoc as hmod
from turingcodec_amd.decisions import DecisionPicture
hv = Havoc(stream="new")
have = inspect.signature(DecisionPicture.__init__).parameters
col = {"tree_rates": True, "pu_modes": True, "cu_close": True, "cqt": True, "unit_trees": True, "commit": True, "finish": True, "motion": (4, 0, 8), "col": None}
options = {"default": {}, "col": col, "merge": dict(col, merge_lists=5)}
store = None
for mode in (sys.argv[1:] or ["default", "col", "merge"]):
    if any(k not in have for k in options[mode]):
        continue
    o = dict(options[mode])
    if "col" in o:          # a store of the picture's size with motion in every entry: list 0 eight pictures back, list 1 eight ahead
        if store is None:
            s = np.zeros((68, 120), hmod.COL_CELL_DT)
            rng = np.random.default_rng(1)
            s["pred_flag"], s["mv"], s["ref_poc"] = 1, rng.integers(-64, 65, (68, 120, 2, 2)), (0, 16)
            store = hv.up(s.view(np.uint8).reshape(-1))
        o["col"] = dict(store=store, col_poc=8, cur_poc=4, target_poc=(0, 8), all_backwards=0, collocated_from_l0=1)
    dp = DecisionPicture(hv, 1920, 1080, 8, 32, seed=5, **o)
    for _ in range(3):
        dp.step()
    t = []
    for _ in range(10):
        t0 = time.perf_counter()
        dp.step()
        t.append((time.perf_counter() - t0) * 1e3)
    print(f"1920x1080 8-bit DecisionPicture.step() {mode}: median {statistics.median(t):.2f} ms  min {min(t):.2f}  max {max(t):.2f}  "
          f"series {' '.join(f'{v:.2f}' for v in t)}", flush=True)
    if mode == "merge":
        m = dp.cqt_merge_results()
        final = m["n_cand"] == 5
        print(f"  units {len(dp.pus)}  final {int(final.sum())}  with a match {int((m['match'][final] >= 0).sum())}", flush=True)
    del dp
