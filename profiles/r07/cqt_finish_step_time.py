"""One-picture step time of DecisionPicture at 1080p 8-bit: by default, with tree_rates + pu_modes + cu_close + cqt + unit_trees + commit, and with finish on top (median
of 10 steps after 3 warm-up steps; every step's time is printed, so that the series can be written down).  The modes run in the order given, so `commit finish commit
finish commit finish` alternates them three times over in one process.  A tree without an option (the parent commit) is timed on what it has: run its own
cqt_commit_step_time.py alternately with this script on the same box to set the default step beside the parent's, and take the parent's run-to-run spread from its
repeated runs.
python profiles/r07/cqt_finish_step_time.py [mode ...]  (from the repository root; modes: default commit finish; cqt_finish_figures.txt holds the result)"""
import inspect, os, sys, time, statistics
sys.path.insert(0, os.getcwd())
import numpy as np
from turingcodec_amd.havoc import Havoc
from turingcodec_amd.decisions import DecisionPicture
hv = Havoc(stream="new")
have = inspect.signature(DecisionPicture.__init__).parameters
commit = {"tree_rates": True, "pu_modes": True, "cu_close": True, "cqt": True, "unit_trees": True, "commit": True}
options = {"default": {}, "commit": commit, "finish": dict(commit, finish=True)}
for mode in (sys.argv[1:] or ["default", "commit", "finish"]):
    if any(k not in have for k in options[mode]):
        continue
    dp = DecisionPicture(hv, 1920, 1080, 8, 32, seed=5, **options[mode])
    for _ in range(3):
        dp.step()
    t = []
    for _ in range(10):
        t0 = time.perf_counter()
        dp.step()
        t.append((time.perf_counter() - t0) * 1e3)
    print(f"1920x1080 8-bit DecisionPicture.step() {mode}: median {statistics.median(t):.2f} ms  min {min(t):.2f}  max {max(t):.2f}  "
          f"series {' '.join(f'{v:.2f}' for v in t)}", flush=True)
    if mode == "finish":
        r = dp.cqt_finish_results()
        pad = dp.PAD
        print(f"  4x4 cells {r['cells'].size}  coded {int((r['cells']['flags'] & 2 != 0).sum())}  not filtered {int((r['cells']['flags'] & 4 != 0).sum())}  "
              f"regions with a strength {int((r['bs'] != 0).sum())} of {r['bs'].size}  luma samples in the picture {int(r['recon'][pad:pad + dp.H, pad:pad + dp.W].size)}", flush=True)
    del dp
