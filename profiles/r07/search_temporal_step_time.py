"""One-picture step time of DecisionPicture at 1080p 8-bit, QP 32: by default; with col (another picture's store: the candidates are made inside the graph and not read);
with col + temporal_mvp (they are made before the searches and the walk's predictor derivation consumes them) -- median of 10 steps after 3 warm-up steps; every step's
time is printed.  The modes run in the order given, so `col col_mvp col col_mvp col col_mvp` alternates them three times over in one process.  A tree without an option
(the parent commit) is timed on what it has: run this script's `default` alternately in both trees on the same box to set the default step beside the parent's.
python profiles/r07/search_temporal_step_time.py [mode ...]  (from the repository root; modes: default col col_mvp; search_temporal_figures.txt holds the result)"""
import inspect, os, sys, time, statistics
sys.path.insert(0, os.getcwd())
import numpy as np
from turingcodec_amd.havoc import Havoc
from turingcodec_amd import havoc as hmod
from turingcodec_amd.decisions import DecisionPicture
hv = Havoc(stream="new")
have = inspect.signature(DecisionPicture.__init__).parameters
options = {"default": {}, "col": {"col": None}, "col_mvp": {"col": None, "temporal_mvp": True}}
store, plain = None, None
for mode in (sys.argv[1:] or ["default", "col", "col_mvp"]):
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
        res = dp.step()[0]
    t = []
    for _ in range(10):
        t0 = time.perf_counter()
        dp.step()
        t.append((time.perf_counter() - t0) * 1e3)
    print(f"1920x1080 8-bit DecisionPicture.step() {mode}: median {statistics.median(t):.2f} ms  min {min(t):.2f}  max {max(t):.2f}  "
          f"series {' '.join(f'{v:.2f}' for v in t)}", flush=True)
    if mode == "col":
        plain = res
    if mode == "col_mvp":
        r = dp.temporal_candidates()
        line = f"  units {len(dp.pus)}  derivations {r.size}  candidates available {int(r['available'].sum())}"
        if plain is not None:
            line += f"  search records that differ from col alone {int(sum(a.tobytes() != b.tobytes() for a, b in zip(res, plain)))} of {len(res)}"
        print(line, flush=True)
    del dp
