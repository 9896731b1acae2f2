"""One-picture step time of DecisionPicture at 1080p 8-bit by default, with tree_rates + pu_modes + cu_close + cqt, and with unit_trees on top (median of 10 steps
after 3 warm-up steps; every step's time is printed, so that the series can be written down).  A tree without an option (the parent commit) is timed on what it
has: run this script alternately from both trees on the same box to set the default step beside the parent's, and take the parent's own run-to-run spread from its
repeated runs.
python profiles/r07/unit_trees_step_time.py [mode ...]  (from the repository root; modes: default cqt unit; unit_trees_figures.txt holds the result)"""
import inspect, os, sys, time, statistics
sys.path.insert(0, os.getcwd())
from turingcodec_amd.havoc import Havoc
from turingcodec_amd.decisions import DecisionPicture
hv = Havoc(stream="new")
have = inspect.signature(DecisionPicture.__init__).parameters
cqt = {"tree_rates": True, "pu_modes": True, "cu_close": True, "cqt": True}
options = {"default": {}, "cqt": cqt, "unit": dict(cqt, unit_trees=True)}
for mode in (sys.argv[1:] or ["default", "cqt", "unit"]):
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
    if mode == "unit":
        q, rec = dp.cqt_decisions, dp.cu_decisions["records"]
        nodes = q["nodes"]
        both = ((nodes["choice"] == 1) | (nodes["choice"] == 2)) & (nodes["cost_full"] != -1) & (nodes["cost_split"] != -1)
        print(f"  searched units {len(dp.pus)}  refused {int((rec['outcome'] < 0).sum())}  CTUs decided {int(q['ctus']['decided'].sum())} of {len(q['ctus'])}  "
              f"coding units {int(q['ctus']['n_cus'].sum())}  comparisons {int(both.sum())}: the unit stood {int((both & (nodes['choice'] == 1)).sum())}, "
              f"the split won {int((both & (nodes['choice'] == 2)).sum())}", flush=True)
    del dp
