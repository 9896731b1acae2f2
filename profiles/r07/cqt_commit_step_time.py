"""One-picture step time of DecisionPicture at 1080p 8-bit by default, with tree_rates + pu_modes + cu_close + cqt + unit_trees, and with commit on top (median of 10
steps after 3 warm-up steps; every step's time is printed, so that the series can be written down).  A tree without an option (the parent commit) is timed on what it
has: run this script alternately from both trees on the same box to set the default step beside the parent's, and take the parent's own run-to-run spread from its
repeated runs.
python profiles/r07/cqt_commit_step_time.py [mode ...]  (from the repository root; modes: default unit commit; cqt_commit_figures.txt holds the result)"""
import collections, inspect, os, sys, time, statistics
sys.path.insert(0, os.getcwd())
from turingcodec_amd.havoc import Havoc
from turingcodec_amd.decisions import DecisionPicture
hv = Havoc(stream="new")
have = inspect.signature(DecisionPicture.__init__).parameters
unit = {"tree_rates": True, "pu_modes": True, "cu_close": True, "cqt": True, "unit_trees": True}
options = {"default": {}, "unit": unit, "commit": dict(unit, commit=True)}
for mode in (sys.argv[1:] or ["default", "unit", "commit"]):
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
    if mode == "commit":
        cells, q = dp.cqt_commit_results()["cells"], dp.cqt_decisions
        units = sorted(set(cells["unit"].ravel().tolist()) - {-1})
        by = collections.Counter((int(dp.cu_decisions["records"]["outcome"][p]), int(dp.unit_plan["units"]["log2_size"][p])) for p in units)
        print(f"  searched units {len(dp.pus)}  CTUs decided {int(q['ctus']['decided'].sum())} of {len(q['ctus'])}  committed units {len(units)} "
              f"(coding units {int(q['ctus']['n_cus'].sum())})  cells without a unit {int((cells['unit'] < 0).sum())} of {cells.size}  "
              f"(outcome, log2 size): count {dict(sorted(by.items()))}", flush=True)
    del dp
