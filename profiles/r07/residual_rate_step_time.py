"""One-picture step time of DecisionPicture at 1080p 8-bit with and without residual_rates=True (median of 10 steps after 3 warm-up steps), twice over so that the
spread between repeated runs shows.  A tree without the option (the parent commit) is timed on its default step alone.
python profiles/r07/residual_rate_step_time.py  (from the repository root; residual_rate_figures.txt holds the result)"""
import inspect, os, sys, time, statistics
sys.path.insert(0, os.getcwd())
from turingcodec_amd.havoc import Havoc
from turingcodec_amd.decisions import DecisionPicture
hv = Havoc(stream="new")
has = "residual_rates" in inspect.signature(DecisionPicture.__init__).parameters
for run in range(2):
    for rated in ((False, True) if has else (False,)):
        dp = DecisionPicture(hv, 1920, 1080, 8, 32, seed=5, **({"residual_rates": True} if rated else {}))
        for _ in range(3):
            dp.step()
        t = []
        for _ in range(10):
            t0 = time.perf_counter()
            dp.step()
            t.append((time.perf_counter() - t0) * 1e3)
        print(f"run {run}: 1920x1080 8-bit DecisionPicture.step() residual_rates={rated}: median {statistics.median(t):.2f} ms  min {min(t):.2f}  max {max(t):.2f}", flush=True)
        del dp
