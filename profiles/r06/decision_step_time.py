"""One-picture step time of DecisionPicture at 1080p 8-bit with and without sao=True (median of 10 steps after 3 warm-up steps).
python profiles/r06/decision_step_time.py  (from the repository root; decision_step_time.txt holds the result)"""
import os, sys, time, statistics
sys.path.insert(0, os.getcwd())
from turingcodec_amd.havoc import Havoc
from turingcodec_amd.decisions import DecisionPicture
hv = Havoc(stream="new")
for sao in (False, True):
    dp = DecisionPicture(hv, 1920, 1080, 8, 32, seed=5, sao=sao)
    for _ in range(3):
        dp.step()
    t = []
    for _ in range(10):
        t0 = time.perf_counter()
        dp.step()
        t.append((time.perf_counter() - t0) * 1e3)
    print(f"1920x1080 8-bit DecisionPicture.step() sao={sao}: median {statistics.median(t):.2f} ms  min {min(t):.2f}  max {max(t):.2f}")
