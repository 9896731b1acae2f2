"""havoc_search_intra_device with and without rates="cabac" on the intra partitions of one 1080p 8-bit picture at the measured call mix (workload.intra_partitions:
about 25 k partitions, 59 % of them 4x4), QP 32.
  python profiles/r07/intra_rate_prof.py time          seconds_gpu of both routes: median of 10 calls after 3, three times over
  python profiles/r07/intra_rate_prof.py cabac [N]     N calls (default 3) of the rated route alone, for a profiler:
  python profiles/r07/intra_rate_prof.py stand-in [N]      rocprofv3 --kernel-trace --stats ... -- python ... cabac ; counters (--pmc SQ_INSTS_VALU) in a run of their own
(from the repository root; intra_rate_figures.txt holds the result)"""
import os, statistics, sys
import numpy as np
sys.path.insert(0, os.getcwd())
from turingcodec_amd import decisions, workload
from turingcodec_amd.havoc import Havoc

W, H, BD, QP, PAD = 1920, 1080, 8, 32, 96
hv = Havoc(stream="new")
src2d = workload.pad_plane(workload.synth_frames(W, H, 1, 5, BD)[0][0], PAD)
stride = src2d.shape[1]
d_src = hv.up(np.ascontiguousarray(src2d.ravel()))
rng = np.random.default_rng(7)
nctu = ((W + 63) // 64) * ((H + 63) // 64)
base = rng.integers(4, 100, 128 + 4)
states = np.clip(base[None, :] + rng.integers(-6, 7, (nctu, 132)), 0, 125).astype(np.uint8)
d_states, d_syntax = hv.up(np.ascontiguousarray(states[:, :128]).reshape(-1)), hv.up(np.ascontiguousarray(states[:, 128:]).reshape(-1))
lam = workload.picture_lambda(QP)
groups = []
for log2, (jobs, nb, ictx, ctu) in sorted(workload.intra_partitions(src2d, W, H, PAD, 36).items(), reverse=True):
    keep = (hv.up(jobs), hv.up(nb), hv.up(np.ascontiguousarray(ictx).view(np.int32)), hv.up(np.ascontiguousarray(ctu, np.int32)), hv.zeros(len(jobs) << (2 * log2), np.uint8))
    groups.append(dict(log2=log2, n=len(jobs), d_nb=keep[1].data_ptr(), d_jobs=keep[0].data_ptr(), d_ictx=keep[2].data_ptr(), d_ctu=keep[3].data_ptr(), d_rec=keep[4].data_ptr(),
                       keep=keep))
args = (hv.h, 1, BD, d_src.data_ptr(), stride, groups, d_states.data_ptr(), decisions.rqt_quant(QP, BD), float(1.0 / np.sqrt(lam)), lam, 1.0 / lam)


def call(rated):
    return decisions.intra_device(*args, **(dict(rates="cabac", d_syntax_states=d_syntax.data_ptr()) if rated else {}))


what = sys.argv[1] if len(sys.argv) > 1 else "time"
if what == "time":
    print("partitions per size", {g["log2"]: g["n"] for g in groups}, flush=True)
    for run in range(3):
        for rated in (False, True):
            for _ in range(3):
                call(rated)
            t, st = [], None
            for _ in range(10):
                _, st = call(rated)
                t.append(st.seconds_gpu * 1e3)
            print(f"run {run}: havoc_search_intra_device{'_rated' if rated else ''}: seconds_gpu median {statistics.median(t):.3f} ms  min {min(t):.3f}  max {max(t):.3f}  "
                  f"({st.candidates} candidates, {st.launches} launches)", flush=True)
else:
    for _ in range(int(sys.argv[2]) if len(sys.argv) > 2 else 3):
        call(what == "cabac")
    hv.sync()
