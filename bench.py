#!/usr/bin/env python3
"""bench.py -- hot-path throughput of the havoc primitive layer on MI355X.

One "step" = one random-access B-frame's worth of havoc primitive calls (turingcodec_amd/workload.py: the call
counts the reference encoder issues per 1920x1080 B-frame at QP32 speed=medium), evaluated
by the batch kernels of libhavoc_mi355x.so with every operand already resident in HBM.  value = frames per second.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--res 1920x1080] [--bit-depth 8] [--dump-outputs DIR] [--full]

The timed region is exactly K steps after W warm-up steps (`ms_per_step` = its time / K; --min-seconds repeats it); --dump-outputs writes what
the last of them computed.  A plain run does only that: set up, warm up, time, dump, print the line.  --full also measures and checks everything
around the headline: per-kernel times and the roofline (with counter passes of their own), the 4K and 10-bit configurations, the step without
RDOQ, the one-picture latency, the decision-driven path, the CPU baselines and the parity check against the reference library.

N > 1 is launched by the driver through torch.distributed.run (one rank per GPU, RCCL): frames are sharded across
ranks (each rank works on its own picture: weak scaling) and after every step the ranks holding reference pictures
broadcast their reconstructed planes to all others (turingcodec_amd/frame_parallel.py), as the frame-parallel
encoder must.  Rank 0 prints ONE JSON line.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# HIP maps streams onto 4 hardware queues unless told otherwise: with more independent pictures in flight than queues, their kernels (the
# one-launch-per-picture search above all) queue up behind each other.  Must be in the environment before the runtime starts, so the
# decision-driven path is measured in a process of its own (`--decisions 2`, started by a --full run) with 16 queues; the primitive-batch
# step keeps the runtime's default (its 8 lanes are branches of one HIP graph; measured slower with 16 queues: 0.62 against 0.49 ms).
if "--decisions" in sys.argv[:-1] and sys.argv[sys.argv.index("--decisions") + 1] in ("2", "4"):
    # (--vr-bands: three streams per picture context, and what WAITS on a stream must never sit in a hardware queue in front of what it waits for)
    # -- measured (gpu calls r05ad): 24 queues 82 pictures/s, 28: 80, 32: 68, 40: 53, 48: 47 with eight contexts; the device has about that many real queues)
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "24" if "--vr-bands" in sys.argv else "16")

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (guides/MI355X_MICROARCH.md); ~6300 GB/s achievable
# vector-instruction issue peak: 256 CUs x 4 SIMD-32 per CU, a wave64 VALU instruction issues over 2 cycles (MI355X_MICROARCH.md "Each CU has 4 SIMD-32 units ...
# issues each VALU instruction over 2 cycles"), 2.4 GHz: wavefront-level instructions per second, in G
VALU_PEAK_GINST = 256 * 4 * 2.4 / 2


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--res", default="1920x1080")
    ap.add_argument("--bit-depth", type=int, default=8)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--yuv", default=None, help="raw planar 4:2:0 file of --res / --bit-depth (the reference's input format): its first three "
                    "frames replace the synthetic clip as L0 reference / current picture / L1 reference (`data` then says so)")
    ap.add_argument("--rdoq", type=int, default=1, help="random-access mix: 1 = Rdoq::runQuantisation on the device between tu_forward and "
                    "tu_reconstruct (speed=medium has RDOQ on); 0 = round 1's step: levels made once, untimed, by havoc_quantize")
    ap.add_argument("--qp", type=int, default=32, help="slice QP: the (de)quantiser scale / shift of the TU chain (turing/QpState.h:85-94)")
    ap.add_argument("--mix", choices=["ra", "ai"], default="ra",
                    help="call mix: one random-access B-frame at speed=medium (default) or one all-intra frame at speed=fast "
                         "(BASELINE.json configs[0]: intra + TU chain with havoc_quantize in it)")
    ap.add_argument("--min-seconds", type=float, default=None,
                    help="repeat the K-step timed block until this much time has been measured and report the median block (default: ONE block, "
                         "so that --steps is the number of timed steps); 0 = one block and no counter passes (runs under a profiler)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write every result buffer of the last timed step's picture as DIR/<name>.npy (float32 for 8- / 16-bit "
                         "results, float64 for 32-bit ones; buffers above a per-buffer share of 64 MB as a fixed seeded sample of their elements)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure and check everything around the headline (see the top of this file): the options "
                         "--extra-4k, --decisions 1, --traffic, --kernel-reps and --no-cpu-baseline shape what it adds; without --full the run "
                         "prints the headline alone")
    ap.add_argument("--extra-4k", type=int, default=1,
                    help="with --full: also measure the 3840x2160 8-bit QP27 workload (BASELINE.json configs[2]) for a few steps and report it under "
                         "`extra` (N=1 only; 0 = off)")
    ap.add_argument("--bands", type=int, default=0, help="frame-parallel runs: exchange the reference pictures in bands of this many CTU rows (turingcodec_amd/"
                    "frame_parallel.py: BandPlan; 0 = one broadcast per picture)")
    ap.add_argument("--decisions", type=int, default=1,
                    help="1 (default): with --full, the N=1 line also carries, under `extra`, the DECISION-DRIVEN path (turingcodec_amd.decisions."
                         "DecisionPicture: motion searches in WPP wavefront order with predictors derived from earlier decisions, batch-fed; then the "
                         "TU chain on the chosen vectors) at 1080p QP32 and 4K QP32, and its ratio to `value`; 2: only that (diagnostic line); 0: off")
    ap.add_argument("--vr-bands", type=int, default=0, help="--decisions 4: CTU rows per band -- a picture's reconstruction enters the mirror band by band while its lower rows "
                    "are still searched (DecisionPicture.step_banded) and the pictures predicting from it follow it down the picture (havoc_mi355x_search_gate); 0 = whole pictures")
    ap.add_argument("--vr-no-intra", type=int, default=0, help="--decisions 4: 1 = contexts without the intra candidates (what --vr-issue single runs: the like-for-like whole-picture figure)")
    ap.add_argument("--vr-issue", default="single", choices=("single", "threads"),
                    help="--vr-bands: who queues the work -- ONE thread for the whole sequence (every dependency is an event or a device counter; the contexts then leave the "
                         "intra candidates out: their call is synchronous) or a thread per context")
    ap.add_argument("--vr-dataflow", type=int, default=1, help="--decisions 4: 1 = a picture starts when its references are in the mirror (default); 0 = a barrier between the slots")
    ap.add_argument("--virtual-ranks", type=int, default=8, help="--decisions 4: contexts / host threads that execute the frame-parallel schedule on ONE GPU")
    ap.add_argument("--decision-pictures", type=int, default=16, help="contexts built for the decision-driven path: `value` is measured with 4 independent pictures in flight (the "
                    "leaf B pictures of one SOP), and again with 8 (what the pipelined hierarchy has in flight) and with all of them; one host thread + "
                    "context each")
    ap.add_argument("--traffic", type=int, default=1, help="1 (default): a --full N=1 run measures roofline.traffic itself with two rocprofv3 --pmc passes "
                    "of a two-step run (when rocprofv3 is on PATH); 0: take it from the committed profiles/r*_hbm_traffic.csv")
    ap.add_argument("--traffic-child", type=int, default=0, help=argparse.SUPPRESS)      # the counter passes' child: exactly this many steps, eagerly, then exit
    ap.add_argument("--decision-distance", type=int, default=1, help="with --decisions 2: temporal distance of the decision-driven picture's two references "
                    "(1 = a leaf B picture of the hierarchy; 2, 4, 8 = its upper layers: longer vectors, 2.5 - 3 x the calls per search)")
    ap.add_argument("--decision-walk", type=int, default=0, help="with --decisions 2: also time the same walk through the reference's tables on one host core "
                    "and compare every decision (the cpu_baseline leg of a --full run)")
    ap.add_argument("--search-client", choices=["device", "batch"], default="device",
                    help="the motion searches of the decision-driven path: `device` = the decision loops inside the kernel (csrc/kernels_search.hip, one launch "
                         "per picture); `batch` = SAD-surface / tile-SATD launches + the loops replayed on host threads (search/picture_search.cpp)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baselines and the parity check against the reference library")
    ap.add_argument("--detail-out", default=os.path.join(ROOT, "gpurun_out", "bench_detail.json"),
                    help="the FULL result (every `what` / `note` string, per-distance decision-path detail, per-kernel tables) goes to this file; the ONE JSON "
                         "line on stdout stays below 8 KB (the driver keeps 8 KB of it: VERDICT r4 next #1c)")
    ap.add_argument("--parity-dump", default=os.path.join(ROOT, "gpurun_out", "bench_parity_mismatches.json"),
                    help="where a failed full-size parity check writes which values differed (group, job, sample, both values, lane plan)")
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying a HIP graph")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="target CPU time of the cpu_baseline sample")
    ap.add_argument("--cpu-worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--cpu-out", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--kernel-reps", type=int, default=5, help="with --full: launches averaged per launch group for the per-kernel times of the roofline")
    ap.add_argument("--sad4", choices=["runs", "calls"], default="runs",
                    help="the 4-way SAD jobs: by runs (default; havoc_mi355x_sad4_runs: the ~112 consecutive calls of a search share one staged window, round 5) "
                         "or one window per call (havoc_mi355x_sad4, round 4's k_sad4w)")
    ap.add_argument("--ime", choices=["sad4", "surface"], default="sad4",
                    help="integer ME as per-pattern SAD4 jobs (the reference's call mix) or as one SAD surface per search")
    ap.add_argument("--ime-range", type=int, default=16, help="surface half-width R: (2R+1)^2 candidates per search")
    ap.add_argument("--inflight", type=int, default=2,
                    help="pictures in flight per GPU: independent pictures (the B pictures of one hierarchy level) alternate on "
                         "separate streams so that one picture's tail overlaps the next one's head")
    ap.add_argument("--tune", type=int, default=24, help="lane assignments tried by the set-up planner (0: round-robin)")
    ap.add_argument("--pcie", action="store_true",
                    help="diagnostic: every step also moves the frame's host traffic over PCIe (source picture, job tables and "
                         "quantised levels up; costs and coefficients down) -- the PCIe-inclusive rate of DESIGN.md, never the metric")
    ap.add_argument("--skip", default="", help="diagnostic: comma-separated launch groups to leave out (the result is then "
                                               "NOT the metric; the JSON line says so)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="N > 1: weak = steady state of an endless sequence (one picture per rank per slot); strong = a fixed sequence "
                         "of --pictures pictures from first to last slot, pipeline fill and drain included")
    ap.add_argument("--pictures", type=int, default=33, help="--scaling strong: sequence length (IDR + SOPs of 8; SURVEY 8(d): 33)")
    ap.add_argument("--lag", type=int, default=0, help="frame-parallel schedule: slots between a picture and the references it gets from "
                    "other ranks (0 = DagSchedule's default: 2 for 8+ ranks on an endless sequence, else 1)")
    ap.add_argument("--poc-checksums", action="store_true",
                    help="frame-parallel verification: synchronise after every picture and report a checksum of its reconstruction per POC")
    ap.add_argument("--exchange", action="store_true",
                    help="run the reference-picture exchange (process group + RCCL broadcasts) even with one rank")
    ap.add_argument("--lanes", type=int, default=8, help="fork/join lanes: independent launch chains overlap on the GPU")
    ap.add_argument("--tu", choices=["fused", "split"], default="fused",
                    help="TU chain: two fused kernels around the host quantiser (default) or the five separate primitives")
    ap.add_argument("--pred", choices=["merged", "classes"], default="merged",
                    help="prediction launches: all size classes of a table in one launch (default) or one launch per width class")
    ap.add_argument("--separate-scan", action="store_true", help="diagnostic: RDOQ's scan pass as its own kernel (round 2) instead of inside tu_forward")
    ap.add_argument("--subpel", choices=["planes", "fused"], default="planes",
                    help="sub-pel candidates: SATD against per-picture phase planes (default) or the fused per-candidate kernel")
    return ap.parse_args()


# --------------------------------------------------------------------------------------------------------------
# device side
# --------------------------------------------------------------------------------------------------------------

from turingcodec_amd.step import DeviceFrame, FramePipeline      # noqa: E402  (round 6: the step's orchestration lives in the package)


# --------------------------------------------------------------------------------------------------------------
# CPU baseline: the reference's own havoc functions (oracle/_ref, x86 JIT tables) on a bounded sample of the same
# job tables, all host cores.  Runs in a worker process so that a SIMD alignment fault cannot take the bench down.
# --------------------------------------------------------------------------------------------------------------

def _aligned(a, align=64):
    a = np.ascontiguousarray(a)
    raw = np.empty(a.nbytes + align, np.uint8)
    o = (-raw.ctypes.data) % align
    out = raw[o:o + a.nbytes].view(a.dtype).reshape(a.shape)
    out[...] = a
    return out


def usable_cores():
    """host threads we may really use: CPU affinity capped by the cgroup CPU quota"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(quota) // int(period)))
    except Exception:
        pass
    return max(1, n)


def cpu_worker(args):
    """child process: time the reference library on every `stride`-th job; prints a JSON dict"""
    import ctypes as C
    from concurrent.futures import ThreadPoolExecutor
    from turingcodec_amd.workload import FrameWorkload
    handle, stride = (int(v) for v in args.cpu_worker.split(","))
    w, h = (int(v) for v in args.res.split("x"))
    frames = None
    if getattr(args, "yuv", None):
        from turingcodec_amd.picture_io import YuvReader
        rd = YuvReader(args.yuv, w, h, args.bit_depth)
        frames = [rd.planes(i % max(1, len(rd))) for i in range(3)]
    wl = FrameWorkload(w, h, args.bit_depth, args.seed, qp=args.qp, mix=args.mix, frames=frames)
    inter = wl.mix == "ra"
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libhavoc_ref.so"))
    cores = usable_cores()
    lib.ref_mask(handle)   # populate the function tables (JIT assembly) once, before any worker thread touches them
    S, bd, st, cst = wl.S, wl.bit_depth, wl.stride, wl.cstride
    dt = wl.dtype
    P = lambda a: C.c_void_p(a.ctypes.data)
    ip = C.c_ssize_t
    sub = lambda j: _aligned(np.ascontiguousarray(j[::stride]))

    luma = _aligned(np.concatenate([wl.luma, np.zeros(wl.plane_len, dt)]))
    chroma = _aligned(wl.chroma)
    pred = _aligned(np.zeros(wl.pred_len + 4096, dt))
    cpred = _aligned(np.zeros(wl.cpred_len + 1024, dt))
    bi = _aligned(np.zeros(wl.bi_len + 8192, dt))
    cbi = _aligned(np.zeros(len(wl.bi4) * 1024 + 2048, dt))
    sbi = _aligned(np.zeros(len(wl.subtract_bi) * 4096 + 4096, dt))
    tasks = []   # (callable(b, e), njobs, group the GPU bench times it under)
    results = {}   # name -> array: what the reference computed for the sampled jobs (full-size parity check in main)

    def add(group, fn, n, always=False, like=None):
        """`like`: cut this task's jobs into the thread slices of a table of that length -- for a task whose job i reads what job i of an earlier task wrote"""
        if n and (inter or always):
            tasks.append((fn, n, group, like or n))
            if os.environ.get("HAVOC_BENCH_TRACE"):
                sys.stderr.write(f"task {len(tasks)} n={n}\n")
                sys.stderr.flush()
                fn(0, n)

    j4, js = sub(wl.sad4), sub(wl.sad)
    o4, os_ = np.zeros(4 * len(j4), np.int32), np.zeros(len(js), np.int32)
    add("sad4", lambda b, e: lib.ref_run_sad4(handle, S, P(luma), ip(st), P(luma), ip(st), P(j4), b, e, P(o4)), len(j4))
    add("sad", lambda b, e: lib.ref_run_sad(handle, S, P(luma), ip(st), P(luma), ip(st), P(js), b, e, P(os_)), len(js))
    ju8, ju4, jb8, jb4, jsb, jsa = sub(wl.uni8), sub(wl.uni4), sub(wl.bi8), sub(wl.bi4), sub(wl.subtract_bi), sub(wl.satd_inter)
    osa = np.zeros(len(jsa), np.int32)
    add("pred_uni8", lambda b, e: lib.ref_run_pred_uni(handle, S, 8, bd, P(pred), ip(64), P(luma), ip(st), P(ju8), b, e), len(ju8))
    add("satd_inter", lambda b, e: lib.ref_run_satd(handle, S, P(luma), ip(st), P(pred), ip(64), P(jsa), b, e, P(osa)), len(jsa))
    add("pred_uni4", lambda b, e: lib.ref_run_pred_uni(handle, S, 4, bd, P(cpred), ip(32), P(chroma), ip(cst), P(ju4), b, e), len(ju4))
    add("pred_bi8", lambda b, e: lib.ref_run_pred_bi(handle, S, 8, bd, P(bi), ip(64), P(luma), ip(st), P(jb8), b, e), len(jb8))
    # SubtractBi job i reads the bi-prediction slot job i of pred_bi8 wrote, and that table is longer: sliced like IT, so that a thread reads only slots it has itself
    # finished.  (Sliced by its own length -- rounds 1-4 -- another thread could be REWRITING the slot meanwhile: the reference's JIT stores 16 bytes per 8 samples it
    # computes (PRED_BI_V_8NxH: packuswb m3, m3; movdqu [dst], m3 -- havoc/pred_inter.cpp:880-882), so columns x + 8 .. x + 15 of a row briefly hold a copy of columns
    # x .. x + 7 -- the "17 subtract_bi values" of round 4's driver run, caught again and located in round 5: NOTEBOOK.md.)
    add("subtract_bi", lambda b, e: lib.ref_run_subtract_bi(handle, S, bd, P(sbi), ip(64), P(bi), ip(64), P(luma), ip(st), P(jsb), b, e), len(jsb), like=len(jb8))
    add("pred_bi4", lambda b, e: lib.ref_run_pred_bi(handle, S, 4, bd, P(cbi), ip(32), P(chroma), ip(cst), P(jb4), b, e), len(jb4))
    keep = [j4, js, ju8, ju4, jb8, jb4, jsb, jsa, o4, os_, osa]
    late = []
    if inter:
        results.update(sad4=o4, sad=os_, satd_inter=osa)
        # (name, slot buffer, jobs, column of the slot offset, column of w, slot stride): block regions cut out after the run
        late = [("pred_uni8", pred, ju8, 0, 2, 64), ("pred_uni4", cpred, ju4, 0, 2, 32), ("pred_bi8", bi, jb8, 0, 3, 64),
                ("pred_bi4", cbi, jb4, 0, 3, 32), ("subtract_bi", sbi, jsb, 0, 3, 64)]
    for hi, j in wl.subpel.items():   # fused on the GPU; on the CPU the reference's two calls: pred_uni, then measureSatd
        if not len(j) or not inter:
            continue
        jp = sub(j)
        jsat = _aligned(np.stack([jp[:, 0], np.arange(len(jp), dtype=np.int32) * 4096, jp[:, 2], jp[:, 3]], 1).astype(np.int32))
        jp[:, 0] = np.arange(len(jp)) * 4096
        scratch = _aligned(np.zeros(len(jp) * 4096 + 4096, dt))
        osp = np.zeros(len(jp), np.int32)
        keep += [jp, jsat, scratch, osp]
        results[f"subpel_{hi}"] = osp
        add("subpel(interp+satd)", lambda b, e, jp=jp, scratch=scratch: lib.ref_run_pred_uni(handle, S, 8, bd, P(scratch), ip(64), P(luma), ip(st), P(jp), b, e), len(jp))
        add("subpel(interp+satd)", lambda b, e, jsat=jsat, scratch=scratch, osp=osp: lib.ref_run_satd(handle, S, P(luma), ip(st), P(scratch), ip(64), P(jsat), b, e, P(osp)), len(jp))
    for log2, j in wl.intra.items():
        if not len(j):
            continue
        n = 1 << log2
        ji, nb = sub(j), _aligned(wl.intra_nb[log2])
        dst = _aligned(np.zeros((len(j) << (2 * log2)) + 64, dt))
        keep += [ji, nb, dst]
        results[f"intra_{log2}"] = (dst, ji[:, 0], n * n)
        add("intra", lambda b, e, log2=log2, n=n, ji=ji, nb=nb, dst=dst: lib.ref_run_intra(handle, S, bd, log2, P(dst), ip(n), P(nb), P(ji), b, e), len(ji), True)
    for log2, j in wl.intra_search.items():
        if not len(j):
            continue
        jp, nb = sub(j), _aligned(wl.intra_search_nb[log2])
        cost = np.zeros(35 * len(jp), np.int32)
        keep += [jp, nb, cost]
        results[f"intra35_{log2}"] = cost
        add("intra_satd35", lambda b, e, log2=log2, jp=jp, nb=nb, cost=cost: lib.ref_run_intra_satd35(handle, S, bd, log2, P(luma), ip(st), P(nb), P(jp), b, e, P(cost)), len(jp), True)
    from turingcodec_amd.workload import quant_params, dequant_params
    qp = wl.qp
    prepass = []   # untimed: the levels the timed de-quantiser reads (at medium the reference's RDOQ makes them on the host)
    for (log2, tr), g in wl.tu.items():
        m = len(g["jobs"])
        if not m:
            continue
        n = g["n"]
        jt, jsrc, roff = sub(g["jobs"]), sub(g["src"]), sub(g["res_off"])
        res = _aligned(np.zeros(m * n * n + 64, np.int16))
        coef = _aligned(np.zeros(m * n * n + 64, np.int16))
        deq = _aligned(np.zeros(m * n * n + 64, np.int16))
        level = _aligned(np.zeros(m * n * n + 64, np.int16))
        cbf = np.zeros(len(jt), np.int32)
        qj = np.zeros((len(jt), 8), np.int32)
        qj[:, 0] = qj[:, 1] = jt[:, 0]
        qj[:, 2] = n * n
        qj[:, 3], qj[:, 4], qj[:, 5] = quant_params(qp, log2, bd, not inter)
        dj = qj.copy()
        dj[:, 3], dj[:, 4] = dequant_params(qp, log2, bd)
        dj[:, 5] = 0
        qj, dj = _aligned(qj), _aligned(dj)
        keep += [jt, jsrc, roff, res, coef, deq, level, cbf, qj, dj]
        results[f"coef_{log2}_{tr}"] = (coef, jt[:, 0], n * n)
        results[f"level_{log2}_{tr}"] = (level, jt[:, 0], n * n)
        f_res = lambda b, e, n=n, res=res, roff=roff, jsrc=jsrc: lib.ref_run_residual(S, P(res), ip(n), P(roff), P(luma), ip(st), P(luma), ip(st), P(jsrc), b, e)
        f_fwd = lambda b, e, n=n, log2=log2, tr=tr, coef=coef, res=res, jt=jt: lib.ref_run_transform(handle, bd, tr, log2, P(coef), P(res), ip(n), P(jt), b, e)
        f_q = lambda b, e, level=level, coef=coef, qj=qj, cbf=cbf: lib.ref_run_quantize(handle, P(level), P(coef), P(qj), b, e, P(cbf))
        add("tu_forward", f_res, len(jt), True)
        add("tu_forward", f_fwd, len(jt), True)
        if inter and args.rdoq:   # speed=medium: the reference's own Rdoq::runQuantisation (turing/Rdoq.cpp, oracle/ref_shim_rdoq.cpp)
            rj = _aligned(wl.rdoq_jobs((log2, tr))[::stride].copy().view(np.uint8))
            rstates = _aligned(wl.rdoq_states)
            keep += [rj, rstates]
            results[f"cbf_{log2}_{tr}"] = cbf
            add("rdoq", lambda b, e, log2=log2, level=level, coef=coef, rj=rj, rstates=rstates, cbf=cbf: lib.ref_run_rdoq(
                bd, log2, P(level), P(coef), P(rstates), P(rj), C.c_double(wl.rdoq_lambda), b, e, P(cbf)), len(jt), True)
        elif inter:
            prepass.append((len(jt), f_res, f_fwd, f_q))
        else:   # speed=fast: havoc_quantize is in the timed chain (turing/Reconstruct.cpp:310-311)
            add("quantize", f_q, len(jt), True)
        add("tu_reconstruct", lambda b, e, deq=deq, level=level, dj=dj: lib.ref_run_quantize_inverse(handle, P(deq), P(level), P(dj), b, e), len(jt), True)
        rec = _aligned(np.zeros(m * n * n + 64, dt))
        # the SSD table = [one job per TU | the reference's extra ~0.26 calls per TU]: the per-TU part is sampled like the TU
        # tables (same length -> same thread slice -> it reads a reconstruction the SAME thread has just finished); the extra
        # calls re-read reconstructions other threads may be rewriting at that moment (the x86 inverse transform uses its
        # destination as scratch), so they are timed but not part of the parity check
        jss, jsx = sub(g["ssd"][:m]), sub(g["ssd"][m:]) if len(g["ssd"]) > m else np.zeros((0, 4), np.int32)
        oss, osx = np.zeros(len(jss), np.uint32), np.zeros(max(1, len(jsx)), np.uint32)
        keep += [rec, jss, oss, jsx, osx]
        results[f"rec_{log2}_{tr}"] = (rec, jt[:, 3], n * n)
        results[f"ssd_{log2}_{tr}"] = oss
        add("tu_reconstruct", lambda b, e, log2=log2, tr=tr, deq=deq, jt=jt, rec=rec, n=n: lib.ref_run_inverse_transform_add(handle, S, bd, tr, log2, P(rec), ip(n), P(luma), ip(st), P(deq), P(jt), b, e), len(jt), True)
        add("tu_reconstruct", lambda b, e, rec=rec, n=n, jss=jss, oss=oss: lib.ref_run_ssd(handle, S, P(luma), ip(st), P(rec), ip(n), P(jss), b, e, P(oss)), len(jss), True)
        add("tu_reconstruct", lambda b, e, rec=rec, n=n, jsx=jsx, osx=osx: lib.ref_run_ssd(handle, S, P(luma), ip(st), P(rec), ip(n), P(jsx), b, e, P(osx)), len(jsx), True)
    for nj, f_res, f_fwd, f_q in prepass:
        f_res(0, nj)
        f_fwd(0, nj)
        f_q(0, nj)

    group_s = {}
    acc = [dict() for _ in range(cores)]

    def run_slice(k, record):
        """thread k runs its contiguous slice of EVERY task in order: a chain's later primitives read what the same
        thread's earlier ones wrote, so no barrier between tasks is needed (and none is timed)"""
        for fn, n, group, like in tasks:
            chunk = (like + cores - 1) // cores
            b, e = min(n, k * chunk), min(n, (k + 1) * chunk)
            if b < e:
                t = time.perf_counter()
                fn(b, e)
                if record:
                    acc[k][group] = acc[k].get(group, 0.0) + time.perf_counter() - t

    def run_all(pool, record=False):
        list(pool.map(lambda k: run_slice(k, record), range(cores)))

    with ThreadPoolExecutor(cores) as pool:
        run_all(pool)   # warm (JIT assembly, page faults)
        t0 = time.perf_counter()
        reps = 0
        while True:
            run_all(pool, True)
            reps += 1
            if time.perf_counter() - t0 > 2.0 or reps >= 5000:
                break
        dt_s = (time.perf_counter() - t0) / reps
    if args.cpu_out:
        flat = {name: _regions(buf, jobs, oc, wc, sd) for name, buf, jobs, oc, wc, sd in late}
        for name, v in results.items():
            if isinstance(v, tuple):   # (buffer, block offsets, block length): keep only the sampled blocks
                buf, offs, ln = v
                flat[name] = buf[(offs.astype(np.int64)[:, None] + np.arange(ln)[None, :]).ravel()]
            else:
                flat[name] = v
        np.savez(args.cpu_out, **flat)
    print(json.dumps({"seconds_per_sample": dt_s, "stride": stride, "cores": cores, "handle": handle,
                      "jobs": int(sum(t[1] for t in tasks)), "reps": reps,
                      "group_seconds_per_sample": {g: sum(a.get(g, 0.0) for a in acc) / cores / reps for g in acc[0]}}))


def _regions(buf, jobs, ocol, wcol, stride):
    """concatenated w x h regions (row stride `stride`) at jobs[:, ocol] of a slot buffer"""
    buf = np.asarray(buf)
    out = []
    for j in np.asarray(jobs):
        o, w, h = int(j[ocol]), int(j[wcol]), int(j[wcol + 1])
        out.append(buf[o:o + stride * h].reshape(h, stride)[:, :w].ravel())
    return np.concatenate(out) if out else np.zeros(0, buf.dtype)


def parity_vs_reference(dev, path, stride, dump_path=None, lane_plan=None):
    """full-size parity: what the reference library computed for every `stride`-th job (the cpu_baseline sample) against
    the GPU's results for the same jobs; returns {"compared": values, "mismatches": values that differ, ...}.

    Any mismatch is located (group, job of the sampled table, sample inside the job's block, both values), the step is run once more EAGERLY on one stream
    and the group compared again (`mismatches_after_eager_rerun`: 0 there = the replayed graph left a wrong state, the kernels are right), and everything is
    written to `dump_path` and stderr.  main() turns a mismatch into `"parity": "red"` and a non-zero exit code (VERDICT r4 next #1a)."""
    hv, wl = dev.hv, dev.wl
    ref = np.load(path)
    compared = mismatches = 0
    groups = []
    by_group = {}
    getters = {}      # name -> (callable returning the GPU's values, locator(flat index) -> dict)
    located = {}

    def region_locator(jobs, ocol, wcol):
        jobs = np.asarray(jobs)
        ends = np.cumsum(jobs[:, wcol].astype(np.int64) * jobs[:, wcol + 1])

        def loc(i):
            k = int(np.searchsorted(ends, i, side="right"))
            r = int(i - (ends[k - 1] if k else 0))
            w = int(jobs[k, wcol])
            return {"sampled_job": k, "job_index": k * stride, "x": r % w, "y": r // w, "w": w, "h": int(jobs[k, wcol + 1]), "slot_offset": int(jobs[k, ocol]),
                    "job": [int(v) for v in jobs[k]]}
        return loc

    def block_locator(ln):
        return lambda i: {"sampled_job": int(i // ln), "job_index": int(i // ln) * stride, "sample_in_block": int(i % ln)}

    def row_locator(cols):
        return lambda i: {"sampled_job": int(i // cols), "job_index": int(i // cols) * stride, "column": int(i % cols)}

    def cmp(name, get, loc):
        nonlocal compared, mismatches
        a = np.asarray(ref[name]).astype(np.int64).ravel()
        b = np.asarray(get()).astype(np.int64).ravel()
        assert a.shape == b.shape, (name, a.shape, b.shape)
        compared += a.size
        idx = np.flatnonzero(a != b)
        mismatches += len(idx)
        if len(idx):
            by_group[name] = int(len(idx))
            getters[name] = (get, a)
            located[name] = [dict(loc(int(i)), flat_index=int(i), reference=int(a[i]), gpu=int(b[i])) for i in idx[:64]]
        groups.append(name)

    def blocks(buf, offs, ln):
        return buf[(np.asarray(offs, np.int64)[::stride][:, None] + np.arange(ln)[None, :]).ravel()]

    inter = wl.mix == "ra"
    if inter:
        if dev.ime_range is None:
            cmp("sad4", lambda: hv.down(dev.o_sad4, np.int32).reshape(-1, 4)[::stride], row_locator(4))
        cmp("sad", lambda: hv.down(dev.o_sad, np.int32)[::stride], row_locator(1))
        cmp("satd_inter", lambda: hv.down(dev.o_satd, np.int32)[::stride], row_locator(1))
        for name, buf, jobs, wcol, sd in (("pred_uni8", "pred", wl.uni8, 2, 64), ("pred_uni4", "cpred", wl.uni4, 2, 32), ("pred_bi8", "bi", wl.bi8, 3, 64),
                                          ("pred_bi4", "cbi", wl.bi4, 3, 32), ("subtract_bi", "sbi", wl.subtract_bi, 3, 64)):
            cmp(name, lambda buf=buf, jobs=jobs, wcol=wcol, sd=sd: _regions(hv.down(getattr(dev, buf), wl.dtype), jobs[::stride], 0, wcol, sd),
                region_locator(jobs[::stride], 0, wcol))
    if inter and dev.use_planes:
        n = sum(len(v) for v in wl.subpel_idx.values())

        def subpel_costs():
            ca = np.zeros(n, np.int32)
            for c, g in dev.subpel_planes.items():
                idx = wl.subpel_planes_idx[c].ravel()
                ca[idx[idx >= 0]] = hv.down(g["cost"], np.int32)[idx >= 0]
            return ca
        ca0 = subpel_costs()
        for hi, ids in wl.subpel_idx.items():
            if len(ids):
                cmp(f"subpel_{hi}", lambda ids=ids, first=[ca0]: (first.pop() if first else subpel_costs())[ids[::stride]], row_locator(1))
    for log2, g in dev.intra.items():
        n = 1 << log2
        cmp(f"intra_{log2}", lambda g=g, log2=log2, n=n: blocks(hv.down(g["dst"], wl.dtype), wl.intra[log2][:, 0], n * n), block_locator(n * n))
    for log2, g in dev.isearch.items():
        cmp(f"intra35_{log2}", lambda g=g: hv.down(g["cost"], np.int32).reshape(-1, 35)[::stride], row_locator(35))
    for (log2, tr), g in dev.tu.items():
        t = wl.tu[(log2, tr)]
        m, nn = len(t["jobs"]), g["n"] ** 2
        cmp(f"coef_{log2}_{tr}", lambda g=g, t=t, nn=nn: blocks(hv.down(g["coef"], np.int16), t["jobs"][:, 0], nn), block_locator(nn))
        cmp(f"level_{log2}_{tr}", lambda g=g, t=t, nn=nn: blocks(hv.down(g["level"], np.int16), t["jobs"][:, 0], nn), block_locator(nn))
        if dev.rdoq:
            cmp(f"cbf_{log2}_{tr}", lambda g=g: hv.down(g["cbf"], np.int32)[::stride], row_locator(1))
        cmp(f"rec_{log2}_{tr}", lambda g=g, t=t, nn=nn: blocks(hv.down(g["rec"], wl.dtype), t["jobs"][:, 3], nn), block_locator(nn))
        # the SSD tu_reconstruct reduced for each sampled TU (the extra plain-SSD calls are timed, not compared: see cpu_worker)
        cmp(f"ssd_{log2}_{tr}", lambda g=g, m=m: hv.down(g["ossd"], np.uint32)[:m][::stride], row_locator(1))
    out = {"compared": compared, "mismatches": mismatches, "mismatches_by_group": by_group, "groups": groups}
    if mismatches:
        # which side, and is it the replayed state or the kernels: one more step, eagerly, on ONE stream, then the same comparison of the groups that differed
        after = {}
        try:
            dev.step()
            hv.sync()
            for name, (get, a) in getters.items():
                after[name] = int((np.asarray(get()).astype(np.int64).ravel() != a).sum())
        except Exception as e:
            after = {"error": repr(e)}
        out["mismatches_after_eager_rerun"] = after
        report = {"mismatches_by_group": by_group, "mismatches_after_eager_rerun": after, "lane_plan": lane_plan, "first_mismatches": located,
                  "note": "reference = oracle/_ref (the reference's own havoc library) on every %dth job; gpu = the state the last replay of the step left" % stride}
        sys.stderr.write("PARITY RED: " + json.dumps(report)[:6000] + "\n")
        sys.stderr.flush()
        if dump_path:
            try:
                os.makedirs(os.path.dirname(os.path.abspath(dump_path)), exist_ok=True)
                with open(dump_path, "w") as f:
                    json.dump(report, f, indent=1)
                out["dump"] = os.path.relpath(dump_path, ROOT)
            except OSError:
                pass
        out["first_mismatch"] = {k: v[0] for k, v in located.items()}
    return out


def cpu_baseline(args, dev=None):
    """frames/s of the reference library on the host: sample = every `stride`-th job of every table"""
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libhavoc_ref.so")):
        return None
    import tempfile
    stride = 4
    for handle in (1, 0):   # x86 JIT tables first; plain-C tables if the JIT run fails
        tmp = os.path.join(tempfile.gettempdir(), f"havoc_cpu_{os.getpid()}_{handle}.npz")
        cmd = [sys.executable, os.path.abspath(__file__), "--cpu-worker", f"{handle},{stride}", "--res", args.res,
               "--bit-depth", str(args.bit_depth), "--seed", str(args.seed), "--qp", str(args.qp), "--mix", args.mix, "--rdoq", str(getattr(args, "rdoq", 1)),
               "--cpu-out", tmp] + (["--yuv", args.yuv] if getattr(args, "yuv", None) else [])
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if out.returncode == 0:
                r = json.loads(out.stdout.strip().splitlines()[-1])
                fps = 1.0 / (r["seconds_per_sample"] * r["stride"])
                res = {"value": round(fps, 3), "unit": "frames/s", "cores": r["cores"], "kind": "reference",
                       "ms_per_frame_by_group": {g: round(v * r["stride"] * 1e3, 3) for g, v in r["group_seconds_per_sample"].items()},
                       "what": "the reference's havoc primitive tables on the same job tables -- NOT SURVEY 8(d)'s `turing encode` (the full "
                               "encoder needs a CMake-generated header and is not built here, DESIGN.md 2)",
                       "sample": f"every {stride}th job of each primitive's job table ({r['jobs']} calls) through the "
                                 f"reference's own havoc {'x86-JIT' if handle else 'C'} function tables (oracle/_ref), "
                                 f"{r['cores']} host threads, the sample repeated {r['reps']}x "
                                 f"({r['reps'] * r['seconds_per_sample']:.1f} s wall, "
                                 f"{r['reps'] * r['seconds_per_sample'] * r['cores']:.0f} core-seconds), extrapolated x{stride}"}
                if dev is not None and os.path.exists(tmp):
                    try:
                        res["parity_vs_reference"] = parity_vs_reference(dev, tmp, stride, dump_path=getattr(args, "parity_dump", None),
                                                                         lane_plan=getattr(dev, "assign", None))
                    except Exception as e:   # a comparison that could not be made is not a green one: main() reports parity "red"
                        res["parity_vs_reference"] = {"error": repr(e)}
                return res
        except Exception:
            pass
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
    return None


# --------------------------------------------------------------------------------------------------------------

def hbm_traffic_from_profiles(group, S):
    """HBM bytes per launch of a launch group, from the committed PMC passes (profiles/rNN_hbm_traffic.csv: rocprofv3
    --pmc FETCH_SIZE / WRITE_SIZE in separate runs of this bench, FETCH_SIZE x2 per the gfx950 note of
    MI355X_MICROARCH.md; written by profiles/summarize.py).  None when there is no profile for the group's kernel or
    the kernel is shared with another group (k_satd)."""
    import csv
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_hbm_traffic.csv")))
    if not files:
        return None
    prefix = _kernel_prefix(group, S)
    if prefix is None:
        return None
    total, n = 0.0, 0
    for row in csv.DictReader(open(files[-1])):
        if _matches(prefix, row["Kernel"]):
            try:
                total += float(row.get("FETCH_SIZE_bytes_per_launch") or 0) + float(row.get("WRITE_SIZE_bytes_per_launch") or 0)
                n += 1
            except ValueError:
                pass
    return round(total / n) if n else None


def counters_in_run(args, group, S, counters=(("FETCH_SIZE", 2.0 * 1024.0), ("WRITE_SIZE", 1024.0), ("SQ_INSTS_VALU", 1.0)), also=()):
    """Per-STEP sums of hardware counters over the group's kernels, measured NOW: one rocprofv3 --pmc pass per counter (one counter per pass and no trace
    domain beside it, as MI355X_MICROARCH.md prescribes) over a child run of this bench that executes exactly `nsteps` steps of the same workload and nothing
    else (--traffic-child).  FETCH_SIZE / WRITE_SIZE are in KiB, FETCH_SIZE x2 (gfx950 note): their sum is the HBM traffic in the unit of
    roofline.algorithmic_bytes_per_step; SQ_INSTS_VALU = wavefront-level vector instructions.  Returns {counter: value per step} (a counter whose pass failed is
    missing), {} when rocprofv3 is not on PATH or --traffic 0.  `also`: further launch groups read from the SAME passes -> out["also"][group] = {counter: value}."""
    import csv
    import glob
    import shutil
    import tempfile
    exe = shutil.which("rocprofv3")
    prefix = _kernel_prefix(group, S)
    if not exe or prefix is None or not args.traffic:
        return {}
    nsteps = 2
    base = [sys.executable, os.path.abspath(__file__), "--traffic-child", str(nsteps), "--no-graph", "--inflight", "1", "--tune", "0", "--no-cpu-baseline", "--extra-4k", "0",
            "--decisions", "0", "--traffic", "0", "--res", args.res, "--bit-depth", str(args.bit_depth), "--qp", str(args.qp),
            "--seed", str(args.seed), "--mix", args.mix, "--rdoq", str(args.rdoq), "--sad4", args.sad4]
    out = {}
    env = dict(os.environ, TMPDIR="/tmp")
    for counter, mult in counters:
        d = tempfile.mkdtemp(prefix="havoc_pmc_", dir="/tmp")
        try:
            subprocess.run([exe, "--pmc", counter, "--output-format", "csv", "-d", d, "--"] + base, capture_output=True, text=True, timeout=400, cwd="/tmp", env=env)
            vals = []
            more = {g: [] for g in also if _kernel_prefix(g, S) is not None}
            for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    if row["Counter_Name"] != counter:
                        continue
                    if _matches(prefix, row["Kernel_Name"]):
                        vals.append(float(row["Counter_Value"]))
                    for g in more:
                        if _matches(_kernel_prefix(g, S), row["Kernel_Name"]):
                            more[g].append(float(row["Counter_Value"]))
            if vals:
                out[counter] = sum(vals) * mult / nsteps
            for g, v in more.items():
                if v:
                    out.setdefault("also", {}).setdefault(g, {})[counter] = sum(v) * mult / nsteps
        except (subprocess.TimeoutExpired, OSError, KeyError, ValueError):
            pass
        finally:
            shutil.rmtree(d, ignore_errors=True)
    return out


def valu_busy_from_profiles(group, S):
    """VALU busy % of the group's kernel(s) from the newest profiles/r*_sq_counters.csv (rocprofv3 --pmc passes of this bench,
    profiles/collect.sh: 100 * 4 * SQ_ACTIVE_INST_VALU / 1024 SIMDs / busy cycles), weighted by busy time; None without a profile"""
    import csv
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_sq_counters.csv")))
    prefix = _kernel_prefix(group, S)
    if not files or prefix is None:
        return None
    num = den = 0.0
    for row in csv.DictReader(open(files[-1])):
        if _matches(prefix, row["Kernel"]):
            try:
                t = float(row["busy_us_at_2.4GHz"])
                num += float(row["VALUBusy_pct"]) * t
                den += t
            except (KeyError, ValueError):
                pass
    return round(num / den, 2) if den else None


def _matches(prefix, name):
    return any(p in name for p in prefix) if isinstance(prefix, tuple) else prefix in name


def _kernel_prefix(group, S):
    return {"sad4": (f"k_sad4r<{S}", f"k_sad4w<{S}", f"k_sad<{S}, 4"), "sad": f"k_sad<{S}, 1", "interp_planes": "k_interp_planes", "intra_satd35": "k_intra_satd35<",
              "intra": "k_intra<", "residual": "k_residual<", "transform": "k_transform<", "quantize_inverse": "k_quantize_inverse",
              "inverse_transform_add": "k_inverse_transform<", "ssd": "k_ssd<", "subtract_bi": "k_subtract_bi<",
              "subpel_satd": "k_subpel_satd<", "rdoq": "k_rdoq_", "deblock": "k_deblock<"}.get(group)


def kernel_figures(args, dev, wl, world, ms_step):
    """--full: the per-kernel times of the step (HIP events, each launch group alone), the roofline of its dominant and of its worst launch group
    (with counter passes of a child run: counters_in_run) and a checksum of every result buffer -- the keys `roofline`, `roofline_worst_group`,
    `whole_step` and `checksum` of the line"""
    ktimes, kcount = dev.kernel_times_ms(args.kernel_reps)
    kbytes = wl.algorithmic_bytes()
    kbytes["sad_surface"] = kbytes["sad_surface"](args.ime_range)
    # the dominant KERNEL: the launch group whose single launch takes longest (a group's time / its launches per step).  Round 4 picked the group with the largest TOTAL,
    # which since the run form of sad4 would be `rdoq` -- four to five launches of different kernels per step, none of them the step's longest
    dom = max(ktimes, key=lambda k: ktimes[k] / kcount[k])
    # roofline of the dominant launch group.  HBM: `achieved` counts UNIQUE algorithmic bytes -- SURVEY 8(d)'s operands once +
    # results once per call, except where the calls of one search overlap (sad4: the box of a search's candidates + its source block once per run + 16 B per
    # call; the per-call figure, which counts every reference sample ~112 times, is kept beside it as `operand_bytes_per_step`), so frac <= 1 by construction
    # and comparable with `traffic`.  VALU: wavefront-level vector instructions (SQ_INSTS_VALU of a --pmc pass of this run) / duration against the issue peak.
    unique = dict(kbytes)
    if dom == "sad4":
        unique["sad4"] = wl.sad4_unique_bytes()
    ach = unique[dom] / (ktimes[dom] * 1e-3) / 1e9
    total_bytes = sum(kbytes[k] for k in ktimes)
    traffic, traffic_source, valu = None, None, None
    if world == 1 and not (args.pcie or args.skip or args.no_graph) and args.min_seconds != 0:
        c = counters_in_run(args, dom, wl.S, also=("rdoq",) if dom != "rdoq" and "rdoq" in ktimes else ())
        if "FETCH_SIZE" in c and "WRITE_SIZE" in c:
            traffic = round(c["FETCH_SIZE"] + c["WRITE_SIZE"])
            traffic_source = ("measured in this run, bytes PER STEP (the unit of algorithmic_bytes_per_step): rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE, one "
                              "counter per pass, no trace domain) over a child run of exactly two steps of the same workload; FETCH_SIZE x2 per the gfx950 note; "
                              "summed over every launch of the group's kernels, divided by the steps")
        if "SQ_INSTS_VALU" in c:
            insts = c["SQ_INSTS_VALU"]
            rate = insts / (ktimes[dom] * 1e-3) / 1e9
            valu = {"insts_per_step": round(insts), "achieved": round(rate, 2), "peak": VALU_PEAK_GINST, "unit": "G wavefront-instructions/s",
                    "frac": round(rate / VALU_PEAK_GINST, 5)}
    if traffic is None:
        traffic = hbm_traffic_from_profiles(dom, wl.S)
        if traffic is not None:
            traffic *= kcount[dom]      # the committed summary is per launch: times the group's launches per step (kernels of unequal size: approximate)
        traffic_source = ("profiles/r*_hbm_traffic.csv (mean per launch x launches per step: approximate): separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this bench (profiles/collect.sh), "
                          "FETCH_SIZE x2 per the gfx950 note; not re-measured in this run (rocprofv3 not on PATH, --traffic 0, or a diagnostic run)")
    # the launch group furthest below any roofline is in the line too: `rdoq` -- several kernels of dependent decision chains per step
    worst = None
    if "rdoq" in ktimes and dom != "rdoq":
        wc = (c.get("also", {}).get("rdoq", {}) if world == 1 and not (args.pcie or args.skip or args.no_graph) and args.min_seconds != 0 else {})      # (`c`: the counter passes above)
        wa = kbytes["rdoq"] / (ktimes["rdoq"] * 1e-3) / 1e9
        worst = {"bound": "hbm", "kernel": "rdoq", "achieved": round(wa, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(wa / HBM_PEAK_GBS, 5),
                 "traffic": round(wc["FETCH_SIZE"] + wc["WRITE_SIZE"]) if "FETCH_SIZE" in wc and "WRITE_SIZE" in wc else None,
                 "group_ms": round(ktimes["rdoq"], 5), "launches_per_step": kcount["rdoq"], "algorithmic_bytes_per_step": kbytes["rdoq"]}
        if "SQ_INSTS_VALU" in wc:
            wr = wc["SQ_INSTS_VALU"] / (ktimes["rdoq"] * 1e-3) / 1e9
            worst["valu"] = {"insts_per_step": round(wc["SQ_INSTS_VALU"]), "achieved": round(wr, 2), "peak": VALU_PEAK_GINST, "frac": round(wr / VALU_PEAK_GINST, 5)}
    return {
        "roofline": {"bound": "hbm", "kernel": dom, "achieved": round(ach, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(ach / HBM_PEAK_GBS, 5), "traffic": traffic,
                     "traffic_source": traffic_source,
                     "launch_ms": round(ktimes[dom] / kcount[dom], 5), "launches_per_step": kcount[dom],
                     "algorithmic_bytes_per_step": unique[dom], "operand_bytes_per_step": kbytes[dom],
                     "valu": valu, "valu_busy_pct": valu_busy_from_profiles(dom, wl.S),
                     "note": ("achieved = unique algorithmic bytes / the group's isolated HIP-event time.  The group is not HBM-bound: its operands are cache- and LDS-resident "
                              "and what bounds it is instruction issue along short dependent chains -- `valu` is the instruction roofline (SQ_INSTS_VALU / time against "
                              "256 CUs x 4 SIMDs x 2.4 GHz / 2 cycles per wave64 instruction); `traffic` / `algorithmic_bytes_per_step` says how close the kernel is to "
                              "touching every byte once")},
        "roofline_worst_group": worst,
        # operand_gbs: the per-CALL operand bytes of SURVEY 8(d) over the step time -- NOT an HBM figure (the calls of a search name the same reference samples ~112 times and
        # the operands are cache- and LDS-resident: it can exceed the HBM peak); the HBM statement is `roofline` (unique bytes, measured traffic)
        "whole_step": {"operand_bytes": total_bytes, "operand_gbs": round(total_bytes / (ms_step * 1e-3) / 1e9, 2),
                       "kernel_ms": {k: round(v, 4) for k, v in sorted(ktimes.items(), key=lambda kv: -kv[1])},
                       "kernel_gbs": {k: round(kbytes[k] / (v * 1e-3) / 1e9, 1) for k, v in ktimes.items()}},
        "checksum": dev.checksum(),
    }


def parity_problems(out):
    """every comparison with the reference this run made that did NOT come out equal (or could not be made): [] = green"""
    bad = []
    cb = out.get("cpu_baseline")
    if isinstance(cb, dict):
        pv = cb.get("parity_vs_reference")
        if isinstance(pv, dict):
            if "error" in pv:
                bad.append("primitive parity could not be checked: " + str(pv["error"])[:200])
            elif pv.get("mismatches"):
                bad.append(f"primitives: {pv['mismatches']} of {pv['compared']} values differ from the reference library ({pv.get('mismatches_by_group')})")
        he = cb.get("hooked_encoder")
        if isinstance(he, dict) and he.get("stream_identical") is False:
            bad.append("the reference encoder over the drop-in tables wrote a different stream than over its own havoc library")
    for label, r in (out.get("extra") or {}).items():
        pv = r.get("parity_vs_reference") if isinstance(r, dict) else None
        if isinstance(pv, dict):
            if "error" in pv:
                bad.append(f"{label}: decision parity could not be checked: " + str(pv["error"])[:200])
            elif pv.get("mismatching") or pv.get("bi_directional_mismatching") or pv.get("motion_field_equal") is False:
                bad.append(f"{label}: {pv.get('mismatching')} searches / {pv.get('bi_directional_mismatching')} refinements differ from the walk through the reference's tables")
    return bad


def short_label(label):
    """`extra` keys of the ONE line: the long, self-explaining labels stay in the detail file"""
    import re
    m = re.match(r"decision-driven path (\d+)x(\d+) (\d+)-bit QP(\d+)", label)
    if m:
        d = re.search(r"temporal distance (\d+)", label)
        return f"decisions_{m.group(2)}p_{m.group(3)}bit_qp{m.group(4)}_d{d.group(1) if d else 1}"
    m = re.match(r"(\d+)x(\d+) (\d+)-bit.*QP(\d+)", label)
    if m:
        return f"primitives_{m.group(2)}p_{m.group(3)}bit_qp{m.group(4)}"
    if label.startswith("same picture without RDOQ"):
        return "primitives_without_rdoq"
    if label.startswith("same step, one picture in flight"):
        return "primitives_one_in_flight_latency"
    return re.sub(r"[^a-z0-9]+", "_", label.lower())[:48]


def compact_line(out, args):
    """the ONE JSON line: the contract's keys, `roofline`, `cpu_baseline`, `parity`, and figures only under `extra` -- every explanatory string and every
    per-kernel / per-distance table is in --detail-out (the driver keeps 8 KB of the line; round 4's 41 KB line went unparsed)"""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "parity")
    line = {k: out[k] for k in keep if k in out}
    line["metric"] = out["metric"][:120]
    cfg = out.get("config", {})
    line["config"] = {"workload": cfg.get("workload", "")[:160], **{k: cfg[k] for k in ("calls_per_frame", "launches_per_frame", "pictures_in_flight", "pictures_per_timed_block") if k in cfg},
                      "parallelism": cfg.get("parallelism_short") or cfg.get("parallelism", "")[:100]}
    t = out.get("timing", {})
    line["timing"] = {k: t[k] for k in ("timed_blocks", "block_seconds_median", "block_seconds_min", "block_seconds_max") if k in t}
    if "roofline" in out:
        rf = dict(out["roofline"])
        for k in ("note", "traffic_source"):
            rf.pop(k, None)
        line["roofline"] = rf
    if out.get("roofline_worst_group"):
        line["roofline_worst_group"] = out["roofline_worst_group"]
    ws = out.get("whole_step", {})
    if ws:
        line["whole_step"] = {"operand_bytes": ws.get("operand_bytes"), "operand_gbs": ws.get("operand_gbs"),
                              "kernel_ms": {k: round(v, 3) for k, v in list(ws.get("kernel_ms", {}).items())[:8]}}
    if "checksum" in out:
        line["checksum"] = out["checksum"]
    cb = out.get("cpu_baseline")
    if isinstance(cb, dict):
        c = {k: cb[k] for k in ("value", "unit", "cores", "kind") if k in cb}
        c["sample"] = str(cb.get("sample", ""))[:200]
        pv = cb.get("parity_vs_reference")
        if isinstance(pv, dict):
            c["parity_vs_reference"] = {k: pv[k] for k in ("compared", "mismatches", "mismatches_by_group", "mismatches_after_eager_rerun", "first_mismatch", "dump", "error") if k in pv}
            if len(json.dumps(c["parity_vs_reference"])) > 1500:
                c["parity_vs_reference"].pop("first_mismatch", None)
        pt = cb.get("primitive_tables")
        if isinstance(pt, dict):
            c["primitive_tables"] = {"value": pt.get("value"), "unit": pt.get("unit"), "cores": pt.get("cores")}
        dw = cb.get("decision_walk")
        if isinstance(dw, dict):
            c["decision_walk"] = {k: dw[k] for k in ("pictures_per_second", "cores", "searches") if k in dw}
            if isinstance(dw.get("parity_vs_reference"), dict):
                c["decision_walk"]["parity_vs_reference"] = dw["parity_vs_reference"]
        he = cb.get("hooked_encoder")
        if isinstance(he, dict):
            c["hooked_encoder"] = {k: he[k] for k in ("value", "unit", "served_fraction", "us_per_table_call", "stream_identical", "error") if k in he}
        line["cpu_baseline"] = c
    elif "cpu_baseline" in out:
        line["cpu_baseline"] = cb
    ex = {}
    for label, r in (out.get("extra") or {}).items():
        if not isinstance(r, dict):
            continue
        e = {k: r[k] for k in ("value", "unit", "ms_per_step", "ms_per_picture", "pictures_in_flight", "one_picture_alone_ms", "ratio_to_value", "error") if k in r}
        for k, v in r.items():
            if k.startswith("pictures_in_flight_") and isinstance(v, dict):
                e[k] = v.get("value")
        if isinstance(r.get("sop_weighted"), dict):
            e["sop_weighted"] = r["sop_weighted"].get("value")
        pv = r.get("parity_vs_reference")
        if isinstance(pv, dict):
            e["mismatching"] = (pv.get("mismatching", 0) or 0) + (pv.get("bi_directional_mismatching", 0) or 0) if "error" not in pv else pv["error"][:80]
            e["searches_compared"] = pv.get("searches_compared")
        if "error" in e:
            e["error"] = str(e["error"])[:160]
        ex[short_label(label)] = e
    if ex:
        line["extra"] = ex
    if out.get("poc_checksums"):
        line["poc_checksums"] = out["poc_checksums"]
    if out.get("parity_problems"):
        line["parity_problems"] = [p[:300] for p in out["parity_problems"][:4]]
    if args.detail_out:
        line["detail"] = os.path.relpath(args.detail_out, ROOT)
    return line


def build_contexts(args, torch, Havoc, FrameWorkload, local, res, bit_depth, qp, mix, seed0, count, tune):
    """`count` picture contexts: each has a private compute stream (the step is captured into a HIP graph and replayed on
    it; made through torch so that torch events can order it against the exchange stream), its own picture store / job
    tables / outputs and its own planned graph."""
    w, h = (int(v) for v in res.split("x"))
    out = []
    for k in range(count):
        compute_k = torch.cuda.Stream(device=local)
        hv_k = Havoc(local, stream=compute_k.cuda_stream)
        frames = None
        if getattr(args, "yuv", None) and res == args.res:
            from turingcodec_amd.picture_io import YuvReader
            rd = YuvReader(args.yuv, w, h, bit_depth)
            frames = [rd.planes((3 * k + i) % max(1, len(rd))) for i in range(3)]
        wl_k = FrameWorkload(w, h, bit_depth, seed0 + 1000 * k, qp=qp, mix=mix, frames=frames)
        dev_k = DeviceFrame(hv_k, wl_k, use_planes=(args.subpel == "planes"), fused_tu=(args.tu == "fused"),
                            ime_range=args.ime_range if args.ime == "surface" else None, skip=[s for s in args.skip.split(",") if s],
                            rdoq=args.rdoq, pred_launches=getattr(args, "pred", "merged"), scan_in_forward=not getattr(args, "separate_scan", False),
                            sad4_runs=getattr(args, "sad4", "runs") == "runs")
        dev_k.step()          # first eager pass (loads the code objects) -- also what the graph must reproduce
        hv_k.sync()
        if args.no_graph:
            graph_k = None
        elif args.lanes > 1 and tune > 0:
            graph_k, _ = dev_k.plan_lanes(args.lanes, tune)     # lane assignment chosen by measurement (set-up, untimed)
        else:
            graph_k = hv_k.graph_capture(lambda: dev_k.step(args.lanes))
        out.append((compute_k, hv_k, wl_k, dev_k, graph_k))
    return out


def timed_blocks(torch, dist, world, steps, min_seconds, run_block, max_blocks=64):
    """Repeat [barrier + synchronize | exactly `steps` steps | synchronize + barrier] until `min_seconds` have been measured
    (a 20-step block of this path is a few milliseconds: one block alone is mostly noise).  Every block's duration is
    the MAX over ranks, so all ranks take the same stop decision.  Returns the list of block durations in seconds."""
    out, total = [], 0.0
    while True:
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_block(len(out))
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([dt], device="cuda", dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        out.append(dt)
        total += dt
        if total >= min_seconds or len(out) >= max_blocks:
            return out


DUMP_BYTES = 64 * 10 ** 6


def dump_outputs(torch, dev, out_dir):
    """--dump-outputs: every result buffer of `dev` (DeviceFrame.outputs) as out_dir/<name>.npy, 8- / 16-bit values as float32 and 32-bit ones as
    float64 (both exact).  A buffer above its share of DUMP_BYTES is written as the elements at a fixed sample of indices, seeded by its name and
    length, so that two builds run with the same arguments write the same elements.  Returns {name: [elements written, elements in the buffer]}."""
    import zlib
    os.makedirs(out_dir, exist_ok=True)
    bufs = dev.outputs()
    cap = (DUMP_BYTES - 256 * len(bufs)) // (8 * len(bufs))      # (256: room for each file's .npy header)
    written = {}
    for name, (t, dtype) in bufs.items():
        n = t.numel()
        if n > cap:
            rng = np.random.default_rng([zlib.crc32(name.encode()), n])
            t = t[torch.from_numpy(np.unique(rng.integers(0, n, cap))).to(t.device)]
        a = t.cpu().numpy().view(dtype)
        np.save(os.path.join(out_dir, name + ".npy"), a.astype(np.float32 if a.itemsize <= 2 else np.float64))
        written[name] = [int(a.size), int(n)]
    return written


def decision_frame_parallel(args, torch, dist, Havoc, rank, world, local):
    """--decisions 3: the frame-parallel pipeline driving the DECISION step: time slot t of the DagSchedule, this rank's picture of
    the slot = one DecisionPicture.step() (searches in wavefront order, bi-directional refinement, intra candidates, merge candidates, transform-tree decisions,
    chroma chain, deblocking, padding) predicting from the DPB MIRROR -- luma and both chroma planes of its two references are copied out of the mirror slots the
    schedule names -- and, for a reference picture, its padded reconstruction staged into the mirror and broadcast (whole, or in CTU-row bands with --bands).
    A picture's step is host-synchronous (it ends with a wait), so one context per rank.  Reports pictures/s over all ranks and per-POC checksums of the
    reconstructions (equal for every world size: tests compare world 1 with world 2)."""
    from turingcodec_amd.decisions import DecisionPicture
    from turingcodec_amd.frame_parallel import BandPlan, DagSchedule, ReferenceExchange
    w, h = (int(v) for v in args.res.split("x"))
    n_sops = max(1, (args.pictures - 1) // 8)
    sched = DagSchedule(world, n_sops=n_sops, lag=args.lag or None)
    hv = Havoc(local, stream="new")
    dp = DecisionPicture(hv, w, h, args.bit_depth, args.qp, seed=args.seed, threads=max(1, usable_cores() // max(1, world)), distance=max(1, args.decision_distance))
    pe, cpe = dp.pe, dp.cpe
    exch = ReferenceExchange(dist, rank, sched, pe, cpe, dp.d_pic, single_rank_broadcast=args.exchange)
    if args.bands > 0:
        exch.set_bands(BandPlan(h, dp.PAD, dp.stride, dp.cstride, band_ctu_rows=args.bands))
    comm = torch.cuda.current_stream(local)
    sums, pictures = {}, 0
    # every picture of the sequence has its own source (the generator's translating texture, frame = POC): luma, Cb, Cr in the context's padded layout, resident
    from turingcodec_amd import workload
    frames = workload.synth_frames(w, h, 8 * n_sops + 1, args.seed, args.bit_depth)
    sources = []
    for f in frames:
        planes = [workload.pad_plane(f[0], dp.PAD), workload.pad_plane(f[1], dp.PAD // 2), workload.pad_plane(f[2], dp.PAD // 2)]
        assert planes[0].shape[1] == dp.stride and planes[1].shape[1] == dp.cstride
        sources.append([hv.up(np.ascontiguousarray(p.ravel())) for p in planes])
    dp.step()      # allocations, code objects
    dp.step()      # records the fixed launch sequences into HIP graphs
    hv.sync()
    nslots = sched.slots_for_sequence()
    if world > 1 or args.exchange:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(nslots):
        pic = exch.picture_of(t)
        if pic is not None:
            pictures += 1
            src = sources[pic.poc]
            with torch.cuda.stream(hv.tstream):
                torch._foreach_copy_([dp.d_pic[:src[0].numel()], dp.d_cpic[:src[1].numel()], dp.d_cpic[3 * cpe:3 * cpe + src[2].numel()]], src)
            if pic.refs:
                s0, s1 = exch.refs(pic)
                hv.tstream.wait_stream(comm)      # the broadcasts of the earlier slots have landed in the mirror
                with torch.cuda.stream(hv.tstream):
                    torch._foreach_copy_([dp.d_pic[pe:2 * pe], dp.d_pic[2 * pe:3 * pe], dp.d_cpic[cpe:2 * cpe], dp.d_cpic[2 * cpe:3 * cpe], dp.d_cpic[4 * cpe:5 * cpe],
                                          dp.d_cpic[5 * cpe:6 * cpe]],
                                         [exch.dpb_luma[s0], exch.dpb_luma[s1], exch.dpb_cb[s0], exch.dpb_cb[s1], exch.dpb_cr[s0], exch.dpb_cr[s1]])
            dp.step()
            # the chroma planes' borders (the luma plane's are made by the step's loop filter): every picture, so that the checksum below covers whole planes
            hv.pad_block_d(dp.crecon, dp.corigin, w // 2, h // 2, dp.cstride, dp.PAD // 2)
            hv.pad_block_d(dp.crecon, cpe + dp.corigin, w // 2, h // 2, dp.cstride, dp.PAD // 2)
            with torch.cuda.stream(hv.tstream):
                sums[pic.poc] = int(dp.recon.to(torch.int64).sum().item()) * 1000003 + int(dp.crecon.to(torch.int64).sum().item())
            if pic.is_reference:
                hv.tstream.wait_stream(comm)      # the mirror slot's previous picture: its broadcast is over before it is overwritten
                with torch.cuda.stream(hv.tstream):
                    exch.stage(t, (dp.recon[:pe], dp.crecon[:cpe], dp.crecon[cpe:2 * cpe]))
        comm.wait_stream(hv.tstream)
        if exch.plan is not None:
            for b in range(exch.plan.n_bands):
                exch.send_band(t, b)
        else:
            exch.send(t)
    torch.cuda.synchronize()
    if world > 1 or args.exchange:
        dist.barrier()
    el = torch.tensor([time.perf_counter() - t0], device="cuda", dtype=torch.float64)
    n = torch.tensor([pictures], device="cuda", dtype=torch.float64)
    if world > 1:
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
        dist.all_reduce(n)
        parts = [None] * world
        dist.all_gather_object(parts, sums)
        for d in parts:
            sums.update(d)
    if rank == 0:
        total = 0
        for poc in sorted(sums):
            total = (total * 1000003 + sums[poc]) % (1 << 61)
        print(json.dumps({"metric": "DIAGNOSTIC (frame-parallel pipeline driving the decision step) -- not the benchmark metric", "value": round(float(n.item()) / float(el.item()), 2),
                          "unit": "pictures/s", "n_gpus": world, "pictures": int(n.item()), "slots": nslots, "seconds": round(float(el.item()), 4),
                          "config": {"workload": f"{args.res} {args.bit_depth}-bit QP{args.qp}: IDR + {n_sops} SOPs of 8, hierarchical-B docket, one DecisionPicture.step per picture",
                                     "exchange": ("CTU-row bands of %d rows (%d bands x 3 planes per reference picture)" % (args.bands, exch.plan.n_bands)) if exch.plan is not None
                                     else "one broadcast per reference picture", "backend": os.environ.get("HAVOC_BENCH_BACKEND", "nccl") if (world > 1 or args.exchange) else None,
                                     "broadcasts": exch.broadcasts, "bytes_sent_by_rank0": exch.sent_bytes},
                          "checksum_of_poc_checksums": total, "poc_checksums": {str(k): v for k, v in sorted(sums.items())}}), flush=True)


def decision_virtual_ranks(args, torch, Havoc):
    """--decisions 4: ONE sequence through the decision step with its real picture dependencies on ONE GPU (the single-device half): the frame-parallel
    schedule of K = --virtual-ranks ranks (DagSchedule: the hierarchical-B docket, a picture starts after the slots of its references) executed by K host threads, each with
    its own DecisionPicture context and stream, sharing one DPB mirror in device memory -- what K GPUs would do with the broadcasts replaced by the shared mirror.  Slots are
    separated by a barrier of the threads (a picture's references are complete when its slot starts; a mirror slot is reused as the schedule says).  Reports pictures/s of the
    whole sequence and a checksum per POC: equal to --decisions 3 on one rank (tests), whatever K.  The bound of ONE sequence is its anchor chain -- POC 8 -> 16 -> 24 are
    serial, each a picture at reference distance 8 -- so at most 8 pictures per latency of such a picture, however many contexts run."""
    import threading
    from turingcodec_amd import workload
    from turingcodec_amd.decisions import DecisionPicture
    from turingcodec_amd.frame_parallel import DagSchedule, ReferenceExchange
    K = max(1, args.virtual_ranks)
    w, h = (int(v) for v in args.res.split("x"))
    n_sops = max(1, (args.pictures - 1) // 8)
    sched = DagSchedule(K, n_sops=n_sops, lag=args.lag or None)
    cores = usable_cores()
    ctxs = []
    for r in range(K):
        hv = Havoc(0, stream="new")
        ctxs.append(DecisionPicture(hv, w, h, args.bit_depth, args.qp, seed=args.seed, threads=max(1, cores // K), distance=max(1, args.decision_distance),
                                    intra=not (args.vr_bands > 0 and args.vr_issue == "single") and not args.vr_no_intra))
    dp0 = ctxs[0]
    pe, cpe = dp0.pe, dp0.cpe
    exch = [ReferenceExchange(None, r, sched, pe, cpe, dp0.d_pic) for r in range(K)]
    for e in exch[1:]:      # ONE mirror: what a broadcast would have delivered is simply there
        e.dpb, e.dpb_luma, e.dpb_cb, e.dpb_cr = exch[0].dpb, exch[0].dpb_luma, exch[0].dpb_cb, exch[0].dpb_cr
    frames = workload.synth_frames(w, h, 8 * n_sops + 1, args.seed, args.bit_depth)
    sources = []
    for f in frames:
        planes = [workload.pad_plane(f[0], dp0.PAD), workload.pad_plane(f[1], dp0.PAD // 2), workload.pad_plane(f[2], dp0.PAD // 2)]
        sources.append([dp0.hv.up(np.ascontiguousarray(p.ravel())) for p in planes])
    bands = max(0, args.vr_bands)
    sides = []
    if bands:
        # two more contexts per picture context (the bands' work; following the references), each on a stream of its own.  What waits on a stream must not sit in a hardware
        # queue in front of what it waits for: HIP deals the streams of one priority onto GPU_MAX_HW_QUEUES queues -- and the HIGH-priority pool turned out to be small: with
        # these sixteen streams at priority -1 eight contexts ran no faster than one (33-40 pictures/s; at the searching streams' priority 63-82: gpu calls r05ac / r05ad)
        for dp in ctxs:
            prio = int(os.environ.get("HAVOC_VR_SIDE_PRIORITY", "0"))
            st, fs = torch.cuda.Stream(device=0, priority=prio), torch.cuda.Stream(device=0, priority=prio)
            sides.append((Havoc(0, stream=st.cuda_stream), st, Havoc(0, stream=fs.cuda_stream), fs))
    for r, dp in enumerate(ctxs):
        if bands:
            for _ in range(3):      # (allocations, then the bands' launch sequences recorded into graphs, then replayed)
                dp.step_banded(sides[r][0], bands)
        else:
            dp.step()
            dp.step()      # records the fixed launch sequences into HIP graphs
        dp.hv.sync()
    torch.cuda.synchronize()
    nslots = sched.slots_for_sequence()
    barrier = threading.Barrier(K)
    sums, busy, errors = {}, [0.0] * K, []
    # --vr-dataflow 1 (default): no barrier between the slots -- a picture starts when the pictures it predicts from are in the mirror, and stages its reconstruction when every
    # picture that predicts from the mirror slot's previous occupant has taken its copy (each context still works through its own pictures in slot order, so nothing can wait
    # for something scheduled after it)
    dataflow = bool(args.vr_dataflow)
    done = {}                  # poc -> Event: the picture's reconstruction is in the mirror
    readers_left = {}          # poc -> pictures that still have to copy it out of the mirror
    occupant = {}              # mirror slot -> poc staged there last
    lock = threading.Condition()
    for t in range(nslots):
        for q in sched.slot(t):
            if q is not None:
                done[q.poc] = threading.Event()
                if q.refs:
                    for ref_poc in {q.l0, q.l1}:
                        readers_left[ref_poc] = readers_left.get(ref_poc, 0) + 1

    # ---- --vr-bands: a picture's rows enter the mirror as they become final, and its dependants follow it down the picture -------------------------------------------
    queued = {q.poc: threading.Event() for t in range(nslots) for q in sched.slot(t) if q is not None}      # everything of the picture is queued: its band events exist
    band_events = {}           # poc -> [torch event per band]: the band's rows (Y, Cb, Cr, padded) are in the mirror
    PAD = dp0.PAD
    rows_total, crows_total = h + 2 * PAD, h // 2 + PAD
    bl = dp0.band_rows(bands) if bands else []

    def final_rows(b):          # luma rows of a picture that are final once band b is deblocked (the next band's top edge still changes three rows above it)
        return h + PAD if b == len(bl) - 1 else bl[b][1] - 4

    def banded_worker(r):
        dp, hv, ex, (side, side_stream, fol, fol_stream) = ctxs[r], ctxs[r].hv, exch[r], sides[r]
        stride, cstride = dp.stride, dp.cstride
        gate = hv.zeros(2, np.int32)
        try:
            for t in range(nslots):
                pic = ex.picture_of(t)
                if pic is None:
                    continue
                t0 = time.perf_counter()
                refs = sorted({pic.l0, pic.l1}) if pic.refs else []
                for ref_poc in refs:
                    if not queued[ref_poc].wait(timeout=120):
                        raise RuntimeError(f"POC {pic.poc}: reference {ref_poc} was never queued")
                t1 = time.perf_counter()
                if pic.is_reference:      # the mirror slot's previous picture must have been read by everyone who predicts from it before the first band goes in
                    with lock:
                        prev = occupant.get(ex.slot_of(pic.poc))
                        if prev is not None and not lock.wait_for(lambda: readers_left.get(prev, 0) <= 0, timeout=120):
                            raise RuntimeError(f"POC {pic.poc}: the mirror slot of POC {prev} was never released")
                        occupant[ex.slot_of(pic.poc)] = pic.poc
                t2 = time.perf_counter()
                src = sources[pic.poc]
                with torch.cuda.stream(hv.tstream):
                    torch._foreach_copy_([dp.d_pic[:src[0].numel()], dp.d_cpic[:src[1].numel()], dp.d_cpic[3 * cpe:3 * cpe + src[2].numel()]], src)
                    gate.zero_() if pic.refs else gate.fill_(1 << 20)
                    ready = torch.cuda.Event()
                    ready.record(hv.tstream)
                fol_stream.wait_event(ready)      # (what this picture's follower stream does to the reference planes and the gate comes after the source copy and the gate's reset)
                hv.search_gate(gate)
                state = {"rows": 0, "planes": 4, "staged": 0}
                followed = []      # per band of the references: the event "its rows are in this picture's planes
                if pic.refs:
                    s0, s1 = ex.refs(pic)
                    mine = [(dp.d_pic[pe:2 * pe], ex.dpb_luma[s0], stride, 1), (dp.d_pic[2 * pe:3 * pe], ex.dpb_luma[s1], stride, 1),
                            (dp.d_cpic[cpe:2 * cpe], ex.dpb_cb[s0], cstride, 2), (dp.d_cpic[2 * cpe:3 * cpe], ex.dpb_cb[s1], cstride, 2),
                            (dp.d_cpic[4 * cpe:5 * cpe], ex.dpb_cr[s0], cstride, 2), (dp.d_cpic[5 * cpe:6 * cpe], ex.dpb_cr[s1], cstride, 2)]

                def follow(k):      # band k of BOTH references out of the mirror: the rows, the fractional planes of those whose filter taps are there, the gate -- on a
                    # stream of its own: the gate must rise as fast as the references allow, whatever this picture's own bands are doing (queued behind them on the side
                    # stream the follow steps made search and after-search take turns: a picture alone took 50-105 ms instead of 16-46)
                    for ref_poc in refs:
                        fol_stream.wait_event(band_events[ref_poc][k])
                    upto = rows_total if k == len(bl) - 1 else PAD + final_rows(k)
                    lo, end = state["rows"], (rows_total - 4 if upto == rows_total else upto - 4)
                    with torch.cuda.stream(fol_stream):
                        dst, srcs = [], []
                        for own, mirror, st_, div in mine:      # (div 2: a chroma plane, half the rows)
                            a = (lo // div) * st_
                            z = (upto if div == 1 else (crows_total if upto == rows_total else upto // 2)) * st_
                            dst.append(own[a:z])
                            srcs.append(mirror[a:z])
                        for q in (0, 1):      # phase 0 = the picture itself
                            dst.append(dp.d_phase[q * 16 * pe + lo * stride:q * 16 * pe + upto * stride])
                            srcs.append(mine[q][1][lo * stride:upto * stride])
                        # (one copy per plane: torch._foreach_copy_ over these eight gave pictures that differed from run to run with four and more threads issuing --
                        # gpu call r05z; the three-plane one of on_band below and the whole-picture worker's do not)
                        for d_, s_ in zip(dst, srcs):
                            d_.copy_(s_)
                    for q in (0, 1):
                        fol.interp_planes_d(dp.bd, dp.d_phase[q * 16 * pe:(q + 1) * 16 * pe], pe, dp.d_pic[(1 + q) * pe:(2 + q) * pe], stride, 12, state["planes"],
                                            w + 2 * PAD - 24, end - state["planes"])
                    with torch.cuda.stream(fol_stream):
                        gate.fill_(end - PAD)
                        ev = torch.cuda.Event()
                        ev.record(fol_stream)
                    followed.append(ev)
                    state["rows"], state["planes"] = upto, end

                if pic.refs:
                    for k in range(len(bl)):
                        follow(k)

                def before_band(b):      # what band b's predictions read of the references: down to two CTU rows below its last one (+ the filter taps), i.e. their bands up to ...
                    if pic.refs:
                        side_stream.wait_event(followed[min(len(bl) - 1, ((bl[b][1] - 1) // 64 + 3) // bands)])

                events = []

                def on_band(b, final):      # the band into the mirror: chroma borders first (luma's are made by the step), then the rows of the three planes
                    if pic.is_reference:
                        s = ex.slot_of(pic.poc)
                        last = b == len(bl) - 1
                        cy0, cy1 = bl[b][0] // 2, bl[b][1] // 2
                        for comp in (0, 1):
                            side.pad_block_d(dp.crecon, comp * cpe + dp.corigin + cy0 * cstride, w // 2, cy1 - cy0, cstride, PAD // 2, top=b == 0, bottom=last)
                        upto = rows_total if last else PAD + final
                        lo = state["staged"]
                        with torch.cuda.stream(side_stream):
                            c0, c1 = (lo // 2) * cstride, (crows_total if last else upto // 2) * cstride
                            dst = [ex.dpb_luma[s][lo * stride:upto * stride], ex.dpb_cb[s][c0:c1], ex.dpb_cr[s][c0:c1]]
                            srcs = [dp.recon[lo * stride:upto * stride], dp.crecon[c0:c1], dp.crecon[cpe + c0:cpe + c1]]
                            torch._foreach_copy_(dst, srcs)
                        state["staged"] = upto
                    ev = torch.cuda.Event()
                    ev.record(side_stream)
                    events.append(ev)

                def on_queued():
                    band_events[pic.poc] = events
                    queued[pic.poc].set()
                    phases["queued"] = time.perf_counter()

                phases = {}
                dp.step_banded(side, bands, on_band=on_band, before_band=before_band, on_queued=on_queued, make_phase_planes=False)
                t3 = time.perf_counter()
                if os.environ.get("HAVOC_VR_TRACE"):
                    print(f"rank {r} POC {pic.poc:3d} refs {refs}: start {1e3 * (t0 - t_begin[0]):7.1f} ms, waited for its references' queues {1e3 * (t1 - t0):6.1f}, for its mirror slot "
                          f"{1e3 * (t2 - t1):6.1f}, queued after {1e3 * (phases.get('queued', t3) - t2):6.1f}, done after {1e3 * (t3 - t2):6.1f}", file=sys.stderr, flush=True)
                hv.search_gate(None)
                if not pic.is_reference:      # (a leaf's chroma borders: made per band above only where the planes go into the mirror)
                    hv.pad_block_d(dp.crecon, dp.corigin, w // 2, h // 2, dp.cstride, PAD // 2)
                    hv.pad_block_d(dp.crecon, cpe + dp.corigin, w // 2, h // 2, dp.cstride, PAD // 2)
                with torch.cuda.stream(hv.tstream):
                    if args.poc_checksums:
                        sums[pic.poc] = int(dp.recon.to(torch.int64).sum().item()) * 1000003 + int(dp.crecon.to(torch.int64).sum().item())
                hv.sync()
                with lock:
                    for ref_poc in refs:
                        readers_left[ref_poc] -= 1
                    lock.notify_all()
                done[pic.poc].set()
                busy[r] += time.perf_counter() - t0
        except Exception as e:
            errors.append(repr(e))
            for ev in queued.values():      # nobody must wait for a picture that will not come
                ev.set()

    def banded_sequence():
        """--vr-issue single: the whole sequence queued by ONE thread, slot by slot -- nothing on the host waits for the device until the end.  What orders the device:
        a context's streams (its pictures one after the other), an event per band of a reconstruction in the mirror, an event per picture's last follow step (its reads
        of the mirror: the next occupant of a mirror slot stages behind them), the search gates, the wait-for-rows launches."""
        gates = [ctxs[r].hv.zeros(2, np.int32) for r in range(K)]
        ctx_done = [None] * K          # the context's previous picture is complete (its planes and streams are free)
        last_follow = {}               # poc -> event: the picture has taken everything it reads out of the mirror
        readers = {}
        for t in range(nslots):
            for q in sched.slot(t):
                if q is not None and q.refs:
                    for ref_poc in {q.l0, q.l1}:
                        readers.setdefault(ref_poc, []).append(q.poc)
        sum_t = {}
        for t in range(nslots):
            for r in range(K):
                ex = exch[r]
                pic = ex.picture_of(t)
                if pic is None:
                    continue
                dp, hv, (side, side_stream, fol, fol_stream), gate = ctxs[r], ctxs[r].hv, sides[r], gates[r]
                stride, cstride = dp.stride, dp.cstride
                refs = sorted({pic.l0, pic.l1}) if pic.refs else []
                src = sources[pic.poc]
                with torch.cuda.stream(hv.tstream):
                    if ctx_done[r] is not None:
                        hv.tstream.wait_event(ctx_done[r])
                    torch._foreach_copy_([dp.d_pic[:src[0].numel()], dp.d_cpic[:src[1].numel()], dp.d_cpic[3 * cpe:3 * cpe + src[2].numel()]], src)
                    gate.zero_() if pic.refs else gate.fill_(1 << 20)
                    ready = torch.cuda.Event()
                    ready.record(hv.tstream)
                fol_stream.wait_event(ready)
                side_stream.wait_event(ready)
                hv.search_gate(gate)
                state = {"rows": 0, "planes": 4, "staged": 0}
                followed, events = [], []
                if pic.refs:
                    s0, s1 = ex.refs(pic)
                    mine = [(dp.d_pic[pe:2 * pe], ex.dpb_luma[s0], stride, 1), (dp.d_pic[2 * pe:3 * pe], ex.dpb_luma[s1], stride, 1),
                            (dp.d_cpic[cpe:2 * cpe], ex.dpb_cb[s0], cstride, 2), (dp.d_cpic[2 * cpe:3 * cpe], ex.dpb_cb[s1], cstride, 2),
                            (dp.d_cpic[4 * cpe:5 * cpe], ex.dpb_cr[s0], cstride, 2), (dp.d_cpic[5 * cpe:6 * cpe], ex.dpb_cr[s1], cstride, 2)]
                    for k in range(len(bl)):
                        for ref_poc in refs:
                            fol_stream.wait_event(band_events[ref_poc][k])
                        upto = rows_total if k == len(bl) - 1 else PAD + final_rows(k)
                        lo, end = state["rows"], (rows_total - 4 if upto == rows_total else upto - 4)
                        with torch.cuda.stream(fol_stream):
                            for own, mirror, st_, div in mine:
                                a = (lo // div) * st_
                                z = (upto if div == 1 else (crows_total if upto == rows_total else upto // 2)) * st_
                                own[a:z].copy_(mirror[a:z])
                            for q in (0, 1):
                                dp.d_phase[q * 16 * pe + lo * stride:q * 16 * pe + upto * stride].copy_(mine[q][1][lo * stride:upto * stride])
                        for q in (0, 1):
                            fol.interp_planes_d(dp.bd, dp.d_phase[q * 16 * pe:(q + 1) * 16 * pe], pe, dp.d_pic[(1 + q) * pe:(2 + q) * pe], stride, 12, state["planes"],
                                                w + 2 * PAD - 24, end - state["planes"])
                        with torch.cuda.stream(fol_stream):
                            gate.fill_(end - PAD)
                            ev = torch.cuda.Event()
                            ev.record(fol_stream)
                        followed.append(ev)
                        state["rows"], state["planes"] = upto, end
                    last_follow[pic.poc] = followed[-1]
                if pic.is_reference:      # the mirror slot's previous picture: read by everyone who predicts from it before this one's first band goes in
                    prev = occupant.get(ex.slot_of(pic.poc))
                    if prev is not None:
                        for reader in readers.get(prev, []):
                            side_stream.wait_event(last_follow[reader])
                    occupant[ex.slot_of(pic.poc)] = pic.poc

                def before_band(b, followed=followed, side_stream=side_stream, pic=pic):
                    if pic.refs:
                        side_stream.wait_event(followed[min(len(bl) - 1, ((bl[b][1] - 1) // 64 + 3) // bands)])

                def on_band(b, final, dp=dp, ex=ex, pic=pic, side=side, side_stream=side_stream, state=state, events=events, stride=stride, cstride=cstride):
                    if pic.is_reference:
                        s = ex.slot_of(pic.poc)
                        last = b == len(bl) - 1
                        cy0, cy1 = bl[b][0] // 2, bl[b][1] // 2
                        for comp in (0, 1):
                            side.pad_block_d(dp.crecon, comp * cpe + dp.corigin + cy0 * cstride, w // 2, cy1 - cy0, cstride, PAD // 2, top=b == 0, bottom=last)
                        upto = rows_total if last else PAD + final
                        lo = state["staged"]
                        with torch.cuda.stream(side_stream):
                            c0, c1 = (lo // 2) * cstride, (crows_total if last else upto // 2) * cstride
                            torch._foreach_copy_([ex.dpb_luma[s][lo * stride:upto * stride], ex.dpb_cb[s][c0:c1], ex.dpb_cr[s][c0:c1]],
                                                 [dp.recon[lo * stride:upto * stride], dp.crecon[c0:c1], dp.crecon[cpe + c0:cpe + c1]])
                        state["staged"] = upto
                    ev = torch.cuda.Event()
                    ev.record(side_stream)
                    events.append(ev)

                dp.step_banded(side, bands, on_band=on_band, before_band=before_band, make_phase_planes=False, wait=False)
                band_events[pic.poc] = events
                with torch.cuda.stream(hv.tstream):
                    hv.tstream.wait_event(events[-1])
                    if followed:
                        hv.tstream.wait_event(followed[-1])
                if not pic.is_reference:
                    hv.pad_block_d(dp.crecon, dp.corigin, w // 2, h // 2, dp.cstride, PAD // 2)
                    hv.pad_block_d(dp.crecon, cpe + dp.corigin, w // 2, h // 2, dp.cstride, PAD // 2)
                with torch.cuda.stream(hv.tstream):
                    if args.poc_checksums:
                        sum_t[pic.poc] = (dp.recon.to(torch.int64).sum(), dp.crecon.to(torch.int64).sum())
                    done_ev = torch.cuda.Event()
                    done_ev.record(hv.tstream)
                ctx_done[r] = done_ev
        torch.cuda.synchronize()
        for r in range(K):
            ctxs[r].check_banded()      # raises if a device-side wait gave up
        for poc, (a, b) in sum_t.items():
            sums[poc] = int(a.item()) * 1000003 + int(b.item())

    def worker(r):
        if bands:
            return banded_worker(r)
        dp, hv, ex = ctxs[r], ctxs[r].hv, exch[r]
        try:
            for t in range(nslots):
                pic = ex.picture_of(t)
                if pic is not None:
                    if dataflow and pic.refs:
                        for ref_poc in {pic.l0, pic.l1}:
                            if not done[ref_poc].wait(timeout=120):
                                raise RuntimeError(f"POC {pic.poc}: reference {ref_poc} never arrived")
                    t0 = time.perf_counter()
                    src = sources[pic.poc]
                    with torch.cuda.stream(hv.tstream):
                        torch._foreach_copy_([dp.d_pic[:src[0].numel()], dp.d_cpic[:src[1].numel()], dp.d_cpic[3 * cpe:3 * cpe + src[2].numel()]], src)
                        if pic.refs:
                            s0, s1 = ex.refs(pic)
                            torch._foreach_copy_([dp.d_pic[pe:2 * pe], dp.d_pic[2 * pe:3 * pe], dp.d_cpic[cpe:2 * cpe], dp.d_cpic[2 * cpe:3 * cpe], dp.d_cpic[4 * cpe:5 * cpe],
                                                  dp.d_cpic[5 * cpe:6 * cpe]],
                                                 [ex.dpb_luma[s0], ex.dpb_luma[s1], ex.dpb_cb[s0], ex.dpb_cb[s1], ex.dpb_cr[s0], ex.dpb_cr[s1]])
                    dp.step()
                    hv.pad_block_d(dp.crecon, dp.corigin, w // 2, h // 2, dp.cstride, dp.PAD // 2)
                    hv.pad_block_d(dp.crecon, cpe + dp.corigin, w // 2, h // 2, dp.cstride, dp.PAD // 2)
                    if dataflow:
                        hv.sync()      # (the step ended with a wait; the copies out of the mirror were queued before it: they are done)
                        with lock:
                            if pic.refs:
                                for ref_poc in {pic.l0, pic.l1}:
                                    readers_left[ref_poc] -= 1
                            lock.notify_all()
                            if pic.is_reference:      # the mirror slot's previous picture must have been read by everyone who predicts from it
                                prev = occupant.get(ex.slot_of(pic.poc))
                                if prev is not None and not lock.wait_for(lambda: readers_left.get(prev, 0) <= 0, timeout=120):
                                    raise RuntimeError(f"POC {pic.poc}: the mirror slot of POC {prev} was never released")
                                occupant[ex.slot_of(pic.poc)] = pic.poc
                    with torch.cuda.stream(hv.tstream):
                        if args.poc_checksums:
                            sums[pic.poc] = int(dp.recon.to(torch.int64).sum().item()) * 1000003 + int(dp.crecon.to(torch.int64).sum().item())
                        if pic.is_reference:
                            ex.stage(t, (dp.recon[:pe], dp.crecon[:cpe], dp.crecon[cpe:2 * cpe]))
                    hv.sync()
                    done[pic.poc].set()
                    busy[r] += time.perf_counter() - t0
                if not dataflow:
                    barrier.wait()
        except Exception as e:      # a thread that dies must not leave the others at the barrier
            errors.append(repr(e))
            barrier.abort()

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(K)]
    t_begin = [time.perf_counter()]
    t0 = time.perf_counter()
    if bands and args.vr_issue == "single":
        banded_sequence()
        busy = [time.perf_counter() - t0] * K
    else:
        for th in threads:
            th.start()
        for th in threads:
            th.join()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    if errors:
        raise RuntimeError("; ".join(errors))
    pictures = 8 * n_sops + 1
    total = 0
    for poc in sorted(sums):
        total = (total * 1000003 + sums[poc]) % (1 << 61)
    line = {"metric": "DIAGNOSTIC (one sequence through the decision step with its picture dependencies, K virtual ranks on one GPU) -- not the benchmark metric",
            "value": round(pictures / el, 2), "unit": "pictures/s", "n_gpus": 1, "virtual_ranks": K, "pictures": pictures, "slots": nslots, "seconds": round(el, 4),
            "busy_fraction_of_the_contexts": round(sum(busy) / (K * el), 3), "between_slots": (f"bands of {bands} CTU rows (a picture follows its references down the picture), queued by {'one thread' if args.vr_issue == 'single' else 'a thread per context'}" if bands else "dependencies only (dataflow)" if dataflow else "barrier"),
            "config": {"workload": f"{args.res} {args.bit_depth}-bit QP{args.qp}: IDR + {n_sops} SOPs of 8, hierarchical-B docket, one DecisionPicture.step per picture, "
                                   f"schedule of {K} ranks (lag {sched.lag}) run by {K} host threads / contexts sharing one DPB mirror"},
            "checksum_of_poc_checksums": total if sums else None}
    if args.poc_checksums:
        line["poc_checksums"] = {str(k): v for k, v in sorted(sums.items())}
    print(json.dumps(line), flush=True)


def cpu_decision_walk(args, keep):
    """cpu_baseline leg: the SAME decision walk (same pictures, PUs, order, derived predictors) one table call at a time through the
    reference's x86-JIT havoc tables on one host core (tests/search_client.cpp over oracle/_ref -- the checker, timed here as the
    baseline), and every decision compared with what the batch client decided on the GPU"""
    import tempfile
    if not keep or "solo" not in keep:
        return None
    tmp = os.path.join(tempfile.gettempdir(), f"havoc_walk_{os.getpid()}.npz")
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-worker", "decisions", "--res", args.res, "--bit-depth", str(args.bit_depth), "--seed", str(args.seed),
           "--qp", str(args.qp), "--cpu-out", tmp, "--decision-distance", str(max(1, args.decision_distance))]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            return {"error": out.stderr[-500:]}
        r = json.loads(out.stdout.strip().splitlines()[-1])
        ref = np.load(tmp)
        got, field = keep["res"], keep["field"]
        names = ("mv", "mvd", "mv_integer", "mvp_flag", "wrote_2Nx2N", "calls", "cost_integer", "cost_subpel", "cost_mvd_zero")
        bad = sum(int((np.asarray(got[k]) != ref[k]).reshape(len(got), -1).any(axis=1).sum()) for k in names)
        r["parity_vs_reference"] = {"searches_compared": int(len(got)), "fields_per_search": len(names), "mismatching": bad,
                                    "motion_field_equal": bool(np.array_equal(field, ref["field"]))}
        if keep.get("bi") is not None:
            bi = keep["bi"]
            bi_names = ("mv", "mvd", "mvp_flag", "calls", "cost_subpel")
            r["parity_vs_reference"]["bi_directional_refinements_compared"] = int((bi["calls"] > 0).sum())
            r["parity_vs_reference"]["bi_directional_mismatching"] = sum(int((np.asarray(bi[k]) != ref["bi_" + k]).reshape(len(bi), -1).any(axis=1).sum()) for k in bi_names)
            r["seconds_per_picture_with_bi_refinements"] = round(float(ref["seconds_with_bi"]), 4)
        r["what"] = ("the decision walk of extra['decision-driven path ...'] (same picture, PUs, wavefront-compatible order, derived predictors) one table "
                     "call at a time through the reference's x86-JIT havoc tables, ONE host core; searches only (no TU chain)")
        return r
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def cpu_decision_worker(args):
    """child process of cpu_decision_walk"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import search_tools as st
    from turingcodec_amd.decisions import decision_inputs
    w, h = (int(v) for v in args.res.split("x"))
    d = decision_inputs(w, h, args.bit_depth, args.qp, args.seed, distance=max(1, args.decision_distance))
    planes = [_aligned(p) for p in d["planes"]]
    cl = st.Client("ref", -1)      # -1: everything the CPU supports = the reference's x86 JIT tables
    best = None
    for _ in range(2):
        t0 = time.perf_counter()
        res, field = cl.picture_uni(d["params"], planes[0], planes[1], planes[2], d["stride"], d["pad"], d["pus"], d["ctu_first"], d["cx"], d["cy"], d["mvp_rate"])
        t = time.perf_counter() - t0
        best = t if best is None else min(best, t)
    # the same walk with the bi-directional refinements (searchBi), for the comparison with the device's; timed separately
    t0 = time.perf_counter()
    _, _, bi = cl.picture_uni(d["params"], planes[0], planes[1], planes[2], d["stride"], d["pad"], d["pus"], d["ctu_first"], d["cx"], d["cy"], d["mvp_rate"], bi=True)
    t_bi = time.perf_counter() - t0
    np.savez(args.cpu_out, field=field, seconds_with_bi=t_bi, **{k: res[k] for k in res.dtype.names}, **{"bi_" + k: bi[k] for k in ("mv", "mvd", "mvp_flag", "calls", "cost_subpel")})
    print(json.dumps({"seconds_per_picture": round(best, 4), "pictures_per_second": round(1.0 / best, 3), "cores": 1, "searches": int(len(res)),
                      "loop_calls": int(res["calls"].sum())}))


def cpu_reference_encoder(args):
    """cpu_baseline leg: the reference's own ENCODER (oracle/_ref/turing_ref_havoc: turing/*.cpp compiled where they lie + our driver over
    `Encoder`, x86 JIT havoc) on a synthetic clip of --res -- SURVEY 8(d)'s CPU baseline: whole-encoder frames/s at speed=medium, all host threads"""
    import tempfile
    exe = os.path.join(ROOT, "oracle", "_ref", "turing_ref_havoc")
    if not os.path.exists(exe):
        return None
    from turingcodec_amd.workload import synth_frames
    w, h = (int(v) for v in args.res.split("x"))
    frames = 9 if w * h <= 1920 * 1080 else 5
    cores = usable_cores()
    with tempfile.TemporaryDirectory() as d:
        clip = os.path.join(d, "clip.yuv")
        with open(clip, "wb") as f:
            for planes in synth_frames(w, h, frames, args.seed, args.bit_depth):
                for pl in planes:
                    f.write(np.ascontiguousarray(pl).tobytes())
        cmd = [exe, "--input-res", f"{w}x{h}", "--frames", str(frames), "--frame-rate", "24", "--verbosity", "0", "--no-sao", "--qp", str(args.qp),
               "--speed", "medium", "--threads", str(cores), "-o", os.path.join(d, "out.bit"), clip] + (["--bit-depth", "10"] if args.bit_depth > 8 else [])
        t0 = time.perf_counter()
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        t = time.perf_counter() - t0
        if r.returncode != 0:
            return {"error": r.stderr[-300:]}
        size = os.path.getsize(os.path.join(d, "out.bit"))
    return {"value": round(frames / t, 3), "unit": "frames/s", "frames": frames, "threads": cores, "seconds": round(t, 3), "stream_bytes": size,
            "what": f"the reference encoder itself (whole encoder: search, RDOQ, CABAC, loop filter; x86 JIT havoc), {w}x{h} random access QP{args.qp} "
                    f"speed=medium --no-sao, {frames} frames of the synthetic clip, wall clock of the process (start-up included)"}


def hooked_reference_encoder(args):
    """cpu_baseline leg: the reference ENCODER itself running on the drop-in tables -- oracle/_ref/turing_ref_hooked = the reference's own encoder
    linked against libhavoc_classic.so (every havoc table call answered by the MI355X) with the two picture-registration calls of include/havoc_classic_ext.h -- on a short
    416x240 clip at speed=medium, next to the same encoder over its own x86-JIT havoc library on the same clip: frames/s of both, the share of table calls answered from
    precomputed data, microseconds per table call, and whether the two streams are identical (they must be)."""
    import re
    import tempfile
    hooked = os.path.join(ROOT, "oracle", "_ref", "turing_ref_hooked")
    plain = os.path.join(ROOT, "oracle", "_ref", "turing_ref_havoc")
    if not (os.path.exists(hooked) and os.path.exists(plain)):
        return None
    from turingcodec_amd.workload import synth_frames
    w, h, frames = 416, 240, 3
    with tempfile.TemporaryDirectory() as d:
        clip = os.path.join(d, "clip.yuv")
        with open(clip, "wb") as f:
            for planes in synth_frames(w, h, frames, 7, 8):
                for pl in planes:
                    f.write(np.ascontiguousarray(pl).tobytes())
        out = {}
        for name, exe in (("reference", plain), ("hooked", hooked)):
            bit = os.path.join(d, name + ".bit")
            cmd = [exe, "--input-res", f"{w}x{h}", "--frames", str(frames), "--frame-rate", "24", "--verbosity", "0", "--no-sao", "--qp", "32", "--speed", "medium", "-o", bit, clip]
            t0 = time.perf_counter()
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, HAVOC_CLASSIC_REPORT="1"))
            t = time.perf_counter() - t0
            if r.returncode != 0:
                return {"error": f"{name}: " + r.stderr[-300:]}
            out[name] = (t, open(bit, "rb").read(), r.stderr)
    t_ref, s_ref, _ = out["reference"]
    t_hk, s_hk, err = out["hooked"]
    line = [l for l in err.splitlines() if "table calls served" in l]
    n = [int(v) for v in re.findall(r"\d+", line[-1])] if line else [0, 0, 0]
    calls = max(1, n[0] + n[1])
    by_entry = [l.split("entry point:")[1].strip() for l in err.splitlines() if "one-job launches by entry point" in l]
    return {"value": round(frames / t_hk, 3), "unit": "frames/s", "clip": f"{w}x{h}, {frames} frames (1 I + 2 B), QP32 speed=medium --no-sao", "seconds": round(t_hk, 3),
            "reference_encoder_same_clip_fps": round(frames / t_ref, 3), "stream_identical": bool(s_ref == s_hk), "stream_bytes": len(s_hk),
            "table_calls": calls, "served_fraction": round(n[0] / calls, 4), "one_job_launches": n[1], "launches": n[2], "us_per_table_call": round(t_hk / calls * 1e6, 3),
            "one_job_by_entry_point": by_entry[-1] if by_entry else None,
            "what": "the reference encoder over libhavoc_classic.so (the drop-in table library; the MI355X answers every havoc table call), wall clock of the process"}


def decision_path(args, Havoc, res, bit_depth, qp, pictures, seconds=1.5, keep=None):
    """pictures/s of the decision-driven path (turingcodec_amd/decisions.py): `pictures` independent pictures in flight, each on its own
    context / stream and host thread; plus the latency of ONE picture alone and what its search needed (wavefront steps, rounds, launches)"""
    import threading
    from turingcodec_amd.decisions import DecisionPicture
    w, h = (int(v) for v in res.split("x"))
    cores = usable_cores()
    per = max(1, cores // max(1, pictures))
    ctxs = []
    for k in range(pictures):
        hv = Havoc(0, stream="new")
        ctxs.append(DecisionPicture(hv, w, h, bit_depth, qp, seed=args.seed + 13 * k, threads=per, search_on_device=args.search_client == "device",
                                    distance=max(1, args.decision_distance)))
    for dp in ctxs:
        dp.step()      # allocates the client's pinned work memory, pages code in
    # one picture alone, all replay threads: the latency a dependency-bound encoder sees
    solo = ctxs[0]
    solo.threads = cores
    lat = []
    for _ in range(3):
        t0 = time.perf_counter()
        res0, field0, stats = solo.step()
        lat.append(time.perf_counter() - t0)
    bi_count = int((solo.bi_results["calls"] > 0).sum()) if solo.bi_results is not None else 0
    bi0 = solo.bi_results.copy() if solo.bi_results is not None else None
    t0 = time.perf_counter()
    solo.phase_planes()
    solo.hv.sync()
    t_planes = time.perf_counter() - t0
    t0 = time.perf_counter()
    solo.search()
    t_search = time.perf_counter() - t0
    t0 = time.perf_counter()
    solo.tu_chain(field0)
    solo.hv.sync()
    t_chain = time.perf_counter() - t0
    t0 = time.perf_counter()
    solo.intra_decisions()
    t_intra = time.perf_counter() - t0
    t0 = time.perf_counter()
    solo.merge_candidates(field0)
    solo.chroma_chain(field0)
    solo.hv.sync()
    t_merge = time.perf_counter() - t0
    def throughput(count, secs):
        for dp in ctxs[:count]:
            dp.threads = max(1, cores // count)
        done = [0] * count
        stop = time.perf_counter() + secs

        only_search = os.environ.get("HAVOC_DECISION_PHASES") == "search"      # diagnostic: what the searches alone would reach (profiles/)

        def loop(k):
            while time.perf_counter() < stop:
                if only_search:
                    ctxs[k].phase_planes()
                    ctxs[k].search()
                else:
                    ctxs[k].step()
                done[k] += 1
        t0 = time.perf_counter()
        th = [threading.Thread(target=loop, args=(k,)) for k in range(count)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        return sum(done), time.perf_counter() - t0
    first = max(1, min(pictures, 4))
    ndone, el = throughput(first, seconds)
    done = [ndone]
    more = {}
    for count in sorted({c for c in (8, pictures) if first < c <= pictures}):
        n2, e2 = throughput(count, seconds)
        more["pictures_in_flight_%d" % count] = {"value": round(n2 / e2, 2), "unit": "pictures/s", "host_threads_per_picture": max(1, cores // count),
                                                 "note": "8 = as many independent pictures as the hierarchical-B pipeline has in flight across SOPs (SURVEY 8(e)); "
                                                         "more = several such pipelines (streams) on one device"}
    if args.search_client == "device" and args.decisions == 2:
        # the same picture alone through the launch + host replay client, for comparison
        solo.search_on_device = False
        solo.threads = cores
        solo.search()
        t0 = time.perf_counter()
        _, _, bstats = solo.search()
        more["searches_by_the_batch_client_alone_ms"] = {"value": round((time.perf_counter() - t0) * 1e3, 3), "rounds": int(bstats.rounds), "launches": int(bstats.launches),
                                                         "bytes_down": int(bstats.bytes_down), "replay_threads": cores}
        solo.search_on_device = True
    per, pictures = max(1, cores // first), first
    d = stats.as_dict()
    out = {"value": round(sum(done) / el, 2), "unit": "pictures/s", "pictures_in_flight": pictures, "host_threads": cores, "replay_threads_per_picture": per,
           "hardware_queues": os.environ.get("GPU_MAX_HW_QUEUES"),
           "seconds_measured": round(el, 3), "pictures_done": int(sum(done)),
           "one_picture_alone_ms": round(min(lat) * 1e3, 3),
           "one_picture_alone_split_ms": {"phase_planes": round(t_planes * 1e3, 3), "searches_in_wavefront_order": round(t_search * 1e3, 3),
                                          "prediction_and_transform_tree_decisions": round(t_chain * 1e3, 3),
                                          "intra_35_mode_stage_and_rd_refinement": round(t_intra * 1e3, 3),
                                          "merge_candidates_three_planes_and_chroma_tu_chain": round(t_merge * 1e3, 3)},
           "searches_per_picture": int(2 * len(solo.pus)), "ctus": solo.cx * solo.cy,
           "reference_distance": max(1, args.decision_distance), "loop_calls_per_search": round(float(res0["calls"].mean()), 1),
           "bi_directional_refinements_per_picture": bi_count,
           "transform_tree_decisions": {"units": int(len(solo.units)), "candidates": int(solo.rqt_stats.candidates), "launches": int(solo.rqt_stats.launches),
                                        "launches_per_ctu": round(solo.rqt_stats.launches / (solo.cx * solo.cy), 4),
                                        "split": int((solo.rqt_results["depth"] == 1).sum()), "unsplit": int(((solo.rqt_results["depth"] == 0) & (solo.rqt_results["tried_zero"] == 1)).sum()),
                                        "uncoded": int((solo.rqt_results["tried_zero"] == 0).sum()),
                                        "seconds": {"gpu": round(solo.rqt_stats.seconds_gpu, 5), "host": round(solo.rqt_stats.seconds_host, 5)}},
           "intra": {"partitions": int(sum(len(g["jobs"]) for g in solo.intra_parts.values())),
                     "candidates_reconstructed": int(sum(st.candidates for st in solo.intra_stats)),
                     "launches": int(sum(st.launches for st in solo.intra_stats)),
                     "decisions": "on the device (order of refinement, candidates' job records, champions): 40 bytes per partition come back",
                     "champion_is_not_the_satd_winner": round(float(np.mean(np.concatenate([b["index"] != 0 for _, b in solo.intra_results.values()]))), 3)},
           "wavefront_steps": d["steps"], "rounds": d["rounds"], "rounds_per_step": round(d["rounds"] / max(1, d["steps"]), 2),
           "max_rounds_in_step": d["max_rounds_in_step"], "launches": d["launches"], "launches_per_step": round(d["launches"] / max(1, d["steps"]), 2),
           "surfaces": d["surfaces_small"] + d["surfaces_zero"] + d["surfaces_large"], "satd_jobs": d["satd_jobs"],
           "searches_run_ahead_on_a_guess": d["speculative_runs"], "searches_rerun": d["reruns"], "bytes_down": d["bytes_down"],
           "client_seconds": {"gpu_rounds": round(d["seconds_gpu"], 5), "host_replay": round(d["seconds_host"], 5), "total": round(d["seconds_total"], 5)},
           "search_client": ("decision loops inside the kernel (csrc/kernels_search.hip: search/decision.hpp compiled for gfx950; a workgroup per (CTU row, list) "
                             "waits for the row above inside ONE launch; window, source block and neighbour vectors in LDS); only the results come back"
                             if args.search_client == "device" else "SAD-surface / tile-SATD batch launches, the reference's loops replayed on host threads"),
           "what": ("per picture (its two references at temporal distance %d -- 1 = the leaf B pictures, half of a SOP of 8; the upper layers' searches are "
                   "2.5 - 3 x longer: see the distance-4 entry): 2 x 15 phase planes; every PU's uni-directional search in both lists, CTUs in WPP wavefront order (CTU (x, y) after "
                   "(x + 1, y - 1)), predictors of a PU = the vectors decided for its left / upper neighbours, mvPreviousInteger2Nx2N handed along the CTU "
                   "row (turingcodec_amd/search/picture_order.hpp), then the bi-directional refinement of every PU (searchBi: list 0 against list 1's "
                   "vector, list 1 against list 0's refined one; device search only); the five spatial merge candidates of every unit predicted bi-directionally in three planes and "
                   "measured (SATD; vectors from the decided field, Mvp.h's derivation out of scope); then prediction at the chosen vectors and the residual-quadtree decision of every inter unit (both tree depths of "
                   "every 32x32 unit through residual + DCT -> RDOQ -> IQ + IDCT + add -> SSD in one chain per transform size, decisions from 16 bytes per "
                   "candidate, chosen candidates reconstructed into the picture; turingcodec_amd/search/tu_decision.hpp), the chroma planes' prediction (4-tap) and TU chain at the same vectors, boundary strengths derived on "
                   "the device, deblocking, padding; and the picture's intra candidates (42 partitions per CTU: 35-mode SATD stage, then every candidate "
                   "mode of the refinement order reconstructed through T -> RDOQ -> IT and the champion picked; neighbours from the source picture, not "
                   "from the preceding partition's reconstruction). Not in it: the mode decision between the searched PUs (uni / bi / merge) and between "
                   "inter and intra, CABAC (the rate terms of the tree / intra decisions are stand-ins)") % max(1, args.decision_distance)}
    out.update(more)
    if keep is not None:
        keep["solo"], keep["res"], keep["field"], keep["bi"] = solo, res0, field0, bi0
    else:
        for dp in ctxs:
            dp.hv.close()
    return out


def decision_children(args):
    """the decision-driven path of --res / --qp and of 4K QP32, each in a process of its own (16 hardware queues: see the top of this file), run BEFORE
    this process touches the device so that nothing else holds queues or memory while they are measured"""
    paths, walk = {}, None
    main_label = f"decision-driven path {args.res} {args.bit_depth}-bit QP{args.qp}"
    jobs = [(args.res, args.qp, 1, main_label)]
    jobs += [(args.res, args.qp, d, f"{main_label}, references at temporal distance {d} (an upper layer of the hierarchy: longer vectors, more calls per search)") for d in (2, 4, 8)]
    if args.res != "3840x2160":
        k4 = "decision-driven path 3840x2160 8-bit QP32 (BASELINE.json metric: 4K RA QP32)"
        jobs += [("3840x2160", 32, 1, k4)] + [("3840x2160", 32, d, f"{k4}, references at temporal distance {d}") for d in (2, 4, 8)]
    for dres, dqp, dist_, label in jobs:
        try:
            # every timed decision-path figure carries its own comparison with the walk over the reference's tables: the whole
            # picture, every search, through the x86-JIT tables on one core (a second or two even at 4K)
            want_walk = not args.no_cpu_baseline
            primary = dist_ == 1 and dres == args.res
            cmd = [sys.executable, os.path.abspath(__file__), "--decisions", "2", "--res", dres, "--bit-depth", str(args.bit_depth if dres == args.res else 8),
                   "--qp", str(dqp), "--seed", str(args.seed), "--decision-pictures", str(max(1, args.decision_pictures) if primary else 8),
                   "--search-client", args.search_client, "--decision-distance", str(dist_), "--decision-walk", "1" if want_walk else "0"]
            child = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if child.returncode != 0:
                raise RuntimeError(child.stderr[-600:])
            got = json.loads([l for l in child.stdout.splitlines() if l.startswith("{")][-1])
            paths[label] = got["decision_driven_path"]
            w_ = got.get("decision_walk")
            if want_walk and w_:
                paths[label]["parity_vs_reference"] = w_.get("parity_vs_reference", w_)
                paths[label]["one_cpu_core_through_the_reference_tables_pictures_per_second"] = w_.get("pictures_per_second")
                if primary:
                    walk = w_
        except Exception as e:
            paths[label] = {"error": repr(e)}
    # the 8-picture SOP of the hierarchy: four pictures at distance 1, two at 2, one at 4, one at 8 (turing/InputQueue.cpp:370-379) -- measured rates, 8 in flight
    for res_key, base in ((args.res, main_label), ("3840x2160", "decision-driven path 3840x2160 8-bit QP32 (BASELINE.json metric: 4K RA QP32)")):
        try:
            def rate(d):
                key = base if d == 1 else [k for k in paths if k.startswith(base + ",") and k.split("distance ")[1].split(" ")[0] == str(d)][0]
                r = paths[key]
                return r.get("pictures_in_flight_8", {}).get("value") or r["value"]
            rates = {d: rate(d) for d in (1, 2, 4, 8)}
            paths[base]["sop_weighted"] = {"value": round(8.0 / (4 / rates[1] + 2 / rates[2] + 1 / rates[4] + 1 / rates[8]), 2), "unit": "pictures/s",
                                           "rates_by_reference_distance": rates,
                                           "what": "harmonic mean over one SOP of 8 (4 x distance 1, 2 x distance 2, distance 4, distance 8), each rate measured with 8 pictures in flight"}
        except Exception:
            pass
    return {"paths": paths, "walk": walk}


def main():
    args = parse_args()
    if args.cpu_worker == "decisions":
        return cpu_decision_worker(args)
    if args.cpu_worker:
        return cpu_worker(args)
    early = {}
    if (args.full and args.decisions == 1 and args.gpus == 1 and int(os.environ.get("WORLD_SIZE", "1")) == 1 and args.mix == "ra"
            and not (args.pcie or args.skip or args.no_graph)):
        early = decision_children(args)
    import torch
    import torch.distributed as dist
    from turingcodec_amd import Havoc
    from turingcodec_amd.workload import FrameWorkload

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the N ranks ourselves (one process per GPU over RCCL, as the driver's
        # `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N` does) and hand over to them
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1", "--master-port", str(port),
               os.path.abspath(__file__)] + sys.argv[1:]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        sys.exit(subprocess.call(cmd, env=env))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != max(1, args.gpus):
        sys.stderr.write(f"bench.py: --gpus {args.gpus} but the launcher started {world} rank(s) (WORLD_SIZE): the line would not be what was asked for\n")
        sys.exit(2)
    if args.decisions == 4:      # one sequence with its picture dependencies, K virtual ranks on this GPU
        return decision_virtual_ranks(args, torch, Havoc)
    if args.decisions == 2:      # only the decision-driven path of --res / --qp, one line (also how a --full run measures it: see the top of this file)
        keep = {} if args.decision_walk else None
        r = decision_path(args, Havoc, args.res, args.bit_depth, args.qp, max(1, args.decision_pictures), seconds=(1.0 if args.decision_pictures <= 8 else 1.5), keep=keep)
        line = {"metric": "DIAGNOSTIC (decision-driven path only) -- not the benchmark metric", "value": r["value"], "unit": r["unit"],
                "config": {"workload": f"{args.res} {args.bit_depth}-bit QP{args.qp}"}, "decision_driven_path": r}
        if args.decision_walk:
            try:
                line["decision_walk"] = cpu_decision_walk(args, keep)
            except Exception as e:
                line["decision_walk"] = {"error": repr(e)}
        print(json.dumps(line), flush=True)
        return
    grouped = world > 1 or args.exchange
    if grouped:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:   # single-rank --exchange run: any free port
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        backend = os.environ.get("HAVOC_BENCH_BACKEND", "nccl")   # "gloo": rehearsal of the N>1 path on a 1-GPU box
        local %= torch.cuda.device_count()
        torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    if args.decisions == 3:
        decision_frame_parallel(args, torch, dist, Havoc, rank, world, local)
        if grouped:
            dist.barrier()
            dist.destroy_process_group()
        return
    w, h = (int(v) for v in args.res.split("x"))
    inflight = 1 if (args.pcie or args.no_graph or args.poc_checksums) else max(1, args.inflight)
    # Step i runs picture context i % inflight.  Single GPU: every context owns a different synthetic picture.  Frame-parallel:
    # the contexts of every rank are built from the same seeds (a picture's result must not depend on who encodes it).
    slots = build_contexts(args, torch, Havoc, FrameWorkload, local, args.res, args.bit_depth, args.qp, args.mix,
                           args.seed + (0 if grouped else rank), inflight, args.tune)
    compute, hv, wl, dev, graph = slots[0]
    if args.traffic_child:      # hbm_traffic_in_run's child under rocprofv3 --pmc: build_contexts ran the step once; the rest, then nothing else
        for _ in range(args.traffic_child - 1):
            dev.step()
        hv.sync()
        return
    pipe = None
    if grouped:
        from turingcodec_amd.frame_parallel import DagSchedule, ReferenceExchange
        strong = args.scaling == "strong"
        sched = DagSchedule(world, n_sops=(args.pictures - 1) // 8 if strong else None, lag=args.lag or None)
        exch = ReferenceExchange(dist, rank, sched, wl.plane_len, wl.cplane_len, dev.luma, single_rank_broadcast=args.exchange)
        if args.bands > 0:
            from turingcodec_amd.frame_parallel import BandPlan
            exch.set_bands(BandPlan(wl.height, 96, wl.stride, wl.cstride, band_ctu_rows=args.bands))
        comm = torch.cuda.current_stream(local)   # torch.distributed enqueues behind this stream
        pipe = FramePipeline(torch, dist, exch, slots, rank, comm, args.lanes, poc_checksums=args.poc_checksums)

    host_io = None
    if args.pcie:
        # what a host-side encoder exchanges per picture: up = source planes, every job table, the levels its RDOQ
        # produced; down = every cost the decision loops read, the coefficients RDOQ needs, the TU SSDs.  Reference
        # pictures and reconstructions stay on the device.  Pinned staging buffers, async copies on the compute stream.
        ups = [dev.luma[:wl.plane_len], dev.chroma[:wl.cplane_len], dev.j_sad4, dev.j_sad, dev.j_sbi, dev.j_satd]
        ups += [g["jobs"] for g in dev.subpel_planes.values()] + [g["jobs"] for g in dev.isearch.values()] + [g["jobs"] for g in dev.intra.values()]
        ups += [g["nb"] for g in dev.isearch.values()] + [g["nb"] for g in dev.intra.values()]
        # (with RDOQ on the device neither the coefficients nor the levels cross the link: only the coded-block flags come down)
        ups += [t for g in dev.tu.values() for t in ((g["fjobs"],) if dev.rdoq else (g["fjobs"], g["level"]))]
        downs = [dev.o_sad4, dev.o_sad, dev.o_satd] + [g["cost"] for g in dev.subpel_planes.values()] + [g["cost"] for g in dev.isearch.values()]
        downs += [t for g in dev.tu.values() for t in ((g["cbf"], g["ossd"]) if dev.rdoq else (g["coef"], g["ossd"]))]
        host_io = ([(t, torch.empty_like(t, device="cpu").pin_memory()) for t in ups],
                   [(t, torch.empty_like(t, device="cpu").pin_memory()) for t in downs])
        for t, hb in host_io[0]:
            hb.copy_(t)
        pcie_bytes = (sum(t.numel() * t.element_size() for t in ups), sum(t.numel() * t.element_size() for t in downs))

    def one_step(i):
        if pipe is not None:
            return pipe.slot(i)
        compute, hv, wl, dev, graph = slots[i % inflight]
        if host_io is not None:
            with torch.cuda.stream(compute):
                for t, hb in host_io[0]:
                    t.copy_(hb, non_blocking=True)
        if graph is not None:
            hv.graph_launch(graph)
        else:
            dev.step(args.lanes)
        if host_io is not None:
            with torch.cuda.stream(compute):
                for t, hb in host_io[1]:
                    hb.copy_(t, non_blocking=True)

    if pipe is not None and args.scaling == "strong":
        # strong scaling: a FIXED sequence (IDR + SOPs, --pictures) from the first slot to the last, fill and drain of the
        # pipeline included; a step = one time slot, the timed region = the whole sequence, `steps` is set to its slot count
        nslots = sched.slots_for_sequence()
        args.steps, args.warmup = nslots, 0

        def run_block(_b):
            for i in range(nslots):
                one_step(i)
        # one untimed pass over the sequence first (code objects, RCCL channels), on a schedule of its own
        warm = FramePipeline(torch, dist, ReferenceExchange(dist, rank, DagSchedule(world, n_sops=(args.pictures - 1) // 8, lag=args.lag or None), wl.plane_len,
                                                            wl.cplane_len, dev.luma, single_rank_broadcast=args.exchange), slots, rank, comm, args.lanes)
        for i in range(nslots):
            warm.slot(i)
        blocks = timed_blocks(torch, dist, world, nslots, 0.0, run_block, max_blocks=1)
        pictures_per_block = args.pictures
    else:
        base = [0]
        prime = 0
        if pipe is not None and world > 1:
            # weak scaling measures the steady state of an endless sequence: first run the pipeline's fill (the slots before every
            # rank has a picture two slots running: 6 with lag 1, 14 with lag 2 on 8 ranks) -- untimed, like the warm-up steps
            while prime < 64 and not (all(p is not None for p in sched.slot(prime)) and all(p is not None for p in sched.slot(prime + 1))):
                prime += 1
            for i in range(prime):
                one_step(i)
        for i in range(args.warmup):
            one_step(prime + i)
        base[0] = prime + args.warmup

        def run_block(_b):
            for i in range(args.steps):
                one_step(base[0] + i)
            base[0] += args.steps
        before = pipe.pictures if pipe is not None else 0
        blocks = timed_blocks(torch, dist, world, args.steps, args.min_seconds or 0.0, run_block)
        # frame-parallel steady state: every rank works on one picture per slot (DagSchedule); counted, not assumed
        if pipe is not None:
            n = torch.tensor([pipe.pictures - before], device="cuda", dtype=torch.float64)
            if world > 1:
                dist.all_reduce(n)
            pictures_per_block = float(n.item()) / len(blocks)
        else:
            pictures_per_block = float(world * args.steps)
    dumped = None
    if args.dump_outputs and rank == 0:
        # what the last timed step computed (its picture context), before the kernel times, counter passes and extras below launch again
        last = (pipe.count - 1) % len(slots) if pipe is not None else (base[0] - 1) % inflight
        dumped = dump_outputs(torch, slots[last][3], args.dump_outputs)
    blk = float(np.median(blocks))
    elapsed = blk
    all_poc = None
    if args.poc_checksums and pipe is not None:      # every rank's pictures, collected on all ranks (rank 0 reports them)
        all_poc = dict(pipe.poc_checksums)
        if world > 1:
            parts = [None] * world
            dist.all_gather_object(parts, pipe.poc_checksums)
            for d in parts:
                all_poc.update(d)

    if rank == 0:
        ms_step = elapsed / args.steps * 1e3
        figures = kernel_figures(args, dev, wl, world, ms_step) if args.full else {}
        mixname = ("random-access QP%d speed=medium B-frame, MEASURED call mix of the reference encoder on this clip generator (profiles/r04_reference_call_mix_1080p.json: "
                   "call counts x %.2f by CTU count; measured block sizes, phase classes, DCT / DST split)" % (args.qp, ((w + 63) // 64) * ((h + 63) // 64) / 510.0)
                   if args.mix == "ra" else "all-intra QP%d speed=fast call mix (SURVEY A.1 per-CTU intra / TU counts, havoc_quantize in the chain)" % args.qp)
        out = {
            "metric": "encoded fps (havoc hot path, primitive-batch throughput: one picture's primitive calls per frame as whole-frame batches; "
                      "the decision-driven path is in extra)",
            "value": round(pictures_per_block / elapsed, 3),
            "unit": "frames/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_step, 4),
            "higher_is_better": True, "scaling": args.scaling if pipe is not None else "weak", "vs_baseline": None,
            "dtype": "u8" if args.bit_depth == 8 else "u16", "data": "synthetic" if not args.yuv else f"file {os.path.basename(args.yuv)} (job tables synthetic)",
            "config": {"workload": f"{args.res} {args.bit_depth}-bit 4:2:0 {mixname}, 1xMI355X per rank",
                       "calls_per_frame": int(sum(wl.counts.values())), "launches_per_frame": len(dev.launches), "pictures_in_flight": inflight,
                       "integer_me": ("sad4 jobs (the reference's per-pattern calls)" if args.ime == "sad4" else
                                      f"{len(wl.me_search)} SAD surfaces of (2*{args.ime_range}+1)^2 candidates instead of "
                                      f"{len(wl.sad4)} SAD4 calls"),
                       "quantiser": ("Rdoq::runQuantisation on the device between tu_forward and tu_reconstruct (speed=medium has RDOQ on)" if dev.rdoq else
                                     "havoc_quantize in the chain (speed=fast)" if args.mix == "ai" else "levels pre-computed once, untimed (--rdoq 0)"),
                       "parallelism": "single GPU"},
            "timing": {"timed_blocks": len(blocks), "block_seconds_median": round(blk, 6), "block_seconds_min": round(min(blocks), 6),
                       "block_seconds_max": round(max(blocks), 6), "seconds_measured": round(sum(blocks), 4),
                       "note": f"each block = exactly {args.steps} steps between barrier + synchronize; ms_per_step and value are the MEDIAN block"},
            **figures,
        }
        if dumped is not None:
            out["outputs_dumped"] = {"dir": args.dump_outputs, "elements_written_of_buffer": dumped}
        if pipe is not None:
            out["config"]["parallelism"] = (
                f"frame-parallel x{world}: hierarchical-B docket (turing/InputQueue.cpp:370-379) list-scheduled on {world} ranks "
                f"(a picture starts after the broadcasts of its references; references are read from the DPB mirror), "
                f"{pipe.exch.broadcasts} reference pictures broadcast over {'RCCL' if os.environ.get('HAVOC_BENCH_BACKEND', 'nccl') == 'nccl' else 'gloo'} "
                f"in the whole run ({pipe.exch.sent_bytes} B sent by rank 0), overlapped with the next slot"
                + (f"; strong scaling over a fixed {args.pictures}-picture sequence, fill and drain included" if args.scaling == "strong" else
                   f"; weak scaling: steady state of an endless sequence, one picture per rank per slot (schedule lag {sched.lag}, {prime} untimed pipeline-fill slots before the warm-up)"))
            out["config"]["pictures_per_timed_block"] = pictures_per_block
            out["config"]["parallelism_short"] = (f"frame-parallel x{world} over {'RCCL' if os.environ.get('HAVOC_BENCH_BACKEND', 'nccl') == 'nccl' else 'gloo'}, "
                                                  f"{pipe.exch.broadcasts} reference pictures broadcast, {args.scaling} scaling, lag {sched.lag}")
        if args.poc_checksums and pipe is not None:
            out["poc_checksums"] = {str(k): v for k, v in sorted(all_poc.items())}
        if args.pcie:
            out["metric"] = (f"DIAGNOSTIC (PCIe-inclusive: {pcie_bytes[0]} B up, {pcie_bytes[1]} B down per step, serial with the "
                             "kernels) -- not the benchmark metric")
        if args.skip:
            out["metric"] = "DIAGNOSTIC (launch groups skipped: " + args.skip + ") -- not the benchmark metric"
        # the side measurements of --full around the undiagnostic single-GPU step
        extras = args.full and world == 1 and pipe is None and not (args.pcie or args.skip or args.no_graph)
        if extras and args.extra_4k and args.res == "1920x1080" and args.mix == "ra":
            # BASELINE.json configs[2] and [3] (the resolution the north star's target is quoted on, 8- and 10-bit), same code, fewer steps
            for xbd, xqp, label in ((8, 27, "3840x2160 8-bit random-access QP27 speed=medium (BASELINE.json configs[2])"),
                                    (10, 27, "3840x2160 10-bit Main10 random-access QP27 speed=medium (BASELINE.json configs[3])"),
                                    (8, 32, "3840x2160 8-bit random-access QP32 speed=medium (BASELINE.json metric: 4K RA QP32)")):
                try:
                    xs = build_contexts(args, torch, Havoc, FrameWorkload, local, "3840x2160", xbd, xqp, "ra", args.seed + 77, inflight, min(args.tune, 8))
                    ksteps = 20

                    def xblock(_b, xs=xs):
                        for i in range(ksteps):
                            xs[i % len(xs)][1].graph_launch(xs[i % len(xs)][4])
                    xblock(0)
                    xb = timed_blocks(torch, dist, 1, ksteps, 0.3, xblock)
                    out.setdefault("extra", {})[label] = {
                        "value": round(ksteps / float(np.median(xb)), 3), "unit": "frames/s", "ms_per_step": round(float(np.median(xb)) / ksteps * 1e3, 4),
                        "steps": ksteps, "timed_blocks": len(xb), "calls_per_frame": int(sum(xs[0][2].counts.values())), "checksum": xs[0][3].checksum()}
                    del xs
                    torch.cuda.empty_cache()
                except Exception as e:   # the headline line stands on its own
                    out.setdefault("extra", {})[label] = {"error": repr(e)}
            if args.rdoq:
                # round 1's step for continuity: the same picture with the levels made once, untimed, by havoc_quantize (--rdoq 0)
                try:
                    import copy
                    a0 = copy.copy(args)
                    a0.rdoq = 0
                    xs = build_contexts(a0, torch, Havoc, FrameWorkload, local, args.res, args.bit_depth, args.qp, "ra", args.seed, inflight, min(args.tune, 8))
                    ksteps = 50

                    def yblock(_b, xs=xs):
                        for i in range(ksteps):
                            xs[i % len(xs)][1].graph_launch(xs[i % len(xs)][4])
                    yblock(0)
                    yb = timed_blocks(torch, dist, 1, ksteps, 0.3, yblock)
                    out.setdefault("extra", {})["same picture without RDOQ in the timed chain (--rdoq 0: round 1's step)"] = {
                        "value": round(ksteps / float(np.median(yb)), 3), "unit": "frames/s", "ms_per_step": round(float(np.median(yb)) / ksteps * 1e3, 4),
                        "steps": ksteps, "timed_blocks": len(yb)}
                except Exception as e:
                    out.setdefault("extra", {})["rdoq0_error"] = repr(e)
        if extras and args.mix == "ra":
            # the same step with ONE picture in flight, a synchronisation after every picture: the latency a caller sees that needs a picture's
            # results before it can issue the next one
            try:
                hv1, g1 = slots[0][1], slots[0][4]
                lat = []
                for _ in range(40):
                    t0 = time.perf_counter()
                    hv1.graph_launch(g1)
                    hv1.sync()
                    lat.append(time.perf_counter() - t0)
                lat = sorted(lat)[:30]
                out.setdefault("extra", {})["same step, one picture in flight and a synchronisation per picture (latency)"] = {
                    "ms_per_picture": round(float(np.median(lat)) * 1e3, 4), "value": round(1.0 / float(np.median(lat)), 2), "unit": "frames/s",
                    "launches_per_picture": len(dev.launches)}
            except Exception as e:
                out.setdefault("extra", {})["one_in_flight_error"] = repr(e)
        if extras and args.decisions and args.mix == "ra":
            # the decision-driven path: what the batches cost when decisions sit between them
            decision_walk = early.get("walk")
            for label, r in early.get("paths", {}).items():
                if "error" not in r and label == f"decision-driven path {args.res} {args.bit_depth}-bit QP{args.qp}":
                    r["ratio_to_value"] = round(r["value"] / out["value"], 5)
                    r["ratio_note"] = ("`value` is one picture's primitive calls as ideal whole-frame batches (no decision between launches); this is the "
                                       "same kernels driven by decisions in an order a bit-exact encoder could issue them")
                out.setdefault("extra", {})[label] = r
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args, dev)
            if extras and args.decisions and args.mix == "ra" and out["cpu_baseline"] is not None:
                out["cpu_baseline"]["decision_walk"] = decision_walk
                try:
                    enc = cpu_reference_encoder(args)
                except Exception as e:
                    enc = {"error": repr(e)}
                if enc and "value" in enc:
                    # the defensible CPU figure is the reference ENCODER's own frames/s; the per-primitive table timing
                    # (a harness: one C loop per job table, Rdoq objects built per block) stays as a breakdown and as the source of the parity check
                    tables = {k: out["cpu_baseline"].pop(k) for k in ("value", "unit", "cores", "kind", "ms_per_frame_by_group", "what", "sample")}
                    out["cpu_baseline"].update({"value": enc["value"], "unit": "frames/s", "cores": enc["threads"], "kind": "reference",
                                                "sample": enc["what"] + f" ({enc['seconds']} s)", "reference_encoder": enc, "primitive_tables": tables})
                else:
                    out["cpu_baseline"]["reference_encoder"] = enc
                try:
                    out["cpu_baseline"]["hooked_encoder"] = hooked_reference_encoder(args)
                except Exception as e:
                    out["cpu_baseline"]["hooked_encoder"] = {"error": repr(e)}
        red = parity_problems(out)
        if args.full:      # (a plain run compares nothing with the reference, so it states no parity)
            out["parity"] = "red" if red else "green"
            if red:
                out["parity_problems"] = red
        short = compact_line(out, args)
        line = json.dumps(short)
        for drop in ("poc_checksums", "whole_step", "extra", "timing"):      # the line must stay parseable by the driver whatever a run adds to it: shed the least needed first
            if len(line) < 7800:
                break
            short.pop(drop, None)
            line = json.dumps(short)
        if args.detail_out:
            try:
                os.makedirs(os.path.dirname(os.path.abspath(args.detail_out)), exist_ok=True)
                with open(args.detail_out, "w") as f:
                    json.dump(out, f, indent=1)
            except OSError as e:
                sys.stderr.write(f"bench.py: could not write {args.detail_out}: {e}\n")
    if grouped:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        sys.stdout.flush()
        sys.stderr.flush()
        print(line, flush=True)     # the ONE JSON line, after anything the collective library may still say
        if red:                     # a result that differs from the reference's is not a benchmark result (VERDICT r4 next #1a)
            sys.stderr.write("bench.py: PARITY RED -- " + "; ".join(red)[:2000] + "\n")
            sys.exit(3)


if __name__ == "__main__":
    main()
