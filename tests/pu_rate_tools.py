"""The rate measurePuCost measures for one candidate of a prediction unit (turing/Search.hpp:1656-1706: Syntax<prediction_unit>, turing/SyntaxCtu.hpp:267-314, under
Measure<void>) restated on the CPU in plain Python, in the syntax's order, and go2's comparison (Search.hpp:1829-1902) in numpy.  Test infrastructure.

Rates are integers (Cost = FixedPoint<int64_t, 16>): a context-coded bin costs measureEncodeDecision (sao_merge_tools.bin_cost: the tables of
turingcodec_amd/csrc/cabac_tables.h, which the device uses too) and moves its context, a bypass bin 1 << 16.  `pu_rate` counts the branches it takes in `tags` (a
collections.Counter).  `Shim` compiles tests/pu_rate_shim.cpp -- the reference's own syntax function and writers over a stand-in handle -- into a temporary directory;
`DecisionClient` compiles tests/pu_decide_client.cpp (search/pu_decision.hpp's decidePu).  `make_cases` makes the candidates of one slice: a systematic part that reaches
every branch, a random part, and one job per refusal.
"""
import collections
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import sao_decision_tools as T
from sao_merge_tools import bin_cost

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# include/havoc_mi355x.h: HAVOC_PU_SYNTAX_CTX_*
MERGE_FLAG, MERGE_IDX, INTER_PRED_IDC, REF_IDX, GREATER0, GREATER1, MVP_FLAG, SYNTAX_BYTES = 0, 1, 2, 7, 9, 10, 11, 16
MERGE, SKIP = 1, 2                  # HAVOC_PU_RATE_*
L0, L1, BI = 0, 1, 2                # HAVOC_PU_PRED_*
BYPASS = 1 << 16

Slice = collections.namedtuple("Slice", "slice_b max_num_merge_cand mvd_l1_zero_flag num_ref_idx_l0 num_ref_idx_l1")
# the slices of the golden file and the fresh cases: B and P, every MaxNumMergeCand 1..5, mvd_l1_zero_flag, one and several reference pictures per list
SLICES = [Slice(1, 5, 0, 0, 0), Slice(1, 4, 1, 0, 0), Slice(1, 3, 0, 1, 3), Slice(1, 2, 1, 15, 2), Slice(1, 1, 0, 0, 1), Slice(0, 5, 0, 0, 0), Slice(0, 1, 0, 2, 0),
          Slice(0, 3, 0, 0, 0), Slice(0, 2, 0, 0, 0), Slice(0, 4, 0, 5, 0)]
REFUSALS = ("flag_bit", "merge_idx", "bi_small", "pred", "pred_in_p_slice", "cqt_depth", "mvp_flag", "ref_idx")


def refusal(job, sl):
    """why havoc_mi355x_pu_rate does not walk the job (include/havoc_mi355x.h), or None"""
    flags, pred = int(job["flags"]), int(job["pred"])
    if flags & ~(MERGE | SKIP):
        return "flag_bit"
    if flags & (MERGE | SKIP):
        return "merge_idx" if int(job["merge_idx"]) >= sl.max_num_merge_cand else None
    if pred > 2:
        return "pred"
    if int(job["cqt_depth"]) > 3:
        return "cqt_depth"
    if pred == BI and int(job["w"]) + int(job["h"]) == 12:
        return "bi_small"
    if not sl.slice_b and pred != L0:
        return "pred_in_p_slice"
    for l in (0, 1):
        if pred != 1 - l:
            if int(job["mvp_flag"][l]) > 1:
                return "mvp_flag"
            if int(job["ref_idx"][l]) > sl[3 + l]:
                return "ref_idx"
    return None


def eg1_bins(v):
    """Binarization.h:767-798: the number of bypass bins of abs_mvd_minus2 = v, by the writer's own loop"""
    k, n = 1, 0
    while v >= (1 << k):
        n += 1
        v -= 1 << k
        k += 1
    return n + 1 + k


def pu_rate(job, sl, syn, tags=None):
    """Syntax<prediction_unit>::go for one valid job; syn: list of 16 context states, updated in place -> the Q16 rate"""
    tags = collections.Counter() if tags is None else tags
    rate = 0

    def decision(ctx, b):
        nonlocal rate
        syn[ctx], r = bin_cost(syn[ctx], int(b))
        rate += r

    def bypass(n):
        nonlocal rate
        rate += n * BYPASS

    def write_merge_idx():
        if sl.max_num_merge_cand > 1:
            c_max, v = sl.max_num_merge_cand - 1, int(job["merge_idx"])
            for i in range(v):
                decision(MERGE_IDX, 1) if i == 0 else bypass(1)
            if v < c_max:
                decision(MERGE_IDX, 0) if v == 0 else bypass(1)
            tags["merge_idx_last" if v == c_max else "merge_idx_terminated"] += 1
        else:
            tags["merge_idx_not_coded"] += 1

    def mvd_coding(l):
        a = [abs(int(v)) for v in job["mvd"][l]]
        decision(GREATER0, a[0] > 0)
        decision(GREATER0, a[1] > 0)
        if a[0] > 0:
            decision(GREATER1, a[0] > 1)
        if a[1] > 0:
            decision(GREATER1, a[1] > 1)
        for c in (0, 1):
            tags["mvd", c, min(a[c], 4), int(job["mvd"][l][c]) < 0] += 1
            if a[c] > 0:
                if a[c] > 1:
                    bypass(eg1_bins(a[c] - 2))
                    tags["eg1_bins", eg1_bins(a[c] - 2)] += 1
                bypass(1)

    flags, pred = int(job["flags"]), int(job["pred"])
    tags["slice", "B" if sl.slice_b else "P"] += 1
    if flags & SKIP:
        tags["merge", sl.max_num_merge_cand, int(job["merge_idx"]), "skip"] += 1
        write_merge_idx()
        return rate
    decision(MERGE_FLAG, bool(flags & MERGE))
    if flags & MERGE:
        tags["merge", sl.max_num_merge_cand, int(job["merge_idx"]), "merge"] += 1
        write_merge_idx()
        return rate
    small = int(job["w"]) + int(job["h"]) == 12
    if sl.slice_b:
        if not small:
            decision(INTER_PRED_IDC + int(job["cqt_depth"]), pred == BI)
            if pred != BI:
                decision(INTER_PRED_IDC + 4, pred)
            tags["pred", pred, int(job["cqt_depth"])] += 1
        else:
            decision(INTER_PRED_IDC + 4, pred)
            tags["small", int(job["w"]), int(job["h"]), pred] += 1
    for l in (0, 1):
        if pred == 1 - l:
            continue
        c_max = sl[3 + l]
        tags["num_ref_idx", l, c_max > 0] += 1
        if c_max > 0:
            v = int(job["ref_idx"][l])
            for i in range(v + (v < c_max)):
                b = 1 if i < v else 0
                decision(REF_IDX + i, b) if i < 2 else bypass(1)
            tags["ref_idx_bins", min(v + (v < c_max), 3)] += 1
        if l == 1 and pred == BI and sl.mvd_l1_zero_flag:
            tags["mvd_l1_zero_bi"] += 1
        else:
            mvd_coding(l)
        decision(MVP_FLAG, int(job["mvp_flag"][l]))
    return rate


def walk_jobs(jobs, sl, states, tags=None):
    """havoc_mi355x_pu_rate by the restatement -> (rates int64 [max out_index + 1], snapshots after uint8 [njobs, 16], refusal reason per job)"""
    tags = collections.Counter() if tags is None else tags
    nr = int(jobs["out_index"].max()) + 1 if len(jobs) else 0
    rates, after, why = np.zeros(nr, np.int64), np.zeros((len(jobs), SYNTAX_BYTES), np.uint8), []
    for j, job in enumerate(jobs):
        syn = [int(v) for v in states[int(job["ctx_index"])]]
        r = refusal(job, sl)
        why.append(r)
        if r is None:
            rates[int(job["out_index"])] = pu_rate(job, sl, syn, tags)
        else:
            rates[int(job["out_index"])] = -1
            tags["refused", r] += 1
        after[j] = syn
    return rates, after, why


def required_tags(sl):
    """the branches the made cases of a slice must reach"""
    M = sl.max_num_merge_cand
    out = [("slice", "B" if sl.slice_b else "P")]
    out += [("merge", M, i, how) for i in range(M) for how in ("merge", "skip")]
    out += ["merge_idx_not_coded"] if M == 1 else ["merge_idx_last", "merge_idx_terminated"]
    preds = (L0, L1, BI) if sl.slice_b else (L0,)
    if sl.slice_b:
        out += [("pred", p, d) for p in preds for d in range(4)]
        out += [("small", w, h, p) for w, h in ((8, 4), (4, 8)) for p in (L0, L1)]
        out += ["mvd_l1_zero_bi"] if sl.mvd_l1_zero_flag else []
    out += [("mvd", c, a, neg) for c in (0, 1) for a in range(5) for neg in ((False,) if a == 0 else (False, True))]
    out += [("eg1_bins", n) for n in range(2, 31, 2)]          # |mvd| - 2 from 0 to 32766: every prefix length
    for l in (0, 1) if sl.slice_b else (0,):
        out += [("num_ref_idx", l, sl[3 + l] > 0)]
    if sl.num_ref_idx_l0 > 0 or (sl.slice_b and sl.num_ref_idx_l1 > 0):
        out += [("ref_idx_bins", n) for n in range(1, min(max(sl.num_ref_idx_l0, sl.num_ref_idx_l1 if sl.slice_b else 0), 3) + 1)]
    out += [("refused", r) for r in REFUSALS if not (r == "bi_small" and not sl.slice_b) and not (r == "pred_in_p_slice" and sl.slice_b)]
    return out


# the vector differences the made cases walk through, per component: 0, +-1 .. +-3, both sides of every EG1 prefix length, the ends of int16
MVD_VALUES = [0, 1, -1, 2, -2, 3, -3, 4, -4, 5, -5] + [s * (v + 2) for k in range(2, 16) for v in ((1 << k) - 3, (1 << k) - 2) for s in (1, -1) if v + 2 <= 32767] + [32767, -32768]


def make_cases(seed, sl, n_random=200, n_states=7):
    """-> (states uint8 [n_states, 16], jobs PU_RATE_JOB_DT): the systematic cases, n_random random ones and the refusals of one slice; out_index is a permutation"""
    from turingcodec_amd.havoc import PU_RATE_JOB_DT
    rng = np.random.default_rng(seed)
    states = rng.integers(0, 126, (n_states, SYNTAX_BYTES)).astype(np.uint8)
    rows = []
    preds = (L0, L1, BI) if sl.slice_b else (L0,)

    def job(**kw):
        j = np.zeros(1, PU_RATE_JOB_DT)[0]
        j["w"], j["h"] = 1 << int(rng.integers(3, 7)), 1 << int(rng.integers(3, 7))
        j["cqt_depth"] = rng.integers(0, 4)
        j["pred"] = preds[int(rng.integers(len(preds)))]
        j["mvp_flag"] = rng.integers(0, 2, 2)
        j["ref_idx"] = [rng.integers(0, sl[3] + 1), rng.integers(0, sl[4] + 1)]
        mag = 1 << rng.integers(0, 16, (2, 2))
        j["mvd"] = np.clip(rng.integers(-mag, mag + 1), -32768, 32767) * (rng.random((2, 2)) < 0.8)
        j["merge_idx"] = rng.integers(0, sl.max_num_merge_cand)
        for k, v in kw.items():
            j[k] = v
        rows.append(j)
        return j

    for i in range(sl.max_num_merge_cand):                          # every merge index, merged and skipped (skip alone and beside merge)
        job(flags=MERGE, merge_idx=i)
        job(flags=SKIP, merge_idx=i)
        job(flags=SKIP | MERGE, merge_idx=i)
    job(flags=MERGE, merge_idx=0, pred=7, mvp_flag=[9, 9], ref_idx=[99, 99], cqt_depth=200)      # a merged job: the other fields are not read
    for p in preds:
        for d in range(4):
            job(pred=p, cqt_depth=d)
    if sl.slice_b:
        for w, h in ((8, 4), (4, 8)):
            for p in (L0, L1):
                job(pred=p, w=w, h=h)
    for v in MVD_VALUES:                                            # as x and as y, in list 0, list 1 and both
        for p in preds:
            job(pred=p, mvd=[[v, rng.integers(-3, 4)], [rng.integers(-3, 4), v]])
            job(pred=p, mvd=[[rng.integers(-3, 4), v], [v, rng.integers(-3, 4)]])
    for l in (0, 1):                                                # every ref_idx of each list
        for r in range(sl[3 + l] + 1):
            for p in preds:
                ref = [rng.integers(0, sl[3] + 1), rng.integers(0, sl[4] + 1)]
                ref[l] = r
                job(pred=p, ref_idx=ref)
    job(pred=L0, mvp_flag=[1, 7], ref_idx=[0, 99])                  # what list 1 holds is not read for an L0 candidate
    for _ in range(n_random):
        job(flags=[0, 0, 0, MERGE, SKIP][int(rng.integers(5))])
    # ---- one job per refusal (include/havoc_mi355x.h)
    job(flags=4)
    job(flags=0x80 | MERGE)
    job(flags=MERGE, merge_idx=sl.max_num_merge_cand)
    job(flags=SKIP, merge_idx=255)
    job(pred=3)
    job(pred=255)
    job(cqt_depth=4, pred=L0)
    job(pred=L0, mvp_flag=[2, 0])
    job(pred=L0, ref_idx=[sl[3] + 1, 0])
    if sl.slice_b:
        job(pred=BI, w=8, h=4)
        job(pred=BI, w=4, h=8)
        job(pred=L1, mvp_flag=[0, 255])
        job(pred=BI, ref_idx=[0, sl[4] + 1])
    else:
        job(pred=L1)
        job(pred=BI)
    jobs = np.array(rows, PU_RATE_JOB_DT)
    order = rng.permutation(len(jobs))
    jobs = jobs[order]
    jobs["ctx_index"] = rng.integers(0, n_states, len(jobs))
    jobs["out_index"] = rng.permutation(len(jobs))
    return states, jobs


def lambda_q16(d):
    """Lambda::set(double) (turing/FixedPoint.h)"""
    return int(d * 65536 + 0.5)


# ---- the reference's own functions ----------------------------------------------------------------------------------------------------------------
def reference_dir():
    return T.reference_dir()


class Shim:
    """tests/pu_rate_shim.cpp over the reference's turing/SyntaxCtu.hpp, Binarization.h, Write.h, CodedData.h and Cabac.cpp, built with oracle/Makefile's TURFLAGS"""

    def __init__(self):
        ref = T.reference_dir()
        assert ref, "reference sources not present"
        self._tmp = tempfile.TemporaryDirectory()
        so = os.path.join(self._tmp.name, "libpu_rate.so")
        flags = T._make_var("TURFLAGS").split()
        subprocess.check_call(["g++"] + flags + ["-shared", "-o", so, os.path.join(ROOT, "tests", "pu_rate_shim.cpp")]
                              + [os.path.join(ref, "turing", f) for f in ("Cabac.cpp", "ScanOrder.cpp")])
        self.L = C.CDLL(so)
        self.L.pu_rate_candidate.restype = C.c_int64
        self.L.pu_rate_candidate.argtypes = [C.c_void_p] * 3
        self.L.pu_rate_cost.restype = C.c_int64
        self.L.pu_rate_cost.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p]

    def walk_jobs(self, jobs, sl, states):
        """walk_jobs by the reference, for the jobs the contract does not refuse (the refusals are this project's, not the reference's: their rate is -1 here too)
        -> (rates, snapshots after)"""
        nr = int(jobs["out_index"].max()) + 1 if len(jobs) else 0
        rates, after = np.zeros(nr, np.int64), np.zeros((len(jobs), SYNTAX_BYTES), np.uint8)
        s = np.array(sl, np.int32)
        for j, job in enumerate(jobs):
            syn = np.ascontiguousarray(states[int(job["ctx_index"])], np.uint8).copy()
            if refusal(job, sl) is None:
                flags = int(job["flags"])
                p = np.array([bool(flags & SKIP), bool(flags & MERGE), job["merge_idx"], job["pred"], *job["mvd"].reshape(-1), *job["mvp_flag"], *job["ref_idx"], job["w"],
                              job["h"], job["cqt_depth"], 0], np.int32)
                rates[int(job["out_index"])] = self.L.pu_rate_candidate(p.ctypes.data, s.ctypes.data, syn.ctypes.data)
            else:
                rates[int(job["out_index"])] = -1
            after[j] = syn
        return rates, after

    def cost(self, rate, satd, d):
        """measurePuCost's sum with the reference's Cost and Lambda -> (cost, Lambda::set(d).value)"""
        lam = np.zeros(1, np.int32)
        c = self.L.pu_rate_cost(int(rate), int(satd[0]), int(satd[1]), int(satd[2]), float(d), lam.ctypes.data)
        return int(c), int(lam[0])


# ---- go2's comparison in numpy ------------------------------------------------------------------------------------------------------------------
def pu_decide(first, count, rates, satd_y, satd_cb, satd_cr, lam_q16, after=None):
    """havoc_mi355x_pu_decide -> (cost int64 per candidate, best int32 [n], best_cost int64 [n], best_syntax uint8 [n, 16] or None)"""
    rates = np.asarray(rates, np.int64)
    satd = (np.asarray(satd_y, np.int64) + np.asarray(satd_cb, np.int64) + np.asarray(satd_cr, np.int64)).astype(np.uint32).view(np.int32).astype(np.int64)
    cost = np.where(rates < 0, -1, rates + satd * int(lam_q16)).astype(np.int64)
    n = len(first)
    best, best_cost = np.full(n, -1, np.int32), np.full(n, -1, np.int64)
    best_syntax = None if after is None else np.zeros((n, SYNTAX_BYTES), np.uint8)
    for i in range(n):
        f = int(first[i])
        for k in range(int(count[i])):
            if rates[f + k] >= 0 and (best[i] < 0 or cost[f + k] < best_cost[i]):
                best[i], best_cost[i] = k, cost[f + k]
        if best[i] >= 0 and after is not None:
            best_syntax[i] = after[f + best[i]]
    return cost, best, best_cost, best_syntax


class DecisionClient:
    """tests/pu_decide_client.cpp: search/pu_decision.hpp's decidePu, compiled at test time"""

    def __init__(self):
        self._tmp = tempfile.TemporaryDirectory()
        so = os.path.join(self._tmp.name, "libpu_decide_client.so")
        subprocess.check_call(["g++", "-O1", "-std=c++14", "-fPIC", "-shared", "-Wall", "-o", so, os.path.join(ROOT, "tests", "pu_decide_client.cpp")])
        self.L = C.CDLL(so)
        self.L.pu_decide.restype = C.c_int
        self.L.pu_decide.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]

    def decide(self, first, count, rates, satd_y, satd_cb, satd_cr, lam_q16):
        first, count = np.ascontiguousarray(first, np.int32), np.ascontiguousarray(count, np.int32)
        rates = np.ascontiguousarray(rates, np.int64)
        satd = np.ascontiguousarray(np.stack([satd_y, satd_cb, satd_cr]), np.int32)
        cost, best, best_cost = np.zeros(len(rates), np.int64), np.zeros(len(first), np.int32), np.zeros(len(first), np.int64)
        assert self.L.pu_decide(first.ctypes.data, count.ctypes.data, len(first), rates.ctypes.data, satd.ctypes.data, len(rates), lam_q16, cost.ctypes.data,
                                best.ctypes.data, best_cost.ctypes.data) == 0
        return cost, best, best_cost


def random_units(seed, n, lam_q16):
    """n units of 0..8 contiguous candidates with arbitrary rates (some -1) and SATDs.  The first units are made cases: 0 a tie of all three candidates (the first
    wins), 1 a tie between the second and the third below the first (the second wins), 2 every candidate refused, 3 a refused first candidate with the smallest SATD
    (never chosen), 4 the last candidate cheaper by ONE Q16 unit (it wins: the comparison is exact in int64), 5 no candidate at all.
    -> (first, count, rates, satd_y, satd_cb, satd_cr, after)"""
    rng = np.random.default_rng(seed)
    count = rng.integers(0, 9, n).astype(np.int32)
    count[:6] = [3, 3, 3, 3, 2, 0]
    first = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int32)
    m = int(count.sum())
    rates = rng.integers(0, 60 << 16, m).astype(np.int64)
    rates[rng.random(m) < 0.15] = -1
    satd = rng.integers(0, 1 << 20, (3, m)).astype(np.int32)
    satd[:, rng.random(m) < 0.05] = (1 << 27)          # large: the product needs all of int64's low 48 bits
    f = first
    rates[f[0]:f[0] + 3], satd[:, f[0]:f[0] + 3] = 5 << 16, 100
    rates[f[1]:f[1] + 3], satd[:, f[1]:f[1] + 3] = [9 << 16, 5 << 16, 5 << 16], 100
    rates[f[2]:f[2] + 3] = -1
    rates[f[3]:f[3] + 3], satd[:, f[3]:f[3] + 3] = [-1, 7 << 16, 8 << 16], [[0, 50, 50]] * 3
    rates[f[4]:f[4] + 2], satd[:, f[4]:f[4] + 2] = [lam_q16 + 1, 0], [[0, 1], [0, 0], [0, 0]]      # costs lam + 1 and lam
    after = rng.integers(0, 126, (m, SYNTAX_BYTES)).astype(np.uint8)
    return first, count, rates, satd[0].copy(), satd[1].copy(), satd[2].copy(), after
