"""The rate the reference measures for one refined intra candidate "since the partition began" (EstimateRateLuma over Syntax<IntraPartition>, turing/Search.hpp:199,
242-246; turing/SyntaxCtu.hpp:704-722), restated on the CPU in plain Python on top of residual_rate_tools.walk_block.  Test infrastructure.

In the syntax's order: prev_intra_luma_pred_flag (one context; 1 when the mode is in candModeList, turing/Binarization.h:395-452), mpm_idx (1 bypass bit for 0, 2 for
1 or 2, :454-487) or rem_intra_luma_pred_mode (5 bypass bits, :489-502), split_transform_flag = 0 with ctxInc = 5 - log2 where transform_tree codes it
(SyntaxCtu.hpp:330-337, Binarization.h:617-634), cbf_luma with ctxInc = (trafoDepth == 0) (:637-651), and the block's residual_coding when it has a level.  cbf_cb,
cbf_cr and the chroma residuals are priced as nothing (turing/EstimateRate.h:114-119).  `candidate_rate` counts the branches it takes in `tags`.  `Shim` compiles
tests/intra_rate_shim.cpp -- the reference's own syntax functions and element writers over a stand-in handle -- into a temporary directory.  `make_cases` makes the
candidates: RDOQ blocks of rdoq_tools.make_blocks and residual_rate_tools.special_blocks (all-zero, DC only, a lone level at the last position of the last sub-block,
...), each with a mode, a candModeList and a kind of unit.
"""
import collections
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import residual_rate_tools as R
import sao_decision_tools as T
from sao_merge_tools import bin_cost

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PREV_FLAG, SPLIT_FLAG, SYNTAX_BYTES = 0, 1, 4      # include/havoc_mi355x.h: HAVOC_INTRA_SYNTAX_CTX_*
CBF_LUMA = 1                                       # HAVOC_RDOQ_CTX_CBF_LUMA
SPLIT_CODED, DEPTH_NONZERO = 1, 2                  # HAVOC_INTRA_RATE_*

# what says which kind of unit a candidate belongs to, beside its size: (IntraSplitFlag, max_transform_hierarchy_depth_intra, MinTbLog2SizeY, MaxTbLog2SizeY)
ENCODER = dict(depth_intra=1, min_tb=2, max_tb=5)      # turing/Encoder.cpp:662-665 (CtbLog2SizeY >= 5)


def rate_flags(log2, split, depth_intra=1, min_tb=2, max_tb=5):
    """SyntaxCtu.hpp:332-334 for the transform_tree Syntax<IntraPartition> opens (:714-720: trafoDepth = IntraSplitFlag, MaxTrafoDepth = depth_intra + IntraSplitFlag)"""
    depth = 1 if split else 0
    coded = log2 <= max_tb and log2 > min_tb and depth < depth_intra + depth and not (split and depth == 0)
    return (SPLIT_CODED if coded else 0) | (DEPTH_NONZERO if depth else 0)


def mpm_index(mode, cand):
    """Binarization.h:432-447: the first x with mode == candModeList[x]; 3: none (rem_intra_luma_pred_mode)"""
    for x in range(3):
        if mode == cand[x]:
            return x
    return 3


def job_valid(log2, job):
    return int(job["mpm_idx"]) <= 3 and int(job["scan_idx"]) <= 2 and (int(job["scan_idx"]) == 0 or log2 <= 3) and not (int(job["flags"]) & SPLIT_CODED and log2 == 2)


def candidate_rate(block, log2, mpm_idx, flags, scan_idx, sdh, st, syn, tags=None):
    """block: int [n, n] levels; st: list of 128 context states, syn: list of 4, both updated in place -> the Q16 rate"""
    tags = collections.Counter() if tags is None else tags
    rate = 0
    in_list = int(mpm_idx < 3)
    syn[PREV_FLAG], r = bin_cost(syn[PREV_FLAG], in_list)
    rate += r + ((1 if mpm_idx == 0 else 2 if in_list else 5) << 16)
    tags["mpm", mpm_idx] += 1
    coded = bool(flags & SPLIT_CODED)
    if coded:
        syn[SPLIT_FLAG + 5 - log2], r = bin_cost(syn[SPLIT_FLAG + 5 - log2], 0)
        rate += r
    tags["split_coded", int(coded)] += 1
    depth = 1 if flags & DEPTH_NONZERO else 0
    cbf = int(np.any(block))
    ctx = CBF_LUMA + (0 if depth else 1)
    st[ctx], r = bin_cost(st[ctx], cbf)
    rate += r
    tags["depth", depth] += 1
    tags["cbf", cbf] += 1
    if cbf:
        tags["scan", scan_idx] += 1
        rate += R.walk_block(block, log2, 0, scan_idx, sdh, st, tags)
    return rate


def walk_jobs(log2, levels, states, syntax_states, jobs, tags=None):
    """the device's contract: -> (int64 rates [max rate_index + 1] (entries no job writes 0), uint8 states after [njobs, 128], uint8 syntax states after [njobs, 4])"""
    tags = collections.Counter() if tags is None else tags
    n, n2 = 1 << log2, 1 << 2 * log2
    nr = int(jobs["rate_index"].max()) + 1 if len(jobs) else 0
    rates = np.zeros(nr, np.int64)
    after, after_syn = np.zeros((len(jobs), 128), np.uint8), np.zeros((len(jobs), SYNTAX_BYTES), np.uint8)
    for j, job in enumerate(jobs):
        st = [int(v) for v in states[int(job["ctx_index"])]]
        syn = [int(v) for v in syntax_states[int(job["ctx_index"])]]
        if not job_valid(log2, job):
            rates[int(job["rate_index"])] = -1
        else:
            o = int(job["level_off"])
            rates[int(job["rate_index"])] = candidate_rate(levels[o:o + n2].reshape(n, n), log2, int(job["mpm_idx"]), int(job["flags"]), int(job["scan_idx"]),
                                                           int(job["sdh"]), st, syn, tags)
        after[j], after_syn[j] = st, syn
    return rates, after, after_syn


# ---- candidates -----------------------------------------------------------------------------------------------------------------------------------
AUX_DT = np.dtype([("mode", "<i4"), ("cand", "<i4", 3), ("split", "<i4"), ("blk_idx", "<i4"), ("depth_intra", "<i4"), ("min_tb", "<i4"), ("max_tb", "<i4")])


def make_cases(oracle, seed, log2, rdoq_count, n_states=7, bd=8):
    """-> (levels int16 [blocks * n * n], states uint8 [n_states, 128], syntax states uint8 [n_states, 4], jobs INTRA_RATE_JOB_DT, aux AUX_DT): rdoq_count blocks
    quantised by the oracle's RDOQ plus the hand-made ones, one candidate each.  aux says what the job's mpm_idx and flags were derived from: the mode, the
    candModeList (now and then with the mode in two places: the first wins) and the kind of unit."""
    import rdoq_tools as rt
    from turingcodec_amd.havoc import INTRA_RATE_JOB_DT
    rng = np.random.default_rng(seed)
    n2 = 1 << 2 * log2
    src, states, blocks = rt.make_blocks(seed, log2, bd, rdoq_count, n_states=n_states)
    lv, _ = rt.run_cpu(oracle, src, states, blocks)
    items = [(lv[b["src_off"]:b["src_off"] + n2], b["scan_idx"] if log2 <= 3 else 0, b["sdh"]) for b in blocks]
    items += [(b.ravel(), s, sdh) for b, c, s, sdh in R.special_blocks(rng, log2) if c == 0]
    order = rng.permutation(len(items))
    syntax_states = rng.integers(0, 126, (n_states, SYNTAX_BYTES)).astype(np.uint8)
    jobs, aux, levels = np.zeros(len(items), INTRA_RATE_JOB_DT), np.zeros(len(items), AUX_DT), []
    for k, i in enumerate(order):
        block, scan, sdh = items[i]
        levels.append(block)
        mode = int(rng.integers(0, 35))
        cand = [int(v) for v in rng.choice(35, 3, replace=False)]
        kind = k % 8
        if kind < 3:
            cand[kind] = mode                                  # mpm_idx 0, 1, 2
        elif kind == 3:
            cand[1] = cand[2] = mode                           # in two places: mpm_idx 1
        elif kind == 4 and k % 16 == 4:
            cand[0] = cand[2] = mode                           # ... mpm_idx 0
        # the unit: the encoder's 2Nx2N partition (4x4: a partition of an NxN unit) three times out of four; else the other split and depth settings
        split, depth_intra, min_tb, max_tb = int(log2 == 2), 1, 2, 5
        if k % 4 == 3:
            split, depth_intra = int(rng.integers(0, 2)), int(rng.integers(0, 2))
            if k % 8 == 7:
                min_tb, max_tb = int(rng.integers(2, 4)), int(rng.integers(4, 6))
        a = aux[k]
        a["mode"], a["cand"], a["split"], a["blk_idx"] = mode, cand, split, int(rng.integers(0, 4)) if split else 0
        a["depth_intra"], a["min_tb"], a["max_tb"] = depth_intra, min_tb, max_tb
        j = jobs[k]
        j["level_off"], j["ctx_index"], j["rate_index"] = k * n2, int(rng.integers(0, n_states)), k
        j["scan_idx"], j["sdh"], j["mpm_idx"], j["flags"] = scan, sdh, mpm_index(mode, cand), rate_flags(log2, split, depth_intra, min_tb, max_tb)
    return np.concatenate(levels).astype(np.int16), states, syntax_states, jobs, aux


def required_tags(log2):
    """what the candidates used on the device must reach, per transform size (a 4x4 block never codes split_transform_flag: log2 > MinTbLog2SizeY fails)"""
    req = [("mpm", 0), ("mpm", 1), ("mpm", 2), ("mpm", 3), ("split_coded", 0), ("depth", 0), ("depth", 1), ("cbf", 0), ("cbf", 1), ("scan", 0),
           "dc_only", "lone_last"]
    if log2 > 2:
        req += [("split_coded", 1)]
    if log2 <= 3:
        req += [("scan", 1), ("scan", 2)]
    return req


# ---- the reference's own functions ----------------------------------------------------------------------------------------------------------------
def reference_dir():
    return T.reference_dir()


class Shim:
    """tests/intra_rate_shim.cpp over the reference's turing/SyntaxCtu.hpp, Binarization.h, EncodeResidual.hpp, CodedData.h, Cabac.cpp and ScanOrder.cpp, built with
    oracle/Makefile's TURFLAGS"""

    def __init__(self):
        ref = T.reference_dir()
        assert ref, "reference sources not present"
        self._tmp = tempfile.TemporaryDirectory()
        so = os.path.join(self._tmp.name, "libintra_rate.so")
        flags = T._make_var("TURFLAGS").split()
        subprocess.check_call(["g++"] + flags + ["-shared", "-o", so, os.path.join(ROOT, "tests", "intra_rate_shim.cpp")]
                              + [os.path.join(ref, "turing", f) for f in ("Cabac.cpp", "ScanOrder.cpp")])
        self.L = C.CDLL(so)
        self.L.intra_rate_candidate.restype = C.c_int64
        self.L.intra_rate_candidate.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 3

    def walk_jobs(self, log2, levels, states, syntax_states, jobs, aux):
        """walk_jobs by the reference (valid jobs only), from what the jobs were derived from: the mode and candModeList, the kind of unit.  The job's own mpm_idx and
        flags are not given to it: -> (rates, states after, syntax states after, int32 [njobs, 3]: mpm_idx (3: rem), rem_intra_luma_pred_mode, MaxTrafoDepth)"""
        n2 = 1 << 2 * log2
        levels = np.ascontiguousarray(levels, np.int16)
        nr = int(jobs["rate_index"].max()) + 1 if len(jobs) else 0
        rates = np.zeros(nr, np.int64)
        after, after_syn = np.zeros((len(jobs), 128), np.uint8), np.zeros((len(jobs), SYNTAX_BYTES), np.uint8)
        info = np.zeros((len(jobs), 3), np.int32)
        for j, (job, a) in enumerate(zip(jobs, aux)):
            st = np.ascontiguousarray(states[int(job["ctx_index"])], np.uint8).copy()
            syn = np.ascontiguousarray(syntax_states[int(job["ctx_index"])], np.uint8).copy()
            o = int(job["level_off"])
            blk = np.ascontiguousarray(levels[o:o + n2])
            cand = np.ascontiguousarray(a["cand"], np.int32)
            rates[int(job["rate_index"])] = self.L.intra_rate_candidate(blk.ctypes.data, log2, int(a["mode"]), cand.ctypes.data, int(a["split"]), int(a["blk_idx"]),
                                                                        int(a["depth_intra"]), int(a["min_tb"]), int(a["max_tb"]), int(job["scan_idx"]),
                                                                        int(job["sdh"]), st.ctypes.data, syn.ctypes.data, info[j].ctypes.data)
            after[j], after_syn[j] = st, syn
        return rates, after, after_syn, info


# ---- search/tu_decision.hpp: decideIntraRd with a rate per candidate, in numpy ---------------------------------------------------------------------
def stand_in_rates(mpm, order, count, slot, cbf, stats):
    """what havoc_mi355x_intra_decide charges candidate slot s: the first stage's mode offset + (1 + (cbf ? 2 nonzero + sum_abs : 0)) << 16"""
    out = np.zeros(int((slot + count).max()) if len(slot) else 0, np.int64)
    for i in range(len(count)):
        for j in range(int(count[i])):
            s, mode, c = int(slot[i]) + j, int(order[i, j]), mpm[i]["cand_mode_list"]
            mode_rate = int(mpm[i]["rate_a_minus_c"]) if mode == c[0] else (int(mpm[i]["rate_b_minus_c"]) if mode in (c[1], c[2]) else 0)
            out[s] = mode_rate + int(R.tu_rate(cbf[s], stats[s, 0], stats[s, 1]))
    return out


def decide_intra_rated(order, count, slot, cbf, ssd, rates, rl_q16, stats=None):
    """INTRA_RD_RESULT_DT records as havoc_mi355x_intra_decide_rated writes them: candidates in refinement order, cost = rate + rl_q16 * ssd (the SSD as int32), the
    first with the smallest cost (strict `<`); a partition without candidates: mode -1, cost = the largest int64"""
    from turingcodec_amd.decisions import INTRA_RD_RESULT_DT
    out = np.zeros(len(count), INTRA_RD_RESULT_DT)
    out["mode"], out["cost"] = -1, np.iinfo(np.int64).max
    for i in range(len(count)):
        r = out[i]
        for j in range(int(count[i])):
            s = int(slot[i]) + j
            cost = int(rates[s]) + rl_q16 * int(np.array(ssd[s], np.uint32).view(np.int32))
            r["evaluated"] += 1
            if cost < int(r["cost"]):
                r["mode"], r["index"], r["cost"] = int(order[i, j]), j, cost
                r["outcome"]["cbf"], r["outcome"]["ssd"] = cbf[s], ssd[s]
                if stats is not None:
                    r["outcome"]["nonzero"], r["outcome"]["sum_abs"] = stats[s, 0], stats[s, 1]
    return out


class DecisionClient:
    """tests/intra_rated_client.cpp: search/tu_decision.hpp's decideIntraRd with a rate functor, compiled at test time"""

    def __init__(self):
        self._tmp = tempfile.TemporaryDirectory()
        so = os.path.join(self._tmp.name, "libintra_rated_client.so")
        subprocess.check_call(["g++", "-O1", "-std=c++14", "-fPIC", "-shared", "-Wall", "-o", so, os.path.join(ROOT, "tests", "intra_rated_client.cpp")])
        self.L = C.CDLL(so)
        self.L.intra_rated_decide.restype = C.c_int
        self.L.intra_rated_decide.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int32, C.c_int, C.c_void_p]

    def decide(self, order, count, slot, ssd, rates, rl_q16, measure_like_the_reference=False):
        """-> int64 [n, 5]: mode, index, evaluated, cost, candidates whose rate was not measured"""
        order, count, slot = np.ascontiguousarray(order, np.int32), np.ascontiguousarray(count, np.int32), np.ascontiguousarray(slot, np.int32)
        ssd, rates = np.ascontiguousarray(ssd, np.uint32), np.ascontiguousarray(rates, np.int64)
        out = np.zeros((len(count), 5), np.int64)
        assert self.L.intra_rated_decide(order.ctypes.data, count.ctypes.data, slot.ctypes.data, ssd.ctypes.data, rates.ctypes.data, len(count), rl_q16,
                                         int(measure_like_the_reference), out.ctypes.data) == 0
        return out
