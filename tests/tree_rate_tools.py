"""The rate the reference's inter transform-tree decision measures for one depth of a unit (EstimateRate<void> over `if (rqt_root_cbf) transform_tree`,
turing/Reconstruct.cpp:1296-1428; Syntax<transform_tree>, turing/SyntaxCtu.hpp:329-379; Syntax<transform_unit>, :411-502; the writers, turing/Binarization.h:617-666),
restated on the CPU in plain Python on top of residual_rate_tools.walk_block, and the decision over three planes in numpy.  Test infrastructure.

`tree_rate` walks the tree in the SYNTAX's order -- flags before the residuals they announce, Cb and Cr interleaved per child -- where the device walks the residuals
first and prices the flags after them; it counts the branches it takes in `tags` and lists the residual_coding calls the syntax reaches.  `Shim` compiles
tests/tree_rate_shim.cpp -- the reference's own syntax functions, element writers and CodedData functions over a stand-in handle -- into a temporary directory.
`make_cases` makes the trees from blocks the oracle's RDOQ quantised (rdoq_tools.make_blocks) and residual_rate_tools.special_blocks.
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

SPLIT_FLAG, SYNTAX_BYTES = 1, 4      # include/havoc_mi355x.h: HAVOC_INTRA_SYNTAX_CTX_SPLIT_TRANSFORM_FLAG, _BYTES
CBF_LUMA, CBF_CHROMA = 1, 3          # HAVOC_RDOQ_CTX_CBF_LUMA, _CBF_CHROMA
SPLIT_CODED = 1                      # HAVOC_TREE_RATE_SPLIT_FLAG_CODED
UNITS = [(L, d) for L in (3, 4, 5) for d in (0, 1)]


def geometry(L, depth):
    """-> (luma log2, luma blocks, chroma log2, chroma blocks per component) of a unit of log2 size L coded at `depth`"""
    if depth == 0:
        return L, 1, max(L - 1, 2), 1
    return L - 1, 4, max(L - 2, 2), 4 if L > 3 else 1


def sizes(L, depth):
    """int16 levels a job has in the luma table, and per component in the chroma table"""
    ly, ny, lc, nc = geometry(L, depth)
    return ny << 2 * ly, nc << 2 * lc


def rate_flags(L, max_trafo_depth=1, min_tb=2, max_tb=5):
    """SyntaxCtu.hpp:332-334 for the unit's transform_tree at trafoDepth 0 (inter: IntraSplitFlag 0)"""
    return SPLIT_CODED if L <= max_tb and L > min_tb and 0 < max_trafo_depth else 0


def job_valid(job):
    return (int(job["flags"]) & ~SPLIT_CODED) == 0


def tree_rate(luma, cb, cr, L, depth, flags, sdh, st, syn, tags=None, calls=None, chroma_first=False):
    """luma: [int [n, n] blocks] (1 or 4), cb, cr: the same per component (1 or 4); st: list of 128 context states, syn: list of 4, both updated in place
    -> (the Q16 rate, the cbf mask).  chroma_first: NOT the syntax -- every Cb block before every Cr block -- to show that the order is exercised."""
    tags = collections.Counter() if tags is None else tags
    calls = [] if calls is None else calls
    ly, ny, lc, nc = geometry(L, depth)
    mask = 0
    for k in range(ny):
        mask |= int(np.any(luma[k])) << k
    for k in range(nc):
        mask |= int(np.any(cb[k])) << (4 + k) | int(np.any(cr[k])) << (8 + k)
    if mask == 0:
        tags["zero_tree"] += 1
        return 0, 0
    rate = [0]

    def decision(table, ctx, b):
        table[ctx], r = bin_cost(table[ctx], b)
        rate[0] += r

    def residual(block, x0, y0, log2, c_idx):
        coded = int(np.any(block))
        calls.append((x0, y0, log2, c_idx, coded))
        if coded:
            rate[0] += R.walk_block(block, log2, c_idx, 0, sdh, st)

    coded = bool(flags & SPLIT_CODED)
    tags["split_coded", int(coded)] += 1
    if coded:
        decision(syn, SPLIT_FLAG + 5 - L, depth)
    pcb, pcr = int(mask & 0x0f0 != 0), int(mask & 0xf00 != 0)
    decision(st, CBF_CHROMA, pcb)
    decision(st, CBF_CHROMA, pcr)
    tags["parent_cb", pcb] += 1
    tags["parent_cr", pcr] += 1
    if depth == 0:
        if pcb or pcr:
            decision(st, CBF_LUMA + 1, mask & 1)
            tags["cbf_luma0", mask & 1] += 1
        else:
            tags["cbf_luma0", "inferred"] += 1
        residual(luma[0], 0, 0, L, 0)
        residual(cb[0], 0, 0, lc, 1)
        residual(cr[0], 0, 0, lc, 2)
        return rate[0], mask
    if L == 3:
        tags["l3_depth1"] += 1
    half = 1 << (L - 1)
    for k in range(4):
        x0, y0 = (k & 1) * half, (k >> 1) * half
        if nc == 4:
            if pcb:
                decision(st, CBF_CHROMA + 1, mask >> (4 + k) & 1)
                tags["child_cb", mask >> (4 + k) & 1] += 1
            if pcr:
                decision(st, CBF_CHROMA + 1, mask >> (8 + k) & 1)
                tags["child_cr", mask >> (8 + k) & 1] += 1
        decision(st, CBF_LUMA, mask >> k & 1)
        tags["cbf_luma1", mask >> k & 1] += 1
        residual(luma[k], x0, y0, ly, 0)
        if nc == 4 and not chroma_first:
            residual(cb[k], x0, y0, lc, 1)
            residual(cr[k], x0, y0, lc, 2)
        elif nc == 1 and k == 3:
            residual(cb[0], 0, 0, lc, 1)
            residual(cr[0], 0, 0, lc, 2)
    if nc == 4 and chroma_first:
        for c_idx, blocks in ((1, cb), (2, cr)):
            for k in range(4):
                residual(blocks[k], (k & 1) * half, (k >> 1) * half, lc, c_idx)
    return rate[0], mask


def job_blocks(L, depth, luma_levels, chroma_levels, job):
    ly, ny, lc, nc = geometry(L, depth)

    def cut(table, off, log2, count):
        n, n2 = 1 << log2, 1 << 2 * log2
        return [table[off + k * n2:off + (k + 1) * n2].reshape(n, n) for k in range(count)]

    return cut(luma_levels, int(job["luma_off"]), ly, ny), cut(chroma_levels, int(job["cb_off"]), lc, nc), cut(chroma_levels, int(job["cr_off"]), lc, nc)


def walk_jobs(L, depth, luma_levels, chroma_levels, states, syntax_states, jobs, tags=None, all_calls=None):
    """the device's contract: -> (int64 rates and uint32 masks [max out_index + 1] (entries no job writes 0), uint8 states after [njobs, 128], uint8 syntax states
    after [njobs, 4]); all_calls: a list that gets every job's residual_coding calls"""
    tags = collections.Counter() if tags is None else tags
    nr = int(jobs["out_index"].max()) + 1 if len(jobs) else 0
    rates, masks = np.zeros(nr, np.int64), np.zeros(nr, np.uint32)
    after, after_syn = np.zeros((len(jobs), 128), np.uint8), np.zeros((len(jobs), SYNTAX_BYTES), np.uint8)
    for j, job in enumerate(jobs):
        st = [int(v) for v in states[int(job["ctx_index"])]]
        syn = [int(v) for v in syntax_states[int(job["ctx_index"])]]
        calls = []
        if not job_valid(job):
            rates[int(job["out_index"])] = -1
        else:
            y, cb, cr = job_blocks(L, depth, luma_levels, chroma_levels, job)
            r, m = tree_rate(y, cb, cr, L, depth, int(job["flags"]), int(job["sdh"]), st, syn, tags, calls)
            rates[int(job["out_index"])], masks[int(job["out_index"])] = r, m
            if depth == 1 and L > 3 and m & 0xff0:
                other = tree_rate(y, cb, cr, L, depth, int(job["flags"]), int(job["sdh"]), [int(v) for v in states[int(job["ctx_index"])]],
                                  [int(v) for v in syntax_states[int(job["ctx_index"])]], chroma_first=True)[0]
                if other != r:
                    tags["order_matters"] += 1
        if all_calls is not None:
            all_calls.append(calls)
        after[j], after_syn[j] = st, syn
    return rates, masks, after, after_syn


def required_tags(L, depth):
    """what the trees used on the device must reach, per unit size and depth"""
    req = [("split_coded", 0), ("split_coded", 1), ("parent_cb", 0), ("parent_cb", 1), ("parent_cr", 0), ("parent_cr", 1), "zero_tree"]
    if depth == 0:
        req += [("cbf_luma0", "inferred"), ("cbf_luma0", 0), ("cbf_luma0", 1)]
    else:
        req += [("cbf_luma1", 0), ("cbf_luma1", 1)]
        if L == 3:
            req += ["l3_depth1"]
        else:
            req += [("child_cb", 0), ("child_cb", 1), ("child_cr", 0), ("child_cr", 1), "order_matters"]
    return req


# ---- trees -----------------------------------------------------------------------------------------------------------------------------------------
AUX_DT = np.dtype([("max_trafo_depth", "<i4"), ("min_tb", "<i4"), ("max_tb", "<i4")])


def _pool(oracle, rng, seed, log2, count):
    """levels of `count` blocks the oracle's RDOQ quantised, plus the hand-made ones of residual_rate_tools.special_blocks (diagonal scan)"""
    import rdoq_tools as rt
    n2 = 1 << 2 * log2
    src, states, blocks = rt.make_blocks(seed, log2, 8, count)
    lv, _ = rt.run_cpu(oracle, src, states, blocks)
    pool = [lv[b["src_off"]:b["src_off"] + n2] for b in blocks]
    pool += [b.ravel() for b, c, s, sdh in R.special_blocks(rng, log2) if s == 0]
    return [p.astype(np.int16) for p in pool]


def make_cases(oracle, seed, L, depth, count, n_states=7):
    """-> (luma levels int16, chroma levels int16, states uint8 [n_states, 128], syntax states uint8 [n_states, 4], jobs TREE_RATE_JOB_DT, aux AUX_DT): `count` trees
    of a unit of log2 size L at `depth`.  aux says what the job's flags were derived from.  One tree in eight has no level, one is coded in chroma only, one in luma
    only, one in Cb only; the rest draw every block from the pool or leave it empty."""
    from turingcodec_amd.havoc import TREE_RATE_JOB_DT
    rng = np.random.default_rng(seed)
    ly, ny, lc, nc = geometry(L, depth)
    pool_y = _pool(oracle, rng, seed, ly, max(count * ny // 3, 40))
    pool_c = pool_y if lc == ly else _pool(oracle, rng, seed + 1000, lc, max(count * nc // 3, 40))
    pool_y = [p for p in pool_y if p.any()]
    pool_c = [p for p in pool_c if p.any()]
    states = rng.integers(0, 126, (n_states, 128)).astype(np.uint8)
    syntax_states = rng.integers(0, 126, (n_states, SYNTAX_BYTES)).astype(np.uint8)
    sy, sc = sizes(L, depth)
    luma, chroma = np.zeros(count * sy, np.int16), np.zeros(count * 2 * sc, np.int16)
    jobs, aux = np.zeros(count, TREE_RATE_JOB_DT), np.zeros(count, AUX_DT)

    def draw(pool, blocks, log2, p):
        out = np.zeros(blocks << 2 * log2, np.int16)
        for k in range(blocks):
            if rng.random() < p:
                out[k << 2 * log2:(k + 1) << 2 * log2] = pool[int(rng.integers(0, len(pool)))]
        return out

    for k in range(count):
        kind = k % 8
        p = float(rng.choice([0.35, 0.6, 0.9]))
        y, cb, cr = draw(pool_y, ny, ly, p), draw(pool_c, nc, lc, p), draw(pool_c, nc, lc, p)
        if kind == 1:
            y[:], cb[:], cr[:] = 0, 0, 0
        elif kind == 2:
            y[:] = 0
            if not (cb.any() or cr.any()):
                cr[:1 << 2 * lc] = pool_c[k % len(pool_c)]
        elif kind == 3:
            cb[:], cr[:] = 0, 0
        elif kind == 4:
            cr[:] = 0
            if not cb.any():
                cb[-(1 << 2 * lc):] = pool_c[k % len(pool_c)]
        luma[k * sy:(k + 1) * sy] = y
        chroma[2 * k * sc:(2 * k + 1) * sc], chroma[(2 * k + 1) * sc:(2 * k + 2) * sc] = cb, cr
        a = aux[k]
        a["max_trafo_depth"], a["min_tb"], a["max_tb"] = 1, 2, 5      # the encoder's set-up; one tree in five another one, where the flag is not coded
        if k % 5 == 4:      # depth 0: the residual quadtree off; depth 1: a split that is inferred (a 32x32 unit above MaxTbLog2SizeY, or interSplitFlag)
            if depth == 1 and L == 5 and k % 2 == 0:
                a["max_tb"] = 4
            else:
                a["max_trafo_depth"] = 0
        j = jobs[k]
        j["luma_off"], j["cb_off"], j["cr_off"] = k * sy, 2 * k * sc, (2 * k + 1) * sc
        j["ctx_index"], j["out_index"], j["sdh"] = int(rng.integers(0, n_states)), k, int(rng.integers(0, 3) > 0)
        j["flags"] = rate_flags(L, int(a["max_trafo_depth"]), int(a["min_tb"]), int(a["max_tb"]))
    return luma, chroma, states, syntax_states, jobs, aux


# ---- the reference's own functions ----------------------------------------------------------------------------------------------------------------
def reference_dir():
    return T.reference_dir()


class Shim:
    """tests/tree_rate_shim.cpp over the reference's turing/SyntaxCtu.hpp, Binarization.h, EncodeResidual.hpp, CodedData.h, Cabac.cpp and ScanOrder.cpp, built with
    oracle/Makefile's TURFLAGS"""

    def __init__(self):
        ref = T.reference_dir()
        assert ref, "reference sources not present"
        self._tmp = tempfile.TemporaryDirectory()
        so = os.path.join(self._tmp.name, "libtree_rate.so")
        flags = T._make_var("TURFLAGS").split()
        subprocess.check_call(["g++"] + flags + ["-shared", "-o", so, os.path.join(ROOT, "tests", "tree_rate_shim.cpp")]
                              + [os.path.join(ref, "turing", f) for f in ("Cabac.cpp", "ScanOrder.cpp")])
        self.L = C.CDLL(so)
        self.L.tree_rate_tree.restype = C.c_int64
        self.L.tree_rate_tree.argtypes = [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p] * 4

    def walk_jobs(self, L, depth, luma_levels, chroma_levels, states, syntax_states, jobs, aux):
        """walk_jobs by the reference (valid jobs only), from what the jobs were derived from -- MaxTrafoDepth and the transform size limits, not the job's flags:
        -> (rates, masks, states after, syntax states after, [the residual_coding calls of each job: (x0, y0, log2, cIdx, cbf)])"""
        sy, sc = sizes(L, depth)
        luma_levels, chroma_levels = np.ascontiguousarray(luma_levels, np.int16), np.ascontiguousarray(chroma_levels, np.int16)
        nr = int(jobs["out_index"].max()) + 1 if len(jobs) else 0
        rates, masks = np.zeros(nr, np.int64), np.zeros(nr, np.uint32)
        after, after_syn = np.zeros((len(jobs), 128), np.uint8), np.zeros((len(jobs), SYNTAX_BYTES), np.uint8)
        all_calls = []
        for j, (job, a) in enumerate(zip(jobs, aux)):
            st = np.ascontiguousarray(states[int(job["ctx_index"])], np.uint8).copy()
            syn = np.ascontiguousarray(syntax_states[int(job["ctx_index"])], np.uint8).copy()
            y = np.ascontiguousarray(luma_levels[int(job["luma_off"]):int(job["luma_off"]) + sy])
            cb = np.ascontiguousarray(chroma_levels[int(job["cb_off"]):int(job["cb_off"]) + sc])
            cr = np.ascontiguousarray(chroma_levels[int(job["cr_off"]):int(job["cr_off"]) + sc])
            mask, calls = np.zeros(1, np.uint32), np.zeros(1 + 5 * 12, np.int32)
            rates[int(job["out_index"])] = self.L.tree_rate_tree(y.ctypes.data, cb.ctypes.data, cr.ctypes.data, L, depth, int(a["max_trafo_depth"]), int(a["min_tb"]),
                                                                 int(a["max_tb"]), int(job["sdh"]), st.ctypes.data, syn.ctypes.data, mask.ctypes.data, calls.ctypes.data)
            masks[int(job["out_index"])] = mask[0]
            all_calls.append([tuple(int(v) for v in calls[1 + 5 * i:6 + 5 * i]) for i in range(int(calls[0]))])
            after[j], after_syn[j] = st, syn
        return rates, masks, after, after_syn, all_calls


# ---- search/tu_decision.hpp: decideRqt over three planes with the whole tree's rate, in numpy --------------------------------------------------------------
def decide_tree(units, zero_at, one_at, sizes, csizes, chroma_at, tree_rate, tree_cbf, rl_q16):
    """units: RQT_CU_DT; sizes / csizes: {log2: dict(cbf, ssd)} per luma / chroma candidate; chroma_at: RQT_CHROMA_AT_DT; tree_rate, tree_cbf: [2 n], unit i's depth d
    at 2 i + d -> (RQT_RESULT_DT, RQT_TREE_RESULT_DT) records as havoc_mi355x_rqt_decide_tree writes them: depth 1 first; no level in any plane -> the unit stays
    unsplit without residual and depth 0 is never looked at; else depth 0 wins on cost_zero < cost_one, cost = rate + rl * int32(ssdY + 4 ssdCb + 4 ssdCr)"""
    from turingcodec_amd.decisions import RQT_RESULT_DT
    from turingcodec_amd.havoc import RQT_TREE_RESULT_DT
    out = np.zeros(len(units), RQT_RESULT_DT).view(np.int32).reshape(len(units), 26)
    tree = np.zeros(len(units), RQT_TREE_RESULT_DT)
    cost = np.zeros((len(units), 2), np.int64)

    def i32(v):
        return int(np.array(v & 0xFFFFFFFF, np.uint32).view(np.int32))

    for i, u in enumerate(units):
        L = int(u["log2_size"])
        s0, s1, j0, j1 = sizes[L], sizes[L - 1], int(zero_at[i]), int(one_at[i])
        c0, a = csizes[max(L - 1, 2)], chroma_at[i]
        chroma_zero = int(c0["ssd"][a["cb_zero"]]) + int(c0["ssd"][a["cr_zero"]])
        if L > 3:
            c1 = csizes[L - 2]
            chroma_one = sum(int(c1["ssd"][a["cb_one"] + k]) + int(c1["ssd"][a["cr_one"] + k]) for k in range(4))
        else:
            chroma_one = chroma_zero
        ssd_one = 0
        for k in range(4):
            out[i, 6 + 4 * k:10 + 4 * k] = [int(s1["cbf"][j1 + k]), i32(int(s1["ssd"][j1 + k])), 0, 0]
            ssd_one += int(s1["ssd"][j1 + k])
        tree[i]["mask_one"], tree[i]["chroma_ssd_one"] = tree_cbf[2 * i + 1], i32(chroma_one)
        cost[i, 1] = int(tree_rate[2 * i + 1]) + rl_q16 * i32(ssd_one + 4 * chroma_one)
        depth = tried = 0
        if tree_cbf[2 * i + 1] != 0:
            tried = 1
            out[i, 2:6] = [int(s0["cbf"][j0]), i32(int(s0["ssd"][j0])), 0, 0]
            tree[i]["mask_zero"], tree[i]["chroma_ssd_zero"] = tree_cbf[2 * i], i32(chroma_zero)
            cost[i, 0] = int(tree_rate[2 * i]) + rl_q16 * i32(int(s0["ssd"][j0]) + 4 * chroma_zero)
            depth = 0 if cost[i, 0] < cost[i, 1] else 1
        out[i, 0], out[i, 1] = depth, tried
    rec = out.reshape(-1).view(RQT_RESULT_DT).copy()
    rec["cost_zero"], rec["cost_one"] = cost[:, 0], cost[:, 1]
    return rec, tree


class DecisionClient:
    """tests/tree_decide_client.cpp: search/tu_decision.hpp's decideRqt with a tree rate and the chroma functor, compiled at test time"""

    def __init__(self):
        self._tmp = tempfile.TemporaryDirectory()
        so = os.path.join(self._tmp.name, "libtree_decide_client.so")
        subprocess.check_call(["g++", "-O1", "-std=c++14", "-fPIC", "-shared", "-Wall", "-o", so, os.path.join(ROOT, "tests", "tree_decide_client.cpp")])
        self.L = C.CDLL(so)
        self.L.tree_decide.restype = C.c_int
        self.L.tree_decide.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_void_p]

    def decide(self, rows, rl_q16):
        """rows: int64 [n, 13] (see the client) -> int64 [n, 5]: depth, tried_zero, cost_zero, cost_one, depth-0 blocks evaluated"""
        rows = np.ascontiguousarray(rows, np.int64)
        out = np.zeros((len(rows), 5), np.int64)
        assert self.L.tree_decide(rows.ctypes.data, len(rows), rl_q16, out.ctypes.data) == 0
        return out


def random_trees(seed, n):
    """n units of 8x8 .. 32x32 with arbitrary outcomes, masks and rates, laid out as DecisionPicture's tree plan lays them out: luma candidates per transform size
    (depth 0 of a unit, the four depth-1 blocks of a unit of the next larger size), chroma candidates per chroma size (Cb then Cr of depth 0; four Cb then four Cr of
    depth 1), the luma cbf of a candidate equal to its mask bit.  The first units are made cases: 0-1 ties (depth 1 stands), 2 a depth-1 tree coded in chroma only
    (no short-cut), 3 an uncoded tree, 4-5 a pair that the factor 4 on chroma flips.  -> (units, zero_at, one_at, sizes, csizes, chroma_at, tree_rate, tree_cbf)"""
    from turingcodec_amd.decisions import RQT_CU_DT
    from turingcodec_amd.havoc import RQT_CHROMA_AT_DT
    rng = np.random.default_rng(seed)
    units = np.zeros(n, RQT_CU_DT)
    units["log2_size"] = rng.integers(3, 6, n)
    units["log2_size"][:6] = [4, 3, 5, 4, 5, 5][:n]
    units["x0"], units["y0"] = 32 * (np.arange(n) % 8), 32 * (np.arange(n) // 8)
    count, ccount = {s: 0 for s in (2, 3, 4, 5)}, {s: 0 for s in (2, 3, 4)}
    zero_at, one_at, chroma_at = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, RQT_CHROMA_AT_DT)
    for i, L in enumerate(units["log2_size"]):
        zero_at[i], one_at[i] = count[L], count[L - 1]
        count[L] += 1
        count[L - 1] += 4
        c = max(L - 1, 2)
        chroma_at[i]["cb_zero"], chroma_at[i]["cr_zero"] = ccount[c], ccount[c] + 1
        ccount[c] += 2
        if L > 3:
            chroma_at[i]["cb_one"], chroma_at[i]["cr_one"] = ccount[L - 2], ccount[L - 2] + 4
            ccount[L - 2] += 8
        else:
            chroma_at[i]["cb_one"], chroma_at[i]["cr_one"] = chroma_at[i]["cb_zero"], chroma_at[i]["cr_zero"]
    sizes = {s: dict(cbf=np.zeros(m, np.int32), ssd=rng.integers(0, 60000, m).astype(np.uint32)) for s, m in count.items()}
    csizes = {s: dict(cbf=np.zeros(m, np.int32), ssd=rng.integers(0, 20000, m).astype(np.uint32)) for s, m in ccount.items()}
    tree_rate = rng.integers(0, 1 << 27, 2 * n).astype(np.int64)
    tree_cbf = np.zeros(2 * n, np.uint32)
    for i, L in enumerate(units["log2_size"]):
        nc = 4 if L > 3 else 1
        kind = rng.integers(0, 6)
        one = int(rng.integers(1, 16)) | int(rng.integers(0, 1 << nc)) << 4 | int(rng.integers(0, 1 << nc)) << 8
        if kind == 0:
            one = 0                                                      # uncoded
        elif kind == 1:
            one &= 0xff0                                                 # chroma only
            one |= 0 if one else 0x100
        tree_cbf[2 * i + 1] = one
        tree_cbf[2 * i] = int(rng.integers(0, 2)) | int(rng.integers(0, 2)) << 4 | int(rng.integers(0, 2)) << 8
    # ---- the made cases
    def set_unit(i, ssd_y1, ssd_c1, rate1, mask1, ssd_y0, ssd_c0, rate0, mask0=0x111):
        L = int(units["log2_size"][i])
        a = chroma_at[i]
        sizes[L - 1]["ssd"][one_at[i]:one_at[i] + 4] = ssd_y1
        sizes[L]["ssd"][zero_at[i]] = ssd_y0
        csizes[max(L - 1, 2)]["ssd"][[a["cb_zero"], a["cr_zero"]]] = ssd_c0
        if L > 3:
            csizes[L - 2]["ssd"][a["cb_one"]:a["cb_one"] + 4] = ssd_c1[0]
            csizes[L - 2]["ssd"][a["cr_one"]:a["cr_one"] + 4] = ssd_c1[1]
        tree_rate[2 * i + 1], tree_rate[2 * i], tree_cbf[2 * i + 1], tree_cbf[2 * i] = rate1, rate0, mask1, mask0

    if n >= 6:
        set_unit(0, [10, 20, 30, 40], ([1, 2, 3, 4], [5, 6, 7, 8]), 5000, 0x3, 244 - 4 * 7, [3, 4], 5000)        # equal distortions and rates: a tie
        set_unit(1, [7, 7, 7, 7], None, 100 << 16, 0x1, 28, [9, 11], 100 << 16)                                      # 8x8: the chroma is shared; a tie
        set_unit(2, [50, 50, 50, 50], ([0, 0, 0, 9], [0, 0, 0, 0]), 7 << 16, 0x080, 150, [1, 1], 6 << 16, 0x001)    # depth 1 coded in Cb block 3 only
        set_unit(3, [5, 5, 5, 5], ([0, 0, 0, 0], [0, 0, 0, 0]), 0, 0, 0, [0, 0], 0, 0x111)                          # uncoded: depth 0 never tried, though cheaper
        # the factor 4: luma alone prefers depth 0 (1000 < 1100), 4 x chroma turns it round (1000 + 4 * 100 > 1100 + 4 * 40) -- and the other way in unit 5
        set_unit(4, [275, 275, 275, 275], ([10, 10, 10, 10], [0, 0, 0, 0]), 1 << 16, 0x0ff, 1000, [50, 50], 1 << 16)
        set_unit(5, [225, 225, 225, 225], ([25, 25, 25, 25], [0, 0, 0, 0]), 1 << 16, 0x0ff, 1000, [20, 20], 1 << 16)
    for i, L in enumerate(units["log2_size"]):      # a candidate's cbf = its mask bit
        a, nc = chroma_at[i], 4 if L > 3 else 1
        for k in range(4):
            sizes[L - 1]["cbf"][one_at[i] + k] = int(tree_cbf[2 * i + 1]) >> k & 1
        sizes[L]["cbf"][zero_at[i]] = int(tree_cbf[2 * i]) & 1
        c0 = csizes[max(L - 1, 2)]
        c0["cbf"][a["cb_zero"]], c0["cbf"][a["cr_zero"]] = int(tree_cbf[2 * i]) >> 4 & 1, int(tree_cbf[2 * i]) >> 8 & 1
        if L > 3:
            for k in range(4):
                csizes[L - 2]["cbf"][a["cb_one"] + k] = int(tree_cbf[2 * i + 1]) >> (4 + k) & 1
                csizes[L - 2]["cbf"][a["cr_one"] + k] = int(tree_cbf[2 * i + 1]) >> (8 + k) & 1
    return units, zero_at, one_at, sizes, csizes, chroma_at, tree_rate, tree_cbf


def client_rows(units, zero_at, one_at, sizes, csizes, chroma_at, tree_rate, tree_cbf):
    """the int64 [n, 13] rows tests/tree_decide_client.cpp takes, from the same tables"""
    rows = np.zeros((len(units), 13), np.int64)
    for i, u in enumerate(units):
        L, a = int(u["log2_size"]), chroma_at[i]
        j0, j1 = int(zero_at[i]), int(one_at[i])
        c0 = csizes[max(L - 1, 2)]["ssd"]
        cb0, cr0 = int(c0[a["cb_zero"]]), int(c0[a["cr_zero"]])
        if L > 3:
            c1 = csizes[L - 2]["ssd"]
            cb1, cr1 = int(c1[a["cb_one"]:a["cb_one"] + 4].astype(np.int64).sum()), int(c1[a["cr_one"]:a["cr_one"] + 4].astype(np.int64).sum())
        else:
            cb1, cr1 = cb0, cr0
        rows[i] = [int(tree_cbf[2 * i + 1])] + [int(v) for v in sizes[L - 1]["ssd"][j1:j1 + 4]] + [cb1, cr1, int(tree_rate[2 * i + 1]),
                                                                                                   int(tree_cbf[2 * i]), int(sizes[L]["ssd"][j0]), cb0, cr0, int(tree_rate[2 * i])]
    return rows
