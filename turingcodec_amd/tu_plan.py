"""The formats of DecisionPicture's transform chains, one copy each, as plain numpy tables (no device, no buffers): the RDOQ job records of a group of transform
blocks, where the candidates of a list of units' transform trees lie, and the tree-rate job records made from that layout.  decisions.py gives them buffers and
issues the launches.

A CANDIDATE is one transform block a unit's tree decision tries: at depth 0 the unit's own block, at depth 1 one of its four quarters (k in z-order).  The luma
candidates of one transform size form a list, the chroma candidates of one chroma transform size another; a candidate's index in its list names its slot in the
list's coefficient / level / piece buffers.
"""
import numpy as np

from . import workload
from .havoc import RDOQ_JOB_DT, RQT_CHROMA_AT_DT, TREE_RATE_JOB_DT, TREE_RATE_SPLIT_FLAG_CODED, rdoq_lambda


def quantiser(qp, bit_depth, log2):
    """(quant_scale, quant_shift, inv_scale, dequant_shift) of a 2^log2 transform block of an inter unit -- luma and chroma alike (turing/QpState.h:85-94,
    Reconstruct.cpp:774-782)"""
    qs, qshift, _ = workload.quant_params(qp, log2, bit_depth, False)
    inv, dshift = workload.dequant_params(qp, log2, bit_depth)
    return int(qs), int(qshift), int(inv), int(dshift)


def rdoq_jobs(qp, bit_depth, lam, log2, block_off, ctx_index, c_idx=0):
    """the RDOQ_JOB_DT records of a group of 2^log2 blocks: block_off their slots in the group's coefficient and level buffers, ctx_index their CABAC snapshots,
    c_idx 0 luma / 1 Cb / 2 Cr (one value or one per block); sign data hiding on.  Returns (records, inv_scale, dequant_shift)"""
    qs, qshift, inv, dshift = quantiser(qp, bit_depth, log2)
    rj = np.zeros(len(block_off), RDOQ_JOB_DT)
    rj["dst_off"] = rj["src_off"] = block_off
    rj["quant_scale"], rj["quant_shift"], rj["inv_scale"] = qs, qshift, inv
    rj["lambda_q16"], rj["sdh_factor"] = rdoq_lambda(lam, inv)
    rj["sdh"], rj["c_idx"], rj["ctx_index"] = 1, c_idx, ctx_index
    return rj, inv, dshift


def candidate_layout(log2_size):
    """where the candidates of units of sizes 2^log2_size[i] (3..6) lie: dict(luma={transform size: int64 [m, 3] (unit, depth, k)}, chroma={chroma transform size:
    int64 [m, 4] (unit, depth, component, k)}, zero_at, one_at int32 [n]: the unit's depth-0 candidate and the first of its four depth-1 candidates in their luma
    lists, chroma_at RQT_CHROMA_AT_DT [n]: the same for Cb and Cr).  Per luma list: depth 0 of every unit of that size, then the four quarters of every unit of the
    next larger size, unit by unit.  Per chroma list: a unit's depth-0 Cb and Cr block of max(L - 1, 2); for L > 3 its four depth-1 Cb blocks, then its four Cr
    blocks, of L - 2; an 8x8 unit's one 4x4 block per component serves both depths.  A 64x64 unit has no depth-0 candidate in any plane (its split is inferred):
    -1.  Sizes without a candidate are left out of luma / chroma"""
    n = len(log2_size)
    lists, clists = {s: [] for s in (2, 3, 4, 5)}, {s: [] for s in (2, 3, 4)}
    zero_at, one_at, chroma_at = np.full(n, -1, np.int32), np.zeros(n, np.int32), np.zeros(n, RQT_CHROMA_AT_DT)
    for i in range(n):
        L, a = int(log2_size[i]), chroma_at[i]
        if L < 6:
            zero_at[i] = len(lists[L])
            lists[L].append((i, 0, 0))
            c0 = max(L - 1, 2)
            a["cb_zero"], a["cr_zero"] = len(clists[c0]), len(clists[c0]) + 1
            clists[c0] += [(i, 0, 1, 0), (i, 0, 2, 0)]
        else:
            a["cb_zero"], a["cr_zero"] = -1, -1
        one_at[i] = len(lists[L - 1])
        lists[L - 1] += [(i, 1, k) for k in range(4)]
        if L > 3:
            a["cb_one"], a["cr_one"] = len(clists[L - 2]), len(clists[L - 2]) + 4
            clists[L - 2] += [(i, 1, comp, k) for comp in (1, 2) for k in range(4)]
        else:
            a["cb_one"], a["cr_one"] = a["cb_zero"], a["cr_zero"]
    return dict(luma={s: np.array(c, np.int64) for s, c in lists.items() if c}, chroma={s: np.array(c, np.int64) for s, c in clists.items() if c},
                zero_at=zero_at, one_at=one_at, chroma_at=chroma_at)


def candidate_xy(x0, y0, cand, log2, chroma=False):
    """the top-left sample of every candidate of a list of transform size 2^log2 in its plane (chroma: the half-size plane); x0, y0: the units' luma positions"""
    unit, split, k, nn = cand[:, 0], cand[:, 1] == 1, cand[:, -1], 1 << log2
    return ((x0[unit] >> int(chroma)) + np.where(split, (k & 1) * nn, 0), (y0[unit] >> int(chroma)) + np.where(split, (k >> 1) * nn, 0))


def tree_rate_jobs(layout, log2_size, ctx_index):
    """{(L, depth): (TREE_RATE_JOB_DT records of the units of size 2^L, in their order; the luma list; the chroma list their levels lie in)}: every tree from the
    unit's snapshot, out_index = 2 * unit + depth.  split_transform_flag is coded for units of 8 .. 32 (MaxTrafoDepth 1, MinTbLog2SizeY 2, MaxTbLog2SizeY 5); a
    64x64 unit has its depth-1 tree only and no flag bin"""
    out = {}
    for L in (6, 5, 4, 3):
        sel = np.flatnonzero(log2_size == L)
        if not len(sel):
            continue
        for depth in ((1,) if L == 6 else (0, 1)):
            luma, chroma = L - depth, max(L - 1 - depth, 2)
            at, cb, cr = (layout["one_at"], "cb_one", "cr_one") if depth else (layout["zero_at"], "cb_zero", "cr_zero")
            tj = np.zeros(len(sel), TREE_RATE_JOB_DT)
            tj["luma_off"], tj["cb_off"], tj["cr_off"] = at[sel] << 2 * luma, layout["chroma_at"][cb][sel] << 2 * chroma, layout["chroma_at"][cr][sel] << 2 * chroma
            tj["ctx_index"], tj["out_index"], tj["sdh"] = ctx_index[sel], 2 * sel + depth, 1
            tj["flags"] = TREE_RATE_SPLIT_FLAG_CODED if L < 6 else 0
            out[L, depth] = (tj, luma, chroma)
    return out
