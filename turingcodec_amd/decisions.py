"""Host-side binding of libhavoc_search.so's PICTURE client (turingcodec_amd/search/picture_search.cpp): a whole picture's
uni-directional motion searches in wavefront order with predictors derived from earlier decisions (search/picture_order.hpp).

Plain ctypes over raw device pointers and a havoc_mi355x context handle, so that the same binding drives the real library (bench.py,
-m gpu tests) and the CPU stand-in device of the host-logic tests.  There is no CPU path here: the library it loads launches kernels.
"""
import ctypes as C
import os
import typing

import numpy as np

from . import tu_plan
from .workload import PICTURE_PU_DT

_HERE = os.path.dirname(os.path.abspath(__file__))
SEARCH_LIB = os.path.join(_HERE, "libhavoc_search.so")

RESULT_DT = np.dtype([("mv", "i2", (2,)), ("mvd", "i2", (2,)), ("mv_integer", "i2", (2,)), ("mvp_flag", "i2"), ("wrote_2Nx2N", "i2"),
                      ("calls", "i4"), ("replays", "i4"), ("cost_integer", "i8"), ("cost_subpel", "i8"), ("cost_mvd_zero", "i8", (2,))])
assert RESULT_DT.itemsize == 56 and PICTURE_PU_DT.itemsize == 32


class SearchParams(C.Structure):
    """havoc_search_params (search/search_abi.h): what the loops read from encoder state"""
    _fields_ = [("pic_width", C.c_int32), ("pic_height", C.c_int32), ("ctb_size", C.c_int32), ("concurrent_frames", C.c_int32),
                ("met", C.c_int32), ("small_search_window", C.c_int32), ("bi_small_search_window", C.c_int32), ("half_pel", C.c_int32),
                ("quarter_pel", C.c_int32), ("bit_depth", C.c_int32), ("reciprocal_sqrt_lambda", C.c_double)]


class PictureStats(C.Structure):
    """havoc_picture_stats"""
    _fields_ = [("steps", C.c_int32), ("rounds", C.c_int32), ("max_rounds_in_step", C.c_int32), ("launches", C.c_int32), ("surfaces_small", C.c_int32),
                ("surfaces_zero", C.c_int32), ("surfaces_large", C.c_int32), ("satd_jobs", C.c_int32), ("speculative_runs", C.c_int32), ("reruns", C.c_int32),
                ("bytes_down", C.c_int64), ("seconds_gpu", C.c_double), ("seconds_host", C.c_double), ("seconds_total", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


RQT_CU_DT = np.dtype([("x0", "i4"), ("y0", "i4"), ("log2_size", "i4"), ("ctx_index", "i4")])                       # havoc_rqt_cu
TU_OUTCOME_DT = np.dtype([("cbf", "i4"), ("ssd", "u4"), ("nonzero", "i4"), ("sum_abs", "i4")])                    # havoc_tu_outcome
RQT_RESULT_DT = np.dtype([("depth", "i4"), ("tried_zero", "i4"), ("zero", TU_OUTCOME_DT), ("one", TU_OUTCOME_DT, (4,)), ("cost_zero", "i8"),
                          ("cost_one", "i8")])                                                                     # havoc_rqt_result
assert RQT_CU_DT.itemsize == 16 and RQT_RESULT_DT.itemsize == 104


INTRA_CTX_DT = np.dtype([("cand_mode_list", "i4", (3,)), ("neighbour_modes", "i4"), ("max_refine", "i4"), ("reserved", "i4"), ("rate_a_minus_c", "i8"),
                         ("rate_b_minus_c", "i8")])                                                               # havoc_search_intra_ctx
INTRA_RESULT_DT = np.dtype([("costs", "i8", (35,)), ("order", "i4", (35,)), ("count", "i4")])                       # havoc_search_intra_result
INTRA_RD_RESULT_DT = np.dtype([("mode", "i4"), ("index", "i4"), ("evaluated", "i4"), ("reserved", "i4"), ("cost", "i8"), ("outcome", TU_OUTCOME_DT)])
assert INTRA_CTX_DT.itemsize == 40 and INTRA_RESULT_DT.itemsize == 424 and INTRA_RD_RESULT_DT.itemsize == 40


class RqtStats(C.Structure):
    _fields_ = [("launches", C.c_int32), ("candidates", C.c_int32), ("seconds_gpu", C.c_double), ("seconds_host", C.c_double), ("seconds_total", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def rqt_quant(qp, bit_depth):
    """havoc_rqt_quant[4] for transform sizes 4..32 of an inter (non-I slice) luma block (turing/QpState.h:85-94, Reconstruct.cpp:774-782)"""
    return np.array([tu_plan.quantiser(qp, bit_depth, log2) for log2 in (2, 3, 4, 5)], np.int32)


def medium_params(width, height, bit_depth, reciprocal_sqrt_lambda, concurrent_frames=4):
    """speed=medium: multiple early termination on, full search window, half- and quarter-sample refinement (turing/Speed.h)"""
    return SearchParams(width, height, 64, concurrent_frames, 1, 0, 0, 1, 1, bit_depth, reciprocal_sqrt_lambda)


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SEARCH_LIB):
            raise RuntimeError(f"{SEARCH_LIB} is missing: build it with `make -C turingcodec_amd/csrc` -- there is no fallback path")
        L = C.CDLL(SEARCH_LIB)
        vp, ip, i64 = C.c_void_p, C.c_ssize_t, C.c_int64
        L.havoc_search_picture_uni.argtypes = [vp, C.c_int, C.POINTER(SearchParams), vp, i64, ip, vp, C.POINTER(i64), ip, C.c_int, vp, ip, C.POINTER(i64),
                                               vp, vp, C.c_int, C.c_int, C.POINTER(i64), vp, vp, C.c_int, C.POINTER(PictureStats)]
        L.havoc_search_picture_uni.restype = C.c_int
        L.havoc_search_picture_uni_device.argtypes = [vp, C.c_int, C.POINTER(SearchParams), vp, i64, ip, vp, C.POINTER(i64), ip, C.c_int, vp, ip, C.POINTER(i64),
                                                      vp, vp, C.c_int, C.c_int, C.POINTER(i64), vp, vp, vp, vp, C.POINTER(PictureStats)]
        L.havoc_search_picture_uni_device.restype = C.c_int
        L.havoc_search_rqt.argtypes = [vp, C.c_int, C.c_int, vp, i64, ip, vp, ip, vp, i64, ip, vp, vp, C.c_double, C.c_double, C.c_int, vp, C.c_int, vp,
                                       C.POINTER(RqtStats)]
        L.havoc_search_rqt.restype = C.c_int
        L.havoc_search_intra_rd.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, ip, vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_double, C.c_double, C.c_int, vp, vp,
                                            C.POINTER(RqtStats)]
        L.havoc_search_intra_rd.restype = C.c_int
        L.havoc_search_intra_device.argtypes = [vp, C.c_int, C.c_int, vp, ip, vp, C.c_int, vp, vp, C.c_double, C.c_double, C.c_double, C.c_int, C.POINTER(RqtStats)]
        L.havoc_search_intra_device.restype = C.c_int
        L.havoc_search_intra_device_rated.argtypes = [vp, C.c_int, C.c_int, vp, ip, vp, C.c_int, vp, vp, vp, vp, C.c_double, C.c_double, C.c_double, C.c_int,
                                                      C.POINTER(RqtStats)]
        L.havoc_search_intra_device_rated.restype = C.c_int
        L.havoc_search_intra_rate_flags.argtypes = [C.c_int] * 5
        L.havoc_search_intra_rate_flags.restype = C.c_int
        L.havoc_search_intra_modes.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, ip, vp, vp, C.c_int, vp, C.c_double, vp, vp]
        L.havoc_search_intra_modes.restype = C.c_int
        L.havoc_search_intra_chain.argtypes = [vp, C.c_int, C.c_int, vp, vp, ip, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_double, C.c_double, C.c_double, C.c_int, vp]
        L.havoc_search_intra_chain.restype = C.c_int
        L.havoc_search_block_cells.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp]
        L.havoc_search_block_cells.restype = C.c_int
        L.havoc_search_release.argtypes = [vp]
        L.havoc_search_release.restype = None
        _lib = L
    return _lib


def picture_uni(ctx, S, params, d_src, src_origin, src_stride, d_ref, ref_origin, ref_stride, ref_pad, d_phase, plane_elems, phase_origin, pus, ctu_first,
                ctus_x, ctus_y, mvp_rate=(65536, 65536), threads=16, want_field=True, on_device=False, d_field_keep=None, bi=False):
    """havoc_search_picture_uni (launch + host replay rounds) or, on_device, havoc_search_picture_uni_device (the decision loops inside the kernel).
    ctx: havoc_mi355x context handle (int / c_void_p); d_*: device addresses (ints); ref_origin / phase_origin:
    pairs (list 0, list 1).  Returns (results [2 * len(pus)] RESULT_DT indexed 2 * p + list, field int16 [2, cells_y, cells_x, 2] or None, stats);
    with bi (device search only) the bi-directional refinements [2 * len(pus)] as a fourth value."""
    pus = np.ascontiguousarray(pus)
    assert pus.dtype == PICTURE_PU_DT
    ctu_first = np.ascontiguousarray(ctu_first, np.int32)
    out = np.zeros(2 * len(pus), RESULT_DT)
    cw, ch = (params.pic_width + 3) // 4, (params.pic_height + 3) // 4
    field = np.zeros((2, ch, cw, 2), np.int16) if want_field else None
    stats = PictureStats()
    ro = (C.c_int64 * 2)(*[int(v) for v in ref_origin])
    po = (C.c_int64 * 2)(*[int(v) for v in phase_origin])
    mr = (C.c_int64 * 2)(*[int(v) for v in mvp_rate])
    out_bi = np.zeros(2 * len(pus), RESULT_DT) if bi else None
    if bi and not on_device:
        raise ValueError("the bi-directional refinement inside the picture walk exists in the device search only")
    if on_device:
        rc = lib().havoc_search_picture_uni_device(ctx, S, C.byref(params), d_src, int(src_origin), src_stride, d_ref, ro, ref_stride, ref_pad, d_phase, plane_elems, po,
                                                   pus.ctypes.data, ctu_first.ctypes.data, ctus_x, ctus_y, mr, out.ctypes.data,
                                                   field.ctypes.data if want_field else None, d_field_keep, out_bi.ctypes.data if bi else None, C.byref(stats))
    else:
        rc = lib().havoc_search_picture_uni(ctx, S, C.byref(params), d_src, int(src_origin), src_stride, d_ref, ro, ref_stride, ref_pad, d_phase, plane_elems, po,
                                            pus.ctypes.data, ctu_first.ctypes.data, ctus_x, ctus_y, mr, out.ctypes.data,
                                            field.ctypes.data if want_field else None, threads, C.byref(stats))
    if rc != 0:
        raise RuntimeError(f"havoc_search_picture_uni{'_device' if on_device else ''} failed ({rc})")
    return (out, field, stats, out_bi) if bi else (out, field, stats)


def decision_inputs(width, height, bit_depth=8, qp=32, seed=11, density=1.0, frames=None, distance=1):
    """host side of a DecisionPicture: padded luma planes (source, list 0, list 1), the picture's PUs in decision order, search parameters.
    distance: temporal distance of the two reference pictures (1 = the leaf B pictures of the hierarchy, half of a SOP of 8; 2, 4, 8 = its upper
    layers, whose vectors are longer and whose searches run the star / raster refinement far more often)"""
    from . import workload
    pad = 96
    if frames is None:
        frames = workload.synth_frames(width, height, 2 * distance + 1, seed, bit_depth)
        frames = [frames[0], frames[distance], frames[2 * distance]]
    planes = [workload.pad_plane(f[0], pad) for f in (frames[1], frames[0], frames[2])]
    stride = planes[0].shape[1]
    # chroma: Cb of (source, list 0, list 1), then Cr, in the same padded layout at half size (48 samples of border)
    chroma = [workload.pad_plane(f[c], pad // 2) for c in (1, 2) for f in (frames[1], frames[0], frames[2])]
    pus, ctu_first, cx, cy = workload.picture_pus(width, height, seed, density)
    lam = workload.picture_lambda(qp)
    return dict(chroma=[np.ascontiguousarray(p.ravel()) for p in chroma], cstride=chroma[0].shape[1],
                planes=[np.ascontiguousarray(p.ravel()) for p in planes], stride=stride, pad=pad, pus=pus, ctu_first=ctu_first, cx=cx, cy=cy,
                params=medium_params(width, height, bit_depth, 1.0 / np.sqrt(lam)), mvp_rate=(45000, 98000), lam=lam)


def rqt(ctx, S, bit_depth, d_src, src_origin, src_stride, d_pred, pred_stride, d_rec, rec_origin, rec_stride, d_states, quant, lam, reciprocal_lambda, cus, sdh=1):
    """havoc_search_rqt: the residual-quadtree decision of every inter unit of `cus` (RQT_CU_DT) in one chain per transform size.
    Returns (results RQT_RESULT_DT, stats)"""
    cus = np.ascontiguousarray(cus)
    assert cus.dtype == RQT_CU_DT
    quant = np.ascontiguousarray(quant, np.int32)
    out = np.zeros(len(cus), RQT_RESULT_DT)
    stats = RqtStats()
    rc = lib().havoc_search_rqt(ctx, S, bit_depth, d_src, int(src_origin), src_stride, d_pred, pred_stride, d_rec, int(rec_origin), rec_stride, d_states,
                                quant.ctypes.data, float(lam), float(reciprocal_lambda), int(sdh), cus.ctypes.data, len(cus), out.ctypes.data, C.byref(stats))
    if rc != 0:
        raise RuntimeError(f"havoc_search_rqt failed ({rc})")
    return out, stats


def intra_rd(ctx, S, bit_depth, log2, d_src, src_stride, d_neighbours, jobs, order, ictx, ctx_index, d_states, quant_row, lam, reciprocal_lambda, d_rec, sdh=1):
    """havoc_search_intra_rd: the RD refinement of n intra partitions of one size (jobs: int32 [n, 8] havoc_mi355x_intra_search_job rows on the
    HOST; order: INTRA_RESULT_DT from the 35-mode stage; quant_row: int32[4] of rqt_quant for this size).  Returns (INTRA_RD_RESULT_DT[n], stats)"""
    jobs = np.ascontiguousarray(jobs, np.int32)
    order = np.ascontiguousarray(order)
    ictx = np.ascontiguousarray(ictx)
    ctx_index = np.ascontiguousarray(ctx_index, np.int32)
    quant_row = np.ascontiguousarray(quant_row, np.int32)
    out = np.zeros(len(jobs), INTRA_RD_RESULT_DT)
    stats = RqtStats()
    rc = lib().havoc_search_intra_rd(ctx, S, bit_depth, log2, d_src, src_stride, d_neighbours, jobs.ctypes.data, len(jobs), order.ctypes.data, ictx.ctypes.data,
                                     ctx_index.ctypes.data, d_states, quant_row.ctypes.data, float(lam), float(reciprocal_lambda), int(sdh), d_rec, out.ctypes.data,
                                     C.byref(stats))
    if rc != 0:
        raise RuntimeError(f"havoc_search_intra_rd failed ({rc})")
    return out, stats


INTRA_GROUP_DT = np.dtype([("log2", "i4"), ("n", "i4"), ("d_neighbours", "u8"), ("d_jobs", "u8"), ("d_ictx", "u8"), ("d_ctx_index", "u8"), ("d_rec", "u8"),
                           ("out", "u8")])                                                                       # havoc_intra_group
assert INTRA_GROUP_DT.itemsize == 56


INTRA_CHAIN_SIZE_DT = np.dtype([("log2", "i4"), ("n", "i4"), ("d_neighbours", "u8"), ("d_jobs", "u8"), ("d_ictx", "u8"), ("d_ctx_index", "u8"), ("d_parts", "u8"),
                                ("d_blocks", "u8"), ("first", "u8"), ("out", "u8")])                                  # havoc_intra_chain_size
assert INTRA_CHAIN_SIZE_DT.itemsize == 72


def _address(p):
    return int(p.value or 0) if isinstance(p, C.c_void_p) else int(p)


SEARCH_ENOTAVAILABLE = -200      # HAVOC_SEARCH_ENOTAVAILABLE


def intra_rate_flags(log2, intra_split, max_transform_hierarchy_depth_intra=1, min_tb_log2=2, max_tb_log2=5):
    """havoc_search_intra_rate_flags: the INTRA_RATE_* bits of an intra partition's transform block -- whether transform_tree codes split_transform_flag for it, and
    whether its trafoDepth is non-zero (intra_split: one of the four partitions of an NxN unit).  The defaults are the reference encoder's set-up."""
    return lib().havoc_search_intra_rate_flags(int(log2), int(bool(intra_split)), int(max_transform_hierarchy_depth_intra), int(min_tb_log2), int(max_tb_log2))


def intra_device(ctx, S, bit_depth, d_src, src_stride, groups, d_states, quant, reciprocal_sqrt_lambda, lam, reciprocal_lambda, sdh=1, rates="stand-in",
                 d_syntax_states=None):
    """havoc_search_intra_device: both stages of the intra partitions of all sizes, the decisions between the launches taken on the device.
    groups: dicts(log2, n, d_nb, d_jobs, d_ictx, d_ctu, d_rec) of device addresses; quant: int32 [4, 4] (rqt_quant).
    rates="cabac" (havoc_search_intra_device_rated): every candidate is priced with the bits the reference's EstimateRateLuma measures for it -- mode bits,
    split_transform_flag, cbf_luma, residual_coding, from the partition's snapshot -- instead of the stand-in.  d_syntax_states: 4 bytes per snapshot of d_states
    (prev_intra_luma_pred_flag, split_transform_flag[0..2]); a group may carry "flags" (INTRA_RATE_*; default: a 2Nx2N partition, except 4x4: one of an NxN unit,
    in the reference encoder's set-up).  Returns ({log2: INTRA_RD_RESULT_DT[n]}, stats)"""
    if rates not in ("stand-in", "cabac"):
        raise ValueError(f"rates must be 'stand-in' or 'cabac', not {rates!r}")
    if (rates == "cabac") != (d_syntax_states is not None):
        raise ValueError("d_syntax_states goes with rates='cabac', and only with it")
    table = np.zeros(len(groups), INTRA_GROUP_DT)
    outs = {}
    for row, g in zip(table, groups):
        out = np.zeros(g["n"], INTRA_RD_RESULT_DT)
        outs[g["log2"]] = out
        row["log2"], row["n"] = g["log2"], g["n"]
        for k, name in (("d_nb", "d_neighbours"), ("d_jobs", "d_jobs"), ("d_ictx", "d_ictx"), ("d_ctu", "d_ctx_index"), ("d_rec", "d_rec")):
            row[name] = _address(g[k])
        row["out"] = out.ctypes.data
    quant = np.ascontiguousarray(quant, np.int32)
    stats = RqtStats()
    if rates == "cabac":
        flags = np.array([g["flags"] if "flags" in g else intra_rate_flags(g["log2"], g["log2"] == 2) for g in groups], np.int32)
        rc = lib().havoc_search_intra_device_rated(ctx, S, bit_depth, d_src, src_stride, table.ctypes.data, len(table), d_states, _address(d_syntax_states),
                                                   flags.ctypes.data, quant.ctypes.data, float(reciprocal_sqrt_lambda), float(lam), float(reciprocal_lambda), int(sdh),
                                                   C.byref(stats))
        if rc == SEARCH_ENOTAVAILABLE:
            raise RuntimeError("havoc_search_intra_device_rated: the device library has no havoc_mi355x_intra_rate / _intra_rate_jobs / _intra_decide_rated "
                               "(there is no fallback to the stand-in rate)")
        if rc != 0:
            raise RuntimeError(f"havoc_search_intra_device_rated failed ({rc})")
        return outs, stats
    rc = lib().havoc_search_intra_device(ctx, S, bit_depth, d_src, src_stride, table.ctypes.data, len(table), d_states, quant.ctypes.data, float(reciprocal_sqrt_lambda),
                                         float(lam), float(reciprocal_lambda), int(sdh), C.byref(stats))
    if rc != 0:
        raise RuntimeError(f"havoc_search_intra_device failed ({rc})")
    return outs, stats


def intra_modes(ctx, S, bit_depth, log2, d_src, src_stride, d_neighbours, d_jobs, n, ictx, reciprocal_sqrt_lambda):
    """havoc_search_intra_modes: the 35-mode SATD stage of n partitions of one size + the order their modes are refined in (Search.hpp:40-190).
    d_jobs: device copy of the int32 [n, 8] job rows.  Returns INTRA_RESULT_DT[n]"""
    ictx = np.ascontiguousarray(ictx)
    out = np.zeros(n, INTRA_RESULT_DT)
    rc = lib().havoc_search_intra_modes(ctx, S, bit_depth, log2, d_src, src_stride, d_neighbours, d_jobs, n, ictx.ctypes.data, float(reciprocal_sqrt_lambda),
                                        out.ctypes.data, None)
    if rc != 0:
        raise RuntimeError(f"havoc_search_intra_modes failed ({rc})")
    return out


def intra_chain_tables(width, height, bit_depth, qp, seed, stride, pad):
    """host side of an intra picture's dependency chain (IntraChainPicture; tests/intra_chain_runner.py drives the same tables through the CPU stand-in device): the
    partitions, their owner map and levels (workload.intra_picture_partitions), and per partition size -- ordered by level -- the job records, the most-probable-mode
    records (rates and max_refine; the modes are derived from the neighbours' champions as the chain runs), CABAC snapshot indices, chain records and level slices"""
    from . import workload
    parts, owner, level = workload.intra_picture_partitions(width, height, seed + 3)
    cx = (width + 63) // 64
    lam = workload.picture_lambda(qp)
    rng = np.random.default_rng(seed + 7919)
    base = rng.integers(4, 100, 128)
    rdoq_states = np.clip(base[None, :] + rng.integers(-6, 7, (cx * ((height + 63) // 64), 128)), 0, 125).astype(np.uint8)
    nlevels = int(level.max()) + 1
    sizes = {}
    for log2 in (5, 4, 3, 2):
        sel = np.flatnonzero(parts["log2"] == log2)
        if not len(sel):
            continue
        sel = sel[np.argsort(level[sel], kind="stable")]
        m, nn = len(sel), 1 << log2
        L = 4 * nn + 1
        x0, y0 = parts["x0"][sel].astype(np.int64), parts["y0"][sel].astype(np.int64)
        mask = workload.intra_filter_mask(nn)
        jobs = np.zeros((m, 8), np.int64)
        jobs[:, 0] = (y0 + pad) * stride + x0 + pad
        jobs[:, 1] = np.arange(m) * 2 * L + 2 * nn + 1
        jobs[:, 2] = jobs[:, 1] + L
        jobs[:, 3], jobs[:, 4], jobs[:, 5] = mask & 0xffffffff, mask >> 32, 1
        jobs = jobs.astype(np.uint32).view(np.int32).reshape(m, 8)
        ictx = np.zeros(m, INTRA_CTX_DT)
        ictx["max_refine"] = 3 if log2 > 3 else 8            # Speed::nCandidatesIntraRefinement at medium
        ictx["rate_a_minus_c"] = -rng.integers(300000, 420000, m)
        ictx["rate_b_minus_c"] = -rng.integers(100000, 200000, m)
        chain = np.zeros((m, 4), np.int32)
        chain[:, 0], chain[:, 1], chain[:, 2], chain[:, 3] = x0, y0, log2, sel
        ctu = ((y0 // 64) * cx + x0 // 64).astype(np.int32)
        first = np.searchsorted(level[sel], np.arange(nlevels + 1)).astype(np.int64)
        sizes[log2] = dict(sel=sel, m=m, nn=nn, jobs=jobs, ictx=ictx, ctu=ctu, chain=chain, first=first)
    return dict(parts=parts, owner=owner, level=level, nlevels=nlevels, cx=cx, lam=lam, rsl=float(1.0 / np.sqrt(lam)), quant=rqt_quant(qp, bit_depth), rdoq_states=rdoq_states,
                sizes=sizes)


class IntraChainPicture:
    """An INTRA picture with the real dependencies between its partitions (round 4): every partition predicts from the reconstruction
    of the partitions before it and takes its most probable modes from its neighbours' champions (turing/Reconstruct.cpp:609-615, CandModeList.h:33-95), so
    the picture is a dependency graph, cut here into LEVELS of mutually independent partitions (workload.intra_picture_partitions).  A level is one pass of the
    batch chain: reference samples + candModeList gathered on the device from the running reconstruction / mode map (havoc_mi355x_intra_gather), the 35-mode
    SATD stage, the refinement order, every candidate through prediction -> T -> RDOQ -> IQ -> IT -> SSD, the champion (havoc_search_intra_device: decisions on the
    device), and the champions' blocks + modes committed to the picture (havoc_mi355x_intra_commit).  Levels are many (a 4x4 partition's chain reaches across the
    picture: ~600 at 640x360, ~1 900 at 1080p) and each is launch-bound -- the whole picture inside one persistent kernel is the form that would pay; this one is
    the parity-checked statement of the chain."""

    PAD = 96

    def __init__(self, hv, width, height, bit_depth=8, qp=32, seed=11):
        import torch
        from . import havoc as hmod
        from . import workload
        self.hv, self.torch = hv, torch
        self.W, self.H, self.bd, self.qp = width, height, bit_depth, qp
        self.S = 1 if bit_depth == 8 else 2
        self.dt = np.uint8 if self.S == 1 else np.uint16
        src = workload.pad_plane(workload.synth_frames(width, height, 1, seed, bit_depth)[0][0], self.PAD)
        self.stride = src.shape[1]
        self.host_src = np.ascontiguousarray(src.ravel())
        self.n = self.host_src.size
        self.d_src = hv.up(self.host_src)
        self.d_rec = hv.zeros(self.n, self.dt)
        t = intra_chain_tables(width, height, bit_depth, qp, seed, self.stride, self.PAD)
        self.parts, self.owner, self.level, self.nlevels = t["parts"], t["owner"], t["level"], t["nlevels"]
        self.cells_per_row = self.owner.shape[1]
        self.d_owner = hv.up(np.ascontiguousarray(self.owner.ravel()))
        self.d_modes = hv.zeros(self.owner.size, np.uint8)
        self.cx, self.lam, self.rsl, self.quant, self.rdoq_states = t["cx"], t["lam"], t["rsl"], t["quant"], t["rdoq_states"]
        self.d_states = hv.up(self.rdoq_states.reshape(-1))
        self.layout = hv.intra_chain_layout(width, height, self.stride, self.PAD, self.cells_per_row, bit_depth)
        self.sizes = {}
        for log2, g in t["sizes"].items():
            m, nn = g["m"], g["nn"]
            self.sizes[log2] = dict(g, d_jobs=hv.up(g["jobs"]), d_nb=hv.zeros(m * 2 * (4 * nn + 1), self.dt), d_ictx=hv.up(np.ascontiguousarray(g["ictx"]).view(np.int32)),
                                    d_ctu=hv.up(g["ctu"]), d_parts=hv.up(g["chain"]), d_blocks=hv.zeros(m * nn * nn, self.dt), d_mode=hv.zeros(m, np.int32),
                                    best=np.zeros(m, INTRA_RD_RESULT_DT))
        hv.sync()

    def step(self, wait_per_level=False):
        """the picture, level by level; leaves the champions in self.sizes[log2]["best"] (ordered as ["sel"]), the reconstruction in self.d_rec.
        Default: havoc_search_intra_chain -- every level's launches queued without a wait between the levels (the chain runs over the worst-case number of
        candidate slots), one wait at the end.  wait_per_level: the first form of this step, a havoc_search_intra_device call (two waits) per level."""
        hv, S, torch = self.hv, self.S, self.torch
        self.launches = 0
        if not wait_per_level:
            table = np.zeros(len(self.sizes), INTRA_CHAIN_SIZE_DT)
            firsts = []
            for row, (log2, g) in zip(table, self.sizes.items()):
                f = np.ascontiguousarray(g["first"], np.int32)
                firsts.append(f)
                row["log2"], row["n"] = log2, g["m"]
                row["d_neighbours"], row["d_jobs"], row["d_ictx"], row["d_ctx_index"] = g["d_nb"].data_ptr(), g["d_jobs"].data_ptr(), g["d_ictx"].data_ptr(), g["d_ctu"].data_ptr()
                row["d_parts"], row["d_blocks"], row["first"], row["out"] = g["d_parts"].data_ptr(), g["d_blocks"].data_ptr(), f.ctypes.data, g["best"].ctypes.data
            quant = np.ascontiguousarray(self.quant, np.int32)
            stats = RqtStats()
            rc = lib().havoc_search_intra_chain(hv.h, S, self.bd, self.layout, self.d_src.data_ptr(), self.stride, self.d_rec.data_ptr(), self.d_owner.data_ptr(),
                                                self.d_modes.data_ptr(), table.ctypes.data, len(table), self.nlevels, self.d_states.data_ptr(), quant.ctypes.data, self.rsl,
                                                float(self.lam), 1.0 / self.lam, 1, C.byref(stats))
            if rc != 0:
                raise RuntimeError(f"havoc_search_intra_chain failed ({rc})")
            self.launches, self.chain_stats = stats.launches, stats
            return
        for lvl in range(self.nlevels):
            groups, live = [], []
            for log2, g in self.sizes.items():
                a, b = int(g["first"][lvl]), int(g["first"][lvl + 1])
                if b == a:
                    continue
                n, area = b - a, g["nn"] * g["nn"]
                hv.intra_gather_a(S, self.layout, self.d_rec.data_ptr(), self.d_owner.data_ptr(), self.d_modes.data_ptr(), g["d_parts"].data_ptr() + 16 * a, n,
                                  g["d_jobs"].data_ptr() + 32 * a, g["d_nb"].data_ptr(), g["d_ictx"].data_ptr() + 40 * a)
                groups.append(dict(log2=log2, n=n, d_nb=g["d_nb"].data_ptr(), d_jobs=g["d_jobs"].data_ptr() + 32 * a, d_ictx=g["d_ictx"].data_ptr() + 40 * a,
                                   d_ctu=g["d_ctu"].data_ptr() + 4 * a, d_rec=g["d_blocks"].data_ptr() + a * area * S))
                live.append((log2, g, a, b))
            best, st = intra_device(hv.h, S, self.bd, self.d_src.data_ptr(), self.stride, groups, self.d_states.data_ptr(), self.quant, self.rsl, self.lam, 1.0 / self.lam)
            self.launches += st.launches + 2 * len(live)
            for log2, g, a, b in live:
                g["best"][a:b] = best[log2]
                with torch.cuda.stream(hv.tstream):
                    g["d_mode"][a:b].copy_(torch.from_numpy(np.ascontiguousarray(best[log2]["mode"])), non_blocking=False)
                hv.intra_commit_a(S, self.layout, self.d_rec.data_ptr(), self.d_modes.data_ptr(), g["d_parts"].data_ptr() + 16 * a, b - a,
                                  g["d_blocks"].data_ptr() + a * g["nn"] * g["nn"] * S, g["d_mode"].data_ptr() + 4 * a)
        hv.sync()

    def results(self):
        """(champions INTRA_RD_RESULT_DT [partitions] in CODING order, candModeList the device derived [partitions, 3], neighbour_modes, reconstruction plane)"""
        hv = self.hv
        best = np.zeros(len(self.parts), INTRA_RD_RESULT_DT)
        cand, nbm = np.zeros((len(self.parts), 3), np.int32), np.zeros(len(self.parts), np.int32)
        for g in self.sizes.values():
            best[g["sel"]] = g["best"]
            ic = hv.down(g["d_ictx"], np.int32).view(INTRA_CTX_DT)
            cand[g["sel"]], nbm[g["sel"]] = ic["cand_mode_list"], ic["neighbour_modes"]
        return best, cand, nbm, hv.down(self.d_rec, self.dt)


def rqt_units(width, height, ctus_x):
    """the inter units whose transform trees are decided: 32x32 units where they fit, 16x16 then 8x8 units along a partial last row / column"""
    rows = []
    for size, log2 in ((32, 5), (16, 4), (8, 3)):
        for y in range(0, height - size + 1, size):
            for x in range(0, width - size + 1, size):
                # a unit is emitted at the largest size that fits its position on the grid of that size and lies outside the area covered by larger units
                big = size * 2
                covered = size < 32 and x // big * big + big <= width and y // big * big + big <= height
                if not covered:
                    rows.append((x, y, log2, (y // 64) * ctus_x + x // 64))
    return np.array(rows, np.int32).reshape(-1, 4).view(RQT_CU_DT).reshape(-1)


class Stage(typing.NamedTuple):
    """one stage of DecisionPicture's step behind the transform trees and the loop filter, inside the replayed sequence"""
    option: str              # the constructor option that enables it (on unless False / None); the picture keeps it as an attribute of the same name
    launch: str              # the method that issues its launches
    requires: tuple          # ((violated(o), message), ...) over the constructor's options o, in the order they are checked
    banded: str = None       # why step_banded refuses it (None: what it requires is refused already)
    extra: str = None        # results(): the getter of what it decided (None: it has a results method of its own)


def _off_device(o):
    return not o["search_on_device"]


def _no_8_grid(o):
    return bool(o["width"] % 8 or o["height"] % 8)


def _merge_lists_count(o):
    m = o["merge_lists"]
    return isinstance(m, bool) or int(m) != m or not 1 <= int(m) <= 5


def _merge_lists_targets(o):
    col = o["col"]
    return col is not None and "target_poc" in col and tuple(int(v) for v in col["target_poc"]) != tuple(int(v) for v in tuple(o["motion"])[1:3])


# in step()'s order: every stage reads in place what the stages before it left on the device
STAGES = (
    # (the tables its launches read went up before the replay: pu_candidates)
    Stage("pu_modes", "pu_mode_launches", ((_off_device, "pu_modes=True needs the device route (search_on_device=True)"),),
          banded="step_banded does not decide the prediction units' modes: use step() with pu_modes=True", extra="pu_decisions"),
    # (behind pu_decide: it reads the winners in place; before cu_close, which reads its records)
    Stage("unit_trees", "unit_tree_launches",
          ((_off_device, "unit_trees=True needs the device route (search_on_device=True)"),
           (lambda o: not (o["tree_rates"] and o["pu_modes"] and o["cu_close"]),
            "unit_trees=True gives every searched unit the tree of its winning prediction and closes it: it needs tree_rates=True, pu_modes=True and cu_close=True"),
           (_no_8_grid, "unit_trees=True needs a width and a height that are multiples of 8 (the unit prediction planes are addressed in 8-byte pieces)")),
          banded="step_banded does not build the searched units' trees: use step() with unit_trees=True", extra="unit_tree_decisions"),
    # (after the tree decisions AND the prediction units' rates: it reads both in place)
    Stage("cu_close", "cu_close_launches",
          ((_off_device, "cu_close=True needs the device route (search_on_device=True)"),
           (lambda o: not (o["tree_rates"] and o["pu_modes"]),
            "cu_close=True closes a unit over its tree's and its prediction unit's CABAC bits: it needs tree_rates=True and pu_modes=True")),
          banded="step_banded does not close coding units: use step() with cu_close=True", extra="cu_decisions"),
    # (behind cu_close: it reads its records in place)
    Stage("cqt", "cqt_launch",
          ((_off_device, "cqt=True needs the device route (search_on_device=True)"),
           (lambda o: not o["cu_close"], "cqt=True decides the coding quadtree over closed coding units: it needs cu_close=True"),
           (_no_8_grid, "cqt=True needs a width and a height that are multiples of the minimum coding block size, 8")),
          banded="step_banded does not decide coding quadtrees: use step() with cqt=True", extra="cqt_decisions"),
    # (directly behind the quadtree: it acts on its records, into buffers of its own)
    Stage("commit", "cqt_commit_launch",
          ((lambda o: not (o["unit_trees"] and o["cqt"]),
            "commit=True commits the quadtree decided over the searched units into one picture: it needs unit_trees=True and cqt=True"),)),
    # (directly behind the commit: it reads the cells that wrote, nothing else)
    Stage("motion", "cqt_motion_launch",
          ((lambda o: not o["commit"], "motion=(poc, ref_poc0, ref_poc1) makes the collocated motion store of the committed picture: it needs commit=True"),)),
    # (behind the commit: it filters and pads what that wrote, in place)
    Stage("finish", "cqt_finish_launch", ((lambda o: not o["commit"], "finish=True deblocks and pads the committed picture: it needs commit=True"),)),
    # (reads another picture's store and this picture's unit table only; with temporal_mvp step() issues it BEFORE the searches instead, outside the replay)
    Stage("col", "temporal_launch", ((_off_device, "col= needs the device route (search_on_device=True)"),),
          banded="step_banded does not derive temporal candidates: use step() with col="),
    # (behind the commit, whose cells it reads, and the temporal candidates)
    Stage("merge_lists", "cqt_merge_launch",
          ((lambda o: not o["commit"] or o["motion"] is None,
            "merge_lists=max_cand derives the committed picture's merge candidate lists: it needs commit=True and motion=(poc, ref_poc0, ref_poc1)"),
           (_merge_lists_count, "merge_lists must be the number of merge candidates, 1..5"),
           (_merge_lists_targets, "merge_lists: col['target_poc'] differs from motion's two references (the temporal candidates were scaled towards other pictures)"))),
)
# the options that change the step's route without being a stage of their own
ROUTE_REQUIRES = {
    "temporal_mvp": ((lambda o: o["col"] is None, "temporal_mvp=True feeds the temporal candidates of col= into the search walk's predictors: it needs col="),),
    "sao": ((_off_device, "sao=True needs the device route (search_on_device=True)"),),
    "residual_rates": ((_off_device, "residual_rates=True needs the device route (search_on_device=True)"),),
    "tree_rates": ((_off_device, "tree_rates=True needs the device route (search_on_device=True)"),
                   (lambda o: o["residual_rates"], "tree_rates=True prices the whole transform tree, residuals included: not together with residual_rates=True"),
                   (lambda o: o["sao"], "tree_rates=True together with sao=True is not built")),
}
# the order the constructor has always made its refusals in: a caller with two mistakes sees the same one
CHECK_ORDER = ("merge_lists", "motion", "col", "temporal_mvp", "finish", "commit", "unit_trees", "cqt", "cu_close", "pu_modes", "sao", "residual_rates", "tree_rates")


def _on(option, value):
    """motion=, col= and merge_lists= carry a value (on unless None); every other option is a flag"""
    return value is not None if option in ("motion", "col", "merge_lists") else bool(value)


class DecisionPicture:
    """One inter picture through the DECISION-DRIVEN path on the device (bench.py --decisions, tests/test_decisions.py):

      1. the 15 fractional-sample planes of both reference pictures (havoc_mi355x_interp_planes);
      2. every PU's uni-directional search in both lists, CTUs in wavefront order, predictors derived from the vectors decided before, then the
         bi-directional refinement of every PU (searchBi) -- the decision loops run inside the kernel (libhavoc_search.so:
         havoc_search_picture_uni_device -> csrc/kernels_search.hip; search_on_device=False: launch + host replay rounds, no bi refinement);
      3. the TU side ON THE CHOSEN VECTORS: HavocPredUni of every 16x16 block (8x8 in a last partial row) at the list-0 vector the
         search left for it, then the residual-quadtree decision of every inter unit (32x32 units, smaller along partial edges;
         libhavoc_search.so: havoc_search_rqt): both tree depths of every unit through residual + forward DCT -> Rdoq::runQuantisation ->
         de-quantise + inverse DCT + add -> SSD in one chain per transform size, the decisions taken from 16 bytes per candidate, the chosen
         candidates reconstructed into the picture (job tables are built from the decided motion field: they cannot exist before 2).

      4. the intra candidates an inter picture evaluates (21.4 k partitions per 1080p frame): per partition size the 35-mode
         prediction + SATD stage and its refinement order (havoc_search_intra_modes), then every candidate mode reconstructed and the champion
         picked (havoc_search_intra_rd) -- with neighbours from the SOURCE picture, i.e. without the chain through the previous partition's
         reconstruction that the encoder has (stated; that chain needs a device-side loop).

    What is NOT in it (stated, not hidden): the encoder's mode decision between the searched PUs (every PU of workload.picture_pus is
    searched and the last one covering an area stands) and between inter and intra, bi-prediction, CABAC.  `step()` is what bench.py times.

    How it is put together: the formats of the transform chains -- RDOQ job records, where a unit's candidates lie, tree-rate jobs -- are tu_plan.py's; _chain_group
    gives a job table its buffers, _chain / _chain_final issue a chain over groups, _tree_tables builds rqt_plan (self.units) and unit_plan (self.pus) alike.  The stages
    behind the trees (pu_modes ... merge_lists) are the rows of STAGES: the constructor's refusals, step()'s sequence, step_banded's refusals and results()' extras
    are read from it -- a new stage is one row and its own methods.  What the getters download is kept in one cache until the next step (_forget).

    pu_modes=True (device route only) adds the decision WITHIN every searched prediction unit that go2 takes (turing/Search.hpp:1844-1902): its uni L0, uni L1 and
    bi candidates -- the search's own records: the two uni-directional results and the two bi-directional refinements, list l's refined record holding what
    searchMotionBi leaves in codedPu for list l -- predicted in three planes, measured with the SATD against the source, priced with the reference's CABAC bits
    (havoc_mi355x_pu_rate) from one 16-byte snapshot per CTU and compared (havoc_mi355x_pu_decide), inside the replayed graph; `pu_decisions` has the outcome.  The
    workload's units are 2Nx2N of 64 to 8, so go2 tries no merge candidate and every unit may be bi.  Still out: writing the winner's prediction into `pred` / `cpred`
    (overlapping searched units make that a coding-unit decision: predict() keeps the list-0 vector), the merge candidates of searchMerge2Nx2N, contexts carried from
    unit to unit, the coding-unit bits, and the search walk's predictors taking decided modes."""

    PAD = 96

    def __init__(self, hv, width, height, bit_depth=8, qp=32, seed=11, threads=16, frames=None, density=1.0, intra=True, search_on_device=True, distance=1,
                 sao=False, residual_rates=False, tree_rates=False, pu_modes=False, cu_close=False, cqt=False, unit_trees=False, commit=False, finish=False,
                 motion=None, col=None, temporal_mvp=False, merge_lists=None):
        """merge_lists=max_cand (1..5; needs commit=True and motion=, whose two references are the lists' picture order counts): the merge candidate list of every
        final coding unit of the committed picture and the lowest merge index that carries the unit's committed motion, into `cqt_merge` (havoc.MERGE_LIST_DT per
        searched unit; havoc_mi355x_cqt_merge_lists, behind the commit -- and behind the temporal candidates -- inside the replayed graph; cqt_merge_results()).  With
        col= the lists take that option's temporal records (col["target_poc"] must be motion's two references); without col= they have no temporal candidate.
        motion=(poc, ref_poc0, ref_poc1) (needs commit=True): the committed picture also leaves its collocated motion store in `cqt_store`
        (havoc_mi355x_cqt_motion_store, directly behind the commit inside the replayed graph; cqt_motion_results()) -- with finish=True the two things a reference
        picture is.
        col=dict(store=<device tensor of havoc.COL_CELL_DT records, dense rows: another picture's cqt_store>, col_poc=, cur_poc=, target_poc=(l0, l1), all_backwards=,
        collocated_from_l0=) (device search route only): the temporal candidate of every unit of self.pus per list from that store
        (havoc_mi355x_temporal_candidates, inside the replayed graph; temporal_candidates()).  The store belongs to ANOTHER picture: that the step which writes it
        has finished (or is ordered before this picture's step on the same stream) is the caller's to establish, and the tensor must stay alive and in place --
        the recorded graph holds its address.  With col= alone the candidates are produced, not consumed: the search walk's predictors do not read them.
        temporal_mvp=True (needs col=; not step_banded): the search walk's predictor derivation consumes them (havoc_mi355x_search_temporal; picture_order.hpp:
        derivePredictors).  step() then issues temporal_launch() BEFORE the searches, on the context's stream and outside the replayed graph (not again inside it), sets
        the table on the context for the search and removes it afterwards -- also when the search raises; temporal_candidates() returns the records as before.  What
        follows the searches (pu_candidates, pu_rate, cu_close, cqt, the commit, the motion store) reads their results in place and needs nothing of its own."""
        import torch
        o = dict(width=width, height=height, search_on_device=search_on_device, sao=sao, residual_rates=residual_rates, tree_rates=tree_rates, pu_modes=pu_modes,
                 cu_close=cu_close, cqt=cqt, unit_trees=unit_trees, commit=commit, finish=finish, motion=motion, col=col, temporal_mvp=temporal_mvp,
                 merge_lists=merge_lists)
        requires = dict(ROUTE_REQUIRES, **{s.option: s.requires for s in STAGES})
        for option in CHECK_ORDER:
            if _on(option, o[option]):
                for violated, message in requires[option]:
                    if violated(o):
                        raise ValueError(message)
        # the transform-tree decision prices each candidate's residual with the reference's CABAC bits (havoc_mi355x_residual_rate) in place of the stand-in
        self.residual_rates = residual_rates
        # ... or compares what the reference compares: the whole transform_tree's bits of both depths (havoc_mi355x_tree_rate) and the distortion of three planes
        # (havoc_mi355x_rqt_decide_tree), luma AND chroma reconstructed at the decided depth
        self.tree_rates = tree_rates
        # every searched prediction unit's inter mode (L0 / L1 / bi) by the reference's CABAC bits and three-plane SATDs (havoc_mi355x_pu_rate / _pu_decide)
        self.pu_modes = pu_modes
        # every transform-tree unit closed as the reference closes an inter coding unit: the CU's own bits and the residual / no-residual decision (havoc_mi355x_cu_close)
        self.cu_close = cu_close
        # every CTU's coding quadtree decided over those closed units: split_cu_flag's bits and the full / split comparison, CTU after CTU (havoc_mi355x_cqt_decide)
        self.cqt = cqt
        # the tree, close and quadtree stages run over the SEARCHED units (self.pus), each with the transform tree of its own winning prediction (unit_pred_select,
        # a second tree plan, rqt_decide_units); the legacy plan over self.units still makes recon / crecon / cells, untouched
        self.unit_trees = unit_trees
        # the decided quadtree acted on: its final units' samples into cqt_recon / cqt_crecon and one record per 8x8 cell into cqt_cells (havoc_mi355x_cqt_commit);
        # recon / crecon / cells stay the legacy plan's
        self.commit = commit
        # ... and finished as TaskDeblock.cpp:105-167 finishes a picture before it is used for prediction: the committed cells as 4x4 cells (havoc_mi355x_cqt_block_cells),
        # boundary strengths, deblocking of cqt_recon / cqt_crecon in place, padding of the three planes
        self.finish = finish
        # ... and its motion as the store the next picture's temporal candidate is derived from (havoc_mi355x_cqt_motion_store): (poc, ref_poc0, ref_poc1) or None
        self.motion = None if motion is None else tuple(int(v) for v in motion)
        # this picture's own temporal candidates from ANOTHER picture's store (havoc_mi355x_temporal_candidates): the caller's dict or None
        self.col = None if col is None else dict(col)
        self.temporal_mvp = bool(temporal_mvp)      # ... consumed by the search walk's predictor derivation (havoc_mi355x_search_temporal)
        # the committed picture's merge candidate lists (havoc_mi355x_cqt_merge_lists): MaxNumMergeCand or None
        self.merge_lists = None if merge_lists is None else int(merge_lists)
        self.sao = sao                               # in-loop SAO between deblocking and padding (sao_filter_inputs / sao_loop_filter)
        from . import havoc as hmod
        from . import workload
        self.hv, self.torch, self.hmod = hv, torch, hmod
        self.W, self.H, self.bd, self.qp, self.threads = width, height, bit_depth, qp, threads
        self.search_on_device = search_on_device      # the decision loops inside the kernel (kernels_search.hip) / launch + host replay rounds
        self.use_graphs, self._graphs = True, {}
        self.S = 1 if bit_depth == 8 else 2
        self.dt = np.uint8 if self.S == 1 else np.uint16
        d = decision_inputs(width, height, bit_depth, qp, seed, density, frames, distance)
        self.stride = d["stride"]
        self.host_planes = d["planes"]                            # source, list 0, list 1
        self.n = self.host_planes[0].size
        self.pe = (self.n + 63) & ~63
        self.origin = self.PAD * self.stride + self.PAD
        pic = np.zeros(3 * self.pe, self.dt)
        for k, p in enumerate(self.host_planes):
            pic[k * self.pe:k * self.pe + self.n] = p
        self.d_pic = hv.up(pic)                                   # one allocation: a job names a plane by a 32-bit sample offset
        self.d_phase = hv.zeros(32 * self.pe, self.dt)            # 2 references x 16 phase planes
        self.pus, self.ctu_first, self.cx, self.cy = d["pus"], d["ctu_first"], d["cx"], d["cy"]
        lam = d["lam"]
        self.params, self.mvp_rate = d["params"], d["mvp_rate"]
        # ---- prediction: 16x16 blocks over the rows that hold whole ones, 8x8 blocks over a last partial row; the (older) fixed-size TU chain
        # over the same blocks stays available as tu_chain_fixed()
        self.units = rqt_units(width, height, self.cx)
        self.quant = rqt_quant(qp, bit_depth)
        self.lam = lam
        self.groups = []
        h16 = height // 16 * 16
        for log2, y_lo, y_hi in ((4, 0, h16), (3, h16, height // 8 * 8)):
            nn = 1 << log2
            if y_hi <= y_lo:
                continue
            xs, ys = np.meshgrid(np.arange(0, width // nn * nn, nn), np.arange(y_lo, y_hi, nn))
            x0, y0 = xs.ravel().astype(np.int64), ys.ravel().astype(np.int64)
            at = (y0 + self.PAD) * self.stride + x0 + self.PAD
            fj = np.stack([np.arange(len(x0)) * nn * nn, at, y0 * width + x0, at], 1).astype(np.int32)
            self.groups.append(dict(self._chain_group(log2, fj, (y0 // 64) * self.cx + x0 // 64), x0=x0, y0=y0, pj=np.zeros((len(x0), 8), np.int32),
                                    d_pj=hv.zeros(len(x0) * 8, np.int32)))
        self._cache = {}        # what the getters downloaded of the last step
        self.rdoq_states, self.d_states = self._ctu_snapshots(seed + 7919, 128)
        if tree_rates:      # the contexts outside the 128-byte snapshot (HAVOC_INTRA_SYNTAX_CTX_*: split_transform_flag's)
            self.syntax_states, self.d_syntax_states = self._ctu_snapshots(seed + 7927, 4)
        if pu_modes:        # prediction_unit()'s contexts (HAVOC_PU_SYNTAX_CTX_*)
            self.pu_syntax_states, self.d_pu_syntax_states = self._ctu_snapshots(seed + 7933, hmod.PU_SYNTAX_CTX_BYTES)
        if cu_close:        # coding_unit()'s contexts (HAVOC_CU_SYNTAX_CTX_*)
            self.cu_syntax_states, self.d_cu_syntax_states = self._ctu_snapshots(seed + 7937, hmod.CU_SYNTAX_CTX_BYTES)
        self.pred = hv.zeros(width * height, self.dt)
        self.recon = hv.zeros(self.pe, self.dt)
        # chroma (round 4): Cb / Cr of source, list 0, list 1 in ONE allocation (plane k at k * cpe: 0-2 Cb, 3-5 Cr), their prediction and reconstruction planes
        self.host_chroma, self.cstride = d["chroma"], d["cstride"]
        self.cn = self.host_chroma[0].size
        self.cpe = (self.cn + 63) & ~63
        self.corigin = (self.PAD // 2) * self.cstride + self.PAD // 2
        cpic = np.zeros(6 * self.cpe, self.dt)
        for k, p in enumerate(self.host_chroma):
            cpic[k * self.cpe:k * self.cpe + self.cn] = p
        self.d_cpic = hv.up(cpic)
        self.cpred = hv.zeros(2 * (width // 2) * (height // 2), self.dt)      # Cb then Cr, unpadded, stride width / 2
        # the decided motion field stays on the device (int16 [2 lists][cells][2]); the job tables of the steps after the searches are made from it THERE
        self.d_field = hv.zeros(2 * ((width + 3) // 4) * ((height + 3) // 4) * 2, np.int16)
        self.layout = hv.field_layout(width, height, self.stride, self.PAD, self.pe, self.cstride, self.PAD // 2, self.cpe)
        self.crecon = hv.zeros(2 * self.cpe, self.dt)
        if commit:          # the decided picture in buffers of its own, laid out as recon / crecon are; the cells: havoc.CQT_CELL_DT per MinCb cell
            self.cqt_recon, self.cqt_crecon = hv.zeros(self.pe, self.dt), hv.zeros(2 * self.cpe, self.dt)
            self.cqt_cells = hv.zeros((height >> self.CQT_MIN_CB_LOG2) * (width >> self.CQT_MIN_CB_LOG2) * hmod.CQT_CELL_DT.itemsize, np.uint8)
        if self.motion is not None:     # the decided picture's collocated motion store: havoc.COL_CELL_DT per 16x16 luma samples, dense rows
            if len(self.motion) != 3:
                raise ValueError("motion must be (poc, ref_poc0, ref_poc1)")
            self.cqt_store = hv.zeros(((height + 15) // 16) * ((width + 15) // 16) * hmod.COL_CELL_DT.itemsize, np.uint8)
        if self.col is not None:        # a record per (unit, list)
            missing = {"store", "col_poc", "cur_poc", "target_poc", "all_backwards", "collocated_from_l0"} ^ set(self.col)
            if missing:
                raise ValueError("col= takes exactly store, col_poc, cur_poc, target_poc, all_backwards, collocated_from_l0: %s" % sorted(missing))
            c = self.col
            self._temporal_params = hmod.temporal_params(width, height, self.CQT_CTB_LOG2, c["col_poc"], c["cur_poc"], c["target_poc"], c["all_backwards"],
                                                         c["collocated_from_l0"])
            self._d_temporal = hv.zeros(max(1, 2 * len(self.pus)) * hmod.TEMPORAL_CAND_DT.itemsize, np.uint8)
        if self.merge_lists is not None:    # a record per searched unit
            self._merge_params = hmod.merge_params(width, height, self.CQT_CTB_LOG2, self.CQT_MIN_CB_LOG2, self.merge_lists, self.motion[1:3])
            self.cqt_merge = hv.zeros(max(1, len(self.pus)) * hmod.MERGE_LIST_DT.itemsize, np.uint8)
        # ---- the intra candidates of the picture (an inter picture evaluates them per coding unit): partitions with neighbours from the source
        self.intra_parts = {}
        self.rsl = float(self.params.reciprocal_sqrt_lambda)
        if intra:
            src2d = self.host_planes[0].reshape(-1, self.stride)
            for log2, (jobs, nb, ictx, ctu) in workload.intra_partitions(src2d, width, height, self.PAD, seed + 31).items():
                self.intra_parts[log2] = dict(jobs=jobs, nb=nb, ictx=ictx, ctu=ctu, d_jobs=hv.up(jobs), d_nb=hv.up(nb),
                                              d_ictx=hv.up(np.ascontiguousarray(ictx).view(np.int32)), d_ctu=hv.up(np.ascontiguousarray(ctu, np.int32)),
                                              d_rec=hv.zeros(len(jobs) << (2 * log2), self.dt))
        self._filter_buffers()
        self._constructed = tuple(self.__dict__)      # (what a band view shares with its picture: _band_views)
        hv.sync()

    def _ctu_snapshots(self, seed, nbytes):
        """one snapshot of nbytes CABAC context states per CTU, seeded: a base state per context (drawn first), a jitter per CTU, limited to the valid states.
        Returns (uint8 [CTUs, nbytes], its device copy)"""
        rng = np.random.default_rng(seed)
        base = rng.integers(4, 100, nbytes)
        states = np.clip(base[None, :] + rng.integers(-6, 7, (self.cx * self.cy, nbytes)), 0, 125).astype(np.uint8)
        return states, self.hv.up(states.reshape(-1))

    def _up_records(self, records):
        """a table of records of any layout as a uint8 device tensor"""
        return self.hv.up(np.ascontiguousarray(records).view(np.uint8).reshape(-1))

    def _zeros64(self, n):
        with self.torch.cuda.stream(self.hv.tstream):
            return self.torch.zeros(n, dtype=self.torch.int64, device=self.hv.device)

    def _pus_table(self):
        """self.pus on the device, laid out as the search's own copy of it is; it goes up once, for every launch that reads it"""
        if not hasattr(self, "_d_pus"):
            self._d_pus = self._up_records(self.pus)
        return self._d_pus

    # ---- the transform chain: residual + forward transform -> Rdoq::runQuantisation -> de-quantise + inverse transform + add -> SSD, over GROUPS of blocks of one size.
    # A group's job table (int32 [m, 4]) names per block its slot in the group's buffers and its source, prediction and reconstruction blocks by sample offsets
    # (tu_plan.py has the formats) ---------------------------------------------------------------------------------------------------------------------------------
    def _chain_group(self, log2, jobs, ctx_index, c_idx=0, pieces=False, final=False, stats=False, rates=False):
        """the RDOQ records and the buffers of the group of 2^log2 blocks that `jobs` names.  pieces: a buffer of reconstructed blocks, slot by slot (for candidates,
        which are compared before one of them goes into the picture); final: the job records the decision writes for the last reconstruction, and its SSDs; stats:
        the level statistics of the stand-in rate; rates: a CABAC rate per block"""
        hv, m, area = self.hv, len(jobs), 1 << 2 * log2
        rj, inv, dshift = tu_plan.rdoq_jobs(self.qp, self.bd, self.lam, log2, jobs[:, 0], ctx_index, c_idx)
        g = dict(log2=log2, nn=1 << log2, m=m, inv=inv, dshift=dshift, jobs=jobs, d_jobs=hv.up(jobs), d_rj=self._up_records(rj), coef=hv.zeros(m * area, np.int16),
                 level=hv.zeros(m * area, np.int16), cbf=hv.zeros(m, np.int32), ssd=hv.zeros(m, np.uint32), work=hv.rdoq_workspace(m))
        if pieces:
            g["piece"] = hv.zeros(m * area, self.dt)
        if final:
            g["d_fin"], g["ssd2"] = hv.zeros(m * 4, np.int32).view(-1, 4), hv.zeros(m, np.uint32)
        if stats:
            g["d_sj"], g["stats"] = hv.up(np.stack([jobs[:, 0], np.full(m, area)], 1).astype(np.int32)), hv.zeros(2 * m, np.int32)
        if rates:
            g["rates"] = self._zeros64(m)
        return g

    def _chain(self, groups, src, src_stride, pred, pred_stride, dst=None, dst_stride=None, then=None):
        """the chain of every group: blocks of the planes src and pred, reconstructed into the plane dst -- or, without one, into the group's pieces; then(g)
        (optional) issues what follows a group's three launches.  Asynchronous"""
        hv, bd = self.hv, self.bd
        for g in groups:
            rec, rec_stride = (g["piece"], g["nn"]) if dst is None else (dst, dst_stride)
            hv.tu_forward_d(bd, 0, g["log2"], g["coef"], src, src_stride, pred, pred_stride, g["d_jobs"])
            hv.rdoq_d(bd, g["log2"], g["level"], g["coef"], self.d_states, g["d_rj"], g["cbf"], g["work"])
            hv.tu_reconstruct_d(bd, 0, g["log2"], g["inv"], g["dshift"], rec, rec_stride, pred, pred_stride, src, src_stride, g["level"], g["d_jobs"], g["ssd"])
            if then is not None:
                then(g)

    def _chain_final(self, groups, src, src_stride, pred, pred_stride, dst, dst_stride):
        """every candidate reconstructed once more from its levels by the records the decision wrote (final=True): the chosen ones into the plane dst, the others
        into the dump block"""
        for g in groups:
            self.hv.tu_reconstruct_d(self.bd, 0, g["log2"], g["inv"], g["dshift"], dst, dst_stride, pred, pred_stride, src, src_stride, g["level"], g["d_fin"], g["ssd2"])

    def _tree_rates(self, plan):
        """the whole-tree rate and cbf mask per (unit size, depth) of a tree plan, from the levels its chains left"""
        for (L, depth), t in plan["tree_jobs"].items():
            self.hv.tree_rate_d(L, depth, plan["sizes"][t["luma"]]["level"], plan["csizes"][t["chroma"]]["level"], self.d_states, self.d_syntax_states, t["d_jobs"],
                                plan["tree_rate"], plan["tree_cbf"])

    def phase_planes(self):
        hv, pe, S = self.hv, self.pe, self.S
        for r in (0, 1):
            ph = self.d_phase[r * 16 * pe:(r + 1) * 16 * pe]
            ref = self.d_pic[(1 + r) * pe:(2 + r) * pe]
            with self.torch.cuda.stream(hv.tstream):
                ph[:pe] = ref                                   # phase 0 = the picture itself
            hv.interp_planes_d(self.bd, ph, pe, ref, self.stride, 12, 4, self.W + 2 * self.PAD - 24, self.H + 2 * self.PAD - 8)

    def search(self):
        hv, pe, o = self.hv, self.pe, self.origin
        base, ph = self.d_pic.data_ptr(), self.d_phase.data_ptr()
        r = picture_uni(hv.h, self.S, self.params, base, o, self.stride, base, (pe + o, 2 * pe + o), self.stride, self.PAD, ph, pe, (o, 16 * pe + o),
                        self.pus, self.ctu_first, self.cx, self.cy, self.mvp_rate, self.threads, on_device=self.search_on_device, bi=self.search_on_device,
                        d_field_keep=self.d_field.data_ptr() if self.search_on_device else None)
        self.bi_results = r[3] if self.search_on_device else None      # the bi-directional refinements (device search only)
        if not self.search_on_device:                                  # the host-replay search decides on the host: its field goes down once
            with self.torch.cuda.stream(hv.tstream):
                self.d_field.copy_(self.torch.from_numpy(r[1].reshape(-1)), non_blocking=False)
        return r[:3]

    def predict(self, field):
        """HavocPredUni of every inter unit (a 2Nx2N prediction unit per unit of rqt_units) at the list-0 vector decided at its origin, into the
        prediction plane; asynchronous"""
        hv, bd = self.hv, self.bd
        if not hasattr(self, "pgroups"):
            self.pgroups = []
            for log2 in (5, 4, 3):
                sel = np.flatnonzero(self.units["log2_size"] == log2)
                if len(sel):
                    x0, y0 = self.units["x0"][sel].astype(np.int32), self.units["y0"][sel].astype(np.int32)
                    self.pgroups.append(dict(log2=log2, nn=1 << log2, d_x0=hv.up(x0), d_y0=hv.up(y0), d_dst=hv.up(y0 * self.W + x0), d_pj=hv.zeros(len(sel) * 8, np.int32)))
        for g in self.pgroups:
            # the job table from the field, on the device (k_pred_jobs): reference offsets count from the start of the luma allocation
            hv.pred_jobs_d(self.layout, self.d_field, 0, g["d_x0"], g["d_y0"], g["log2"], 0, g["d_dst"], g["d_pj"])
            hv.pred_uni_d(8, bd, self.pred, self.W, self.d_pic, self.stride, g["d_pj"].view(-1, 8), g["nn"], g["nn"])

    # ---- round 4: the merge candidates of every unit and the chroma planes -------------------------------------------------
    MERGE_CANDIDATES = 5

    def merge_vectors(self, field):
        """the candidate vectors of every unit of self.units: both lists' vectors decided for the cells at the five spatial merge positions (HEVC 8.5.3.2.3:
        A1 left-bottom, B1 above-right, B0, A0, B2 -- Mvp.h's derivation with its pruning and temporal candidate stays out of scope: the vectors are INPUTS);
        a position outside the picture gives zero vectors; every vector is limited so that the block and its filter taps stay inside the padded planes
        (as LimitFullPelMv does for the searches).  int16 [units, 5, 2 lists, 2]"""
        u = self.units
        n = 1 << u["log2_size"].astype(np.int64)
        x0, y0 = u["x0"].astype(np.int64), u["y0"].astype(np.int64)
        px = np.stack([x0 - 1, x0 + n - 1, x0 + n, x0 - 1, x0 - 1], 1)
        py = np.stack([y0 + n - 1, y0 - 1, y0 - 1, y0 + n, y0 - 1], 1)
        inside = (px >= 0) & (py >= 0) & (px < self.W) & (py < self.H)
        cx, cy = np.clip(px, 0, self.W - 1) >> 2, np.clip(py, 0, self.H - 1) >> 2
        mv = np.stack([field[0, cy, cx], field[1, cy, cx]], 2).astype(np.int64)      # [units, 5, list, xy]
        mv *= inside[:, :, None, None]
        lo_x, hi_x = (-64 - x0) * 4, (self.W + 64 - x0 - n) * 4
        lo_y, hi_y = (-64 - y0) * 4, (self.H + 64 - y0 - n) * 4
        mv[..., 0] = np.clip(mv[..., 0], lo_x[:, None, None], hi_x[:, None, None])
        mv[..., 1] = np.clip(mv[..., 1], lo_y[:, None, None], hi_y[:, None, None])
        return mv.astype(np.int16)

    def merge_candidates(self, field):
        """searchMergeModes / measurePuCost (turing/Search.hpp:1659-1706, 1754-1768) as batches: every unit's five candidates predicted bi-directionally in all
        three planes (HavocPredBi 8-tap luma, 4-tap Cb / Cr) and measured with the Hadamard SATD against the source (Measure.h:97-168: chroma only where the
        halved unit is a multiple of 4), cost = rate + (satdY + satdCb + satdCr) * reciprocalSqrtLambda with a stand-in rate of the merge index (i + 1 bits,
        4 at most).  Leaves self.merge = dict(vectors, satd [units, 5, 3], cost [units, 5] Q16, best [units]).  9 launches per unit size."""
        hv, bd, torch = self.hv, self.bd, self.torch
        u, K = self.units, self.MERGE_CANDIDATES
        if not hasattr(self, "mgroups"):
            # everything that does not depend on the vectors is made once: the units' positions, destination slots, the source blocks' SATD jobs
            self.mgroups, at = [], 0
            for log2 in (5, 4, 3):
                sel = np.flatnonzero(u["log2_size"] == log2)
                if not len(sel):
                    continue
                nn, m = 1 << log2, len(sel) * K
                x0, y0 = np.repeat(u["x0"][sel].astype(np.int64), K), np.repeat(u["y0"][sel].astype(np.int64), K)
                g = dict(log2=log2, nn=nn, sel=sel, m=m, planes=[], d_x0=hv.up(u["x0"][sel].astype(np.int32)), d_y0=hv.up(u["y0"][sel].astype(np.int32)),
                         d_vec=hv.zeros(m * 4, np.int16), d_cost=torch.zeros(m, dtype=torch.int64, device=hv.device), d_best=hv.zeros(len(sel), np.int32))
                for plane in range(3):
                    c = plane > 0
                    size, stride, pad, pe = (nn // 2, self.cstride, self.PAD // 2, self.cpe) if c else (nn, self.stride, self.PAD, self.pe)
                    bx, by = (x0 // 2, y0 // 2) if c else (x0, y0)
                    first = (3 * (plane - 1)) if c else 0                # plane index of the source inside the allocation (Cb: 0, Cr: 3; luma: 0)
                    dst = np.arange(m) * size * size
                    sj = np.stack([first * pe + (by + pad) * stride + bx + pad, dst, np.full(m, size), np.full(m, size)], 1).astype(np.int32)
                    g["planes"].append(dict(size=size, stride=stride, taps=4 if c else 8, d_bj=hv.zeros(m * 12, np.int32), d_sj=hv.up(sj),
                                            d_dst=hv.zeros(m * size * size, self.dt), at=at))
                    at += m
                self.mgroups.append(g)
            self.d_merge_satd = hv.zeros(at, np.int32)      # every SATD of the step in one buffer
        lam_q16 = int(float(self.params.reciprocal_sqrt_lambda) * 65536 + 0.5)
        for g in self.mgroups:
            q = g["planes"]
            hv.merge_jobs_d(self.layout, self.d_field, g["d_x0"], g["d_y0"], g["log2"], q[0]["d_bj"], q[1]["d_bj"], q[2]["d_bj"], g["d_vec"])
            for plane, p in enumerate(q):
                ref = self.d_cpic if plane else self.d_pic
                hv.pred_bi_d(p["taps"], bd, p["d_dst"], p["size"], ref, p["stride"], p["d_bj"].view(-1, 12), p["size"], p["size"])
                hv.satd_d(ref, p["stride"], p["d_dst"], p["size"], p["d_sj"], self.d_merge_satd[p["at"]:p["at"] + g["m"]], p["size"], p["size"])
            sat = [self.d_merge_satd[p["at"]:p["at"] + g["m"]] for p in q]
            hv.merge_decide_d(sat[0], sat[1], sat[2], len(g["sel"]), lam_q16, g["d_cost"], g["d_best"])

    @property
    def merge(self):
        """what merge_candidates() left on the device, as numpy: dict(vectors int16 [units, 5, 2 lists, 2], satd [units, 5, 3 planes], cost [units, 5] (Q16),
        best [units])"""
        if "merge" not in self._cache:
            hv, u, K = self.hv, self.units, self.MERGE_CANDIDATES
            flat = hv.down(self.d_merge_satd, np.int32)
            vec, satd = np.zeros((len(u), K, 2, 2), np.int16), np.zeros((len(u), K, 3), np.int64)
            cost, best = np.zeros((len(u), K), np.int64), np.zeros(len(u), np.int32)
            for g in self.mgroups:
                for plane, p in enumerate(g["planes"]):
                    satd[g["sel"], :, plane] = flat[p["at"]:p["at"] + g["m"]].reshape(-1, K)
                vec[g["sel"]] = hv.down(g["d_vec"], np.int16).reshape(-1, K, 2, 2)
                with self.torch.cuda.stream(hv.tstream):
                    cost[g["sel"]] = g["d_cost"].cpu().numpy().reshape(-1, K)
                best[g["sel"]] = hv.down(g["d_best"], np.int32)
            self._cache["merge"] = dict(vectors=vec, satd=satd, cost=cost, best=best)
        return self._cache["merge"]

    # ---- the inter mode of every searched prediction unit (go2, turing/Search.hpp:1844-1902) ---------------------------------------------------------
    PU_CANDIDATES = 3       # L0, L1, bi: the order go2 tries them in for a 2Nx2N unit

    def _pu_plan(self):
        """pu_modes' job tables and buffers, built once.  The units of one size form a group (a prediction block is then a contiguous size x size block of its
        group's buffer); candidate 3 i + k of the group's i-th unit (k: 0 L0, 1 L1, 2 bi) has the global index at + 3 i + k, which names its rate, SATDs, cost and
        snapshot; unit p's candidates start at first[p]."""
        if hasattr(self, "pu_plan"):
            return self.pu_plan
        hv, torch, hmod, K = self.hv, self.torch, self.hmod, self.PU_CANDIDATES
        pus, n = self.pus, len(self.pus)
        if not ((pus["w"] == pus["h"]) & (pus["part_2Nx2N"] == 1) & (pus["w"] >= 8)).all():
            raise ValueError("pu_modes=True handles 2Nx2N units of 64 to 8 (no merge candidate in go2, bi allowed)")
        M = K * n
        first, groups, at, cand_y, cand_c = np.zeros(n, np.int32), [], 0, 0, 0
        for log2 in (6, 5, 4, 3):
            sel = np.flatnonzero(pus["w"] == 1 << log2)
            if not len(sel):
                continue
            nn, m = 1 << log2, K * len(sel)
            first[sel] = at + K * np.arange(len(sel))
            x0, y0 = pus["x0"][sel].astype(np.int64), pus["y0"][sel].astype(np.int64)
            g = dict(log2=log2, nn=nn, sel=sel, m=m, at=at, x0=x0, y0=y0, planes=[])
            # where the group's prediction blocks lie in the picture's two candidate allocations (samples): luma; Cb, then Cr
            base = (cand_y, cand_c, cand_c + m * (nn // 2) ** 2)
            cand_y, cand_c = cand_y + m * nn * nn, cand_c + 2 * m * (nn // 2) ** 2
            for plane in range(3):
                c = plane > 0
                size, stride, pad, pe = (nn // 2, self.cstride, self.PAD // 2, self.cpe) if c else (nn, self.stride, self.PAD, self.pe)
                bx, by = (x0 // 2, y0 // 2) if c else (x0, y0)
                src = (3 * (plane - 1)) if c else 0                   # plane index of the source inside the allocation (Cb: 0, Cr: 3; luma: 0)
                here = (by + pad) * stride + bx + pad
                dst = np.arange(m) * size * size
                sj = np.stack([src * pe + np.repeat(here, K), dst, np.full(m, size), np.full(m, size)], 1).astype(np.int32)
                g["planes"].append(dict(size=size, stride=stride, taps=4 if c else 8, shift=3 if c else 2, here=here, first_ref=src + 1, pe=pe,
                                        d_uj=hv.zeros(2 * len(sel) * 8, np.int32), d_bj=hv.zeros(len(sel) * 12, np.int32), d_sj=hv.up(sj), base=base[plane]))
            groups.append(g)
            at += m
        # every group's blocks in ONE luma and ONE chroma allocation (a job of havoc_mi355x_unit_pred_select names a block by an offset from one base); a group's
        # buffer is a view of it: groups run from the largest size down, so every block stays aligned to its own size
        d_cand_y, d_cand_c = hv.zeros(max(cand_y, 1), self.dt), hv.zeros(max(cand_c, 1), self.dt)
        for g in groups:
            for plane, q in enumerate(g["planes"]):
                q["d_dst"] = (d_cand_c if plane else d_cand_y)[q["base"]:q["base"] + g["m"] * q["size"] ** 2]
        jobs = np.zeros(M, hmod.PU_RATE_JOB_DT)
        ctu = ((pus["y0"] // 64) * self.cx + pus["x0"] // 64).astype(np.int32)
        for k in range(K):
            at_k = first + k
            jobs["ctx_index"][at_k], jobs["pred"][at_k] = ctu, k
            jobs["w"][at_k], jobs["h"][at_k], jobs["cqt_depth"][at_k] = pus["w"], pus["h"], pus["cqt_depth"]
        jobs["out_index"] = np.arange(M)
        with torch.cuda.stream(hv.tstream):
            i64 = lambda count: torch.zeros(count, dtype=torch.int64, device=hv.device)
            self.pu_plan = dict(groups=groups, first=first, jobs=jobs, M=M, d_cand_y=d_cand_y, d_cand_c=d_cand_c, d_first=hv.up(first), d_count=hv.up(np.full(n, K, np.int32)),
                                d_jobs=torch.zeros(M * hmod.PU_RATE_JOB_DT.itemsize, dtype=torch.uint8, device=hv.device), d_satd=hv.zeros(3 * M, np.int32),
                                d_rate=i64(M), d_cost=i64(M), d_best=hv.zeros(n, np.int32), d_best_cost=i64(n),
                                d_after=hv.zeros(M * hmod.PU_SYNTAX_CTX_BYTES, np.uint8), d_best_syntax=hv.zeros(n * hmod.PU_SYNTAX_CTX_BYTES, np.uint8),
                                slice=hmod.PuSlice(slice_b=1, max_num_merge_cand=5, mvd_l1_zero_flag=0, num_ref_idx_active_minus1=(0, 0)))
        return self.pu_plan

    def pu_candidates(self, res):
        """the candidate and job tables of pu_modes from the search's records, on the host (they arrive there when search() returns), uploaded into the persistent
        buffers the replayed launches read: res[2 p + l] the uni-directional result of unit p in list l, self.bi_results[2 p + l] list l's bi-directional refinement.
        L0 / L1: mv, mvd, mvp_flag of the uni record; bi: list l's mv, mvd, mvp_flag of list l's refined record (what searchMotionBi leaves in codedPu,
        turing/Search.hpp:1651-1652, 1817-1822).  refIdx is 0 (Search.hpp:1883-1884)."""
        P, torch, hv = self._pu_plan(), self.torch, self.hv
        n, bi = len(self.pus), self.bi_results
        uni_mv = res["mv"].reshape(n, 2, 2).astype(np.int64)
        bi_mv = bi["mv"].reshape(n, 2, 2).astype(np.int64)
        jobs, first = P["jobs"], P["first"]
        for l in (0, 1):
            jobs["mvd"][first + l] = 0
            jobs["mvd"][first + l, l] = res["mvd"][l::2]
            jobs["mvp_flag"][first + l] = 0
            jobs["mvp_flag"][first + l, l] = res["mvp_flag"][l::2]
            jobs["mvd"][first + 2, l] = bi["mvd"][l::2]
            jobs["mvp_flag"][first + 2, l] = bi["mvp_flag"][l::2]
        # every block a candidate reads, filter taps included, must lie inside the padded planes
        for mv in (uni_mv, bi_mv):
            for c, (size, lim) in enumerate(((self.pus["w"], self.W), (self.pus["h"], self.H))):
                pos = (self.pus["x0"], self.pus["y0"])[c].astype(np.int64)[:, None] + (mv[:, :, c] >> 2)
                if (pos - 4 < -self.PAD + 8).any() or (pos + size[:, None] + 4 > lim + self.PAD - 8).any():
                    raise RuntimeError("pu_modes: a searched vector leaves the padded reference planes")
        with torch.cuda.stream(hv.tstream):
            P["d_jobs"].copy_(torch.from_numpy(jobs.view(np.uint8).reshape(-1)))
            for g in P["groups"]:
                sel, k = g["sel"], len(g["sel"])
                for q in g["planes"]:
                    sh, fr, size = q["shift"], (1 << q["shift"]) - 1, q["size"]

                    def ref(mv, l):
                        return (q["first_ref"] + l) * q["pe"] + q["here"] + (mv[:, 1] >> sh) * q["stride"] + (mv[:, 0] >> sh)

                    uj = np.zeros((k, 2, 8), np.int32)
                    bj = np.zeros((k, 12), np.int32)
                    for l in (0, 1):
                        mv = uni_mv[sel, l]
                        uj[:, l, 0], uj[:, l, 1] = (3 * np.arange(k) + l) * size * size, ref(mv, l)
                        uj[:, l, 2] = uj[:, l, 3] = size
                        uj[:, l, 4], uj[:, l, 5] = mv[:, 0] & fr, mv[:, 1] & fr
                        mv = bi_mv[sel, l]
                        bj[:, 1 + l] = ref(mv, l)
                        bj[:, 5 + 2 * l], bj[:, 6 + 2 * l] = mv[:, 0] & fr, mv[:, 1] & fr
                    bj[:, 0] = (3 * np.arange(k) + 2) * size * size
                    bj[:, 3] = bj[:, 4] = size
                    q["d_uj"].copy_(torch.from_numpy(uj.reshape(-1)))
                    q["d_bj"].copy_(torch.from_numpy(bj.reshape(-1)))
            if self.commit:     # every candidate's vectors [list][x, y] by its global index, for the cells of the committed units (a list it does not use: 0, 0)
                cand_mv = np.zeros((P["M"], 2, 2), np.int16)
                cand_mv[first, 0], cand_mv[first + 1, 1], cand_mv[first + 2] = uni_mv[:, 0], uni_mv[:, 1], bi_mv
                if "d_cand_mv" not in P:
                    P["d_cand_mv"] = hv.zeros(cand_mv.size, np.int16)
                P["cand_mv"] = cand_mv
                P["d_cand_mv"].copy_(torch.from_numpy(cand_mv.reshape(-1)))

    def pu_mode_launches(self):
        """measurePuCost and go2's comparison as batches over the tables pu_candidates() uploaded: per unit size and plane HavocPredUni of the L0 and L1 candidates,
        HavocPredBi of the bi candidate (8-tap luma, 4-tap Cb / Cr) and the Hadamard SATD of all three against the source (as merge_candidates measures it), then the
        candidates' CABAC bits and the decision.  3 launches per (size, plane) + 2; asynchronous"""
        hv, bd, P = self.hv, self.bd, self._pu_plan()
        M = P["M"]
        for g in P["groups"]:
            for plane, q in enumerate(g["planes"]):
                ref = self.d_cpic if plane else self.d_pic
                hv.pred_uni_d(q["taps"], bd, q["d_dst"], q["size"], ref, q["stride"], q["d_uj"].view(-1, 8), q["size"], q["size"])
                hv.pred_bi_d(q["taps"], bd, q["d_dst"], q["size"], ref, q["stride"], q["d_bj"].view(-1, 12), q["size"], q["size"])
                hv.satd_d(ref, q["stride"], q["d_dst"], q["size"], q["d_sj"], P["d_satd"][plane * M + g["at"]:plane * M + g["at"] + g["m"]], q["size"], q["size"])
        hv.pu_rate_d(self.d_pu_syntax_states, P["d_jobs"], P["slice"], P["d_rate"], P["d_after"])
        lam_q16 = int(float(self.params.reciprocal_sqrt_lambda) * 65536 + 0.5)      # Lambda::set(double)
        hv.pu_decide_d(P["d_first"], P["d_count"], len(self.pus), P["d_rate"], P["d_satd"][:M], P["d_satd"][M:2 * M], P["d_satd"][2 * M:], lam_q16, P["d_after"],
                       P["d_cost"], P["d_best"], P["d_best_cost"], P["d_best_syntax"])

    @property
    def pu_decisions(self):
        """what pu_mode_launches() left on the device, as numpy, per unit of self.pus: dict(mode [n] (0 L0, 1 L1, 2 bi), cost [n] (Q16), costs [n, 3], syntax [n, 16]
        (the winner's snapshot), rates [n, 3] (Q16), satd [n, 3 candidates, 3 planes], jobs [n, 3] (PU_RATE_JOB_DT as uploaded))"""
        if "pu_modes" not in self._cache:
            hv, P, K = self.hv, self._pu_plan(), self.PU_CANDIDATES
            M, at = P["M"], P["first"][:, None] + np.arange(K)[None, :]
            satd = hv.down(P["d_satd"], np.int32).reshape(3, M)
            self._cache["pu_modes"] = dict(mode=hv.down(P["d_best"], np.int32), cost=hv.down(P["d_best_cost"], np.int64), costs=hv.down(P["d_cost"], np.int64)[at],
                                      syntax=hv.down(P["d_best_syntax"], np.uint8).reshape(-1, self.hmod.PU_SYNTAX_CTX_BYTES),
                                      rates=hv.down(P["d_rate"], np.int64)[at], satd=np.stack([satd[c][at] for c in range(3)], 2),
                                      jobs=hv.down(P["d_jobs"], np.uint8).view(self.hmod.PU_RATE_JOB_DT)[at])
        return self._cache["pu_modes"]

    # ---- closing every transform-tree unit as an inter coding unit (Search<IfCbf<rqt_root_cbf, transform_tree>>::go, turing/Search.hpp:2362-2568) -------------
    def _cu_plan(self):
        """cu_close's job tables and buffers, built once: one job per unit of self.units (the units that have a transform tree), 2Nx2N, not merged, cu_skip_flag's
        context increment 0, from the CTU's snapshots.  The PU rate charged is that of the L0 candidate of the SEARCHED unit of the same place and size (predict() keeps
        the list-0 vector: that is the prediction the tree's residual was made from); a tree unit the search did not visit at that size has no prediction-unit rate
        (pu_rate_index -1) and its record comes back refused."""
        if hasattr(self, "cu_plan"):
            return self.cu_plan
        hv, torch, hmod = self.hv, self.torch, self.hmod
        u, pus, P = self.units, self.pus, self._pu_plan()
        if self.unit_trees:      # the searched units themselves, each charged its WINNER's rate from the winner's snapshot (unit_pred_select, pu_decide), by index
            u = self._unit_tree_plan()["units"]
        n = len(u)
        jobs = np.zeros(n, hmod.CU_CLOSE_JOB_DT)
        jobs["ctx_index"] = jobs["pu_before_index"] = u["ctx_index"]
        if self.unit_trees:
            match = np.arange(n, dtype=np.int64)
            jobs["unit_index"] = jobs["pu_rate_index"] = jobs["pu_after_index"] = match
        else:
            at = {(int(p["x0"]), int(p["y0"]), int(p["w"])): i for i, p in enumerate(pus) if p["part_2Nx2N"] == 1 and p["w"] == p["h"]}
            match = np.array([at.get((int(x), int(y), 1 << int(l)), -1) for x, y, l in zip(u["x0"], u["y0"], u["log2_size"])], np.int64)
            cand = np.where(match >= 0, P["first"][np.maximum(match, 0)], 0)          # the unit's L0 candidate
            jobs["unit_index"], jobs["pu_rate_index"], jobs["pu_after_index"] = np.arange(n), np.where(match >= 0, cand, -1), cand
        jobs["log2_cb_size"], jobs["flags"] = u["log2_size"], np.where(u["log2_size"] == 3, hmod.CU_CLOSE_MIN_CB, 0)
        x, y = u["x0"].astype(np.int64), u["y0"].astype(np.int64)
        hw, hh, c2 = self.W // 2, self.H // 2, self.PAD // 2
        sj = np.zeros(n, hmod.PRED_SSD_JOB_DT)
        here_c = (y // 2 + c2) * self.cstride + x // 2 + c2
        sj["src_off"] = np.stack([(y + self.PAD) * self.stride + x + self.PAD, here_c, 3 * self.cpe + here_c], 1)
        sj["pred_off"] = np.stack([y * self.W + x, (y // 2) * hw + x // 2, hw * hh + (y // 2) * hw + x // 2], 1)
        if self.unit_trees:      # the unit's block in the unit prediction planes
            sj["pred_off"] = self.unit_plan["select_jobs"]["dst_off"]
        sj["log2_size"] = u["log2_size"]
        with torch.cuda.stream(hv.tstream):
            up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(hv.device)
            self.cu_plan = dict(jobs=jobs, ssd_jobs=sj, match=match, d_jobs=up(jobs), d_ssd_jobs=up(sj), d_pred_ssd=hv.zeros(3 * n, np.int32),
                                d_out=hv.zeros(n * hmod.CU_CHOICE_DT.itemsize, np.uint8), d_cu_after=hv.zeros(n * hmod.CU_SYNTAX_CTX_BYTES, np.uint8),
                                d_pu_after=hv.zeros(n * hmod.PU_SYNTAX_CTX_BYTES, np.uint8))
        return self.cu_plan

    def cu_close_launches(self):
        """ssdPrediction of every unit in three planes (source against pred / cpred), then the close over what rqt_decide_tree, pu_rate and that launch left on the
        device.  2 launches; asynchronous"""
        hv, Q, P, R = self.hv, self._cu_plan(), self._pu_plan(), self.rqt_plan
        if self.unit_trees:      # over the searched units: their own prediction planes and trees, the winner's rate and snapshot
            U = self.unit_plan
            hv.unit_pred_ssd_d(self.bd, self.d_pic, self.stride, self.d_cpic, self.cstride, U["pred"], self.W, U["cpred"], self.W // 2, Q["d_ssd_jobs"], Q["d_pred_ssd"])
            hv.cu_close_d(self.d_cu_syntax_states, self.d_pu_syntax_states, P["d_best_syntax"], U["d_unit_rate"], U["d_out"], U["d_tree_out"], U["tree_rate"],
                          Q["d_pred_ssd"], Q["d_jobs"], P["slice"].max_num_merge_cand, U["rl_q16"], Q["d_out"], Q["d_cu_after"], Q["d_pu_after"])
            return
        hv.unit_pred_ssd_d(self.bd, self.d_pic, self.stride, self.d_cpic, self.cstride, self.pred, self.W, self.cpred, self.W // 2, Q["d_ssd_jobs"], Q["d_pred_ssd"])
        hv.cu_close_d(self.d_cu_syntax_states, self.d_pu_syntax_states, P["d_after"], P["d_rate"], R["d_out"], R["d_tree_out"], R["tree_rate"], Q["d_pred_ssd"],
                      Q["d_jobs"], P["slice"].max_num_merge_cand, R["rl_q16"], Q["d_out"], Q["d_cu_after"], Q["d_pu_after"])

    @property
    def cu_decisions(self):
        """what cu_close_launches() left on the device, as numpy, per unit of self.units: dict(records (havoc.CU_CHOICE_DT [n]), cu_syntax [n, 16], pu_syntax [n, 16]
        (the snapshots as the winner left them), pred_ssd int32 [n, 3], jobs (CU_CLOSE_JOB_DT as uploaded), searched [n] (the index in self.pus of the searched unit
        whose L0 rate was charged, -1: none, the record is refused)).  With unit_trees=True the units are self.pus themselves (searched = arange(n)) and the
        rate charged is the WINNER's of pu_decide, from the winner's snapshot."""
        if not self.cu_close:
            raise ValueError("cu_decisions: the picture was made without cu_close=True")
        if "cu_close" not in self._cache:
            hv, Q, hmod = self.hv, self._cu_plan(), self.hmod
            self._cache["cu_close"] = dict(records=hv.down(Q["d_out"], np.uint8).view(hmod.CU_CHOICE_DT).copy(),
                                      cu_syntax=hv.down(Q["d_cu_after"], np.uint8).reshape(-1, hmod.CU_SYNTAX_CTX_BYTES),
                                      pu_syntax=hv.down(Q["d_pu_after"], np.uint8).reshape(-1, hmod.PU_SYNTAX_CTX_BYTES),
                                      pred_ssd=hv.down(Q["d_pred_ssd"], np.int32).reshape(-1, 3), jobs=Q["jobs"], searched=Q["match"])
        return self._cache["cu_close"]

    # ---- the coding quadtree of every CTU over the closed units (Search<coding_quadtree>::go, turing/Search.hpp:808-886) ---------------------------------------
    CQT_CTB_LOG2, CQT_MIN_CB_LOG2 = 6, 3

    def _cqt_plan(self):
        """cqt_decide's node table and buffers, built once from self.units: a unit of size 2^L at (x, y) is the node of its CTU at depth 6 - L (index (4^d - 1) / 3 +
        the z-order index of its place); every other node is -1.  The slice's initial snapshot is CTU 0's of cu_syntax_states."""
        if hasattr(self, "cqt_plan"):
            return self.cqt_plan
        hv, torch, hmod = self.hv, self.torch, self.hmod
        ctb, mcb = self.CQT_CTB_LOG2, self.CQT_MIN_CB_LOG2
        u, nodes = self.units, hmod.cqt_nodes(ctb, mcb)
        if self.unit_trees:      # the node table of the searched units: a 64x64 node has a candidate, a node whose four sub-units were searched is compared
            u = self._unit_tree_plan()["units"]
        x, y, l = u["x0"].astype(np.int64), u["y0"].astype(np.int64), u["log2_size"].astype(np.int64)
        d = ctb - l
        assert (d >= 0).all() and (d <= ctb - mcb).all() and self.cx == -(-self.W >> ctb) and self.cy == -(-self.H >> ctb)
        px, py = (x & 63) >> l, (y & 63) >> l
        z = np.zeros(len(u), np.int64)
        for b in range(ctb - mcb):
            z |= (px >> b & 1) << (2 * b) | (py >> b & 1) << (2 * b + 1)
        node_cu = np.full((self.cx * self.cy, nodes), -1, np.int32)
        node_cu[(y >> ctb) * self.cx + (x >> ctb), (4 ** d - 1) // 3 + z] = np.arange(len(u))
        with torch.cuda.stream(hv.tstream):
            d_node_cu = torch.from_numpy(node_cu.reshape(-1).copy()).to(hv.device)
        self.cqt_plan = dict(node_cu=node_cu, d_node_cu=d_node_cu, **hv.cqt_buffers(self.W, self.H, ctb, mcb))
        return self.cqt_plan

    def cqt_launch(self):
        """the coding quadtree of every CTU over the records cu_close_launches() left on the device, WPP on, ecu off.  One call; asynchronous"""
        hv, Q, B = self.hv, self._cu_plan(), self._cqt_plan()
        hv.cqt_decide_d(self.W, self.H, self.CQT_CTB_LOG2, self.CQT_MIN_CB_LOG2, self.hmod.CQT_WPP, self.d_cu_syntax_states, B["d_node_cu"], Q["d_out"], B["work"],
                        B["ctu"], B["node"], B["depth"], B["cu_syntax_out"])

    @property
    def cqt_decisions(self):
        """what cqt_launch() left on the device, as numpy: dict(ctus (havoc.CQT_CTU_DT [CTUs]), nodes (CQT_NODE_DT [CTUs, 85]), depth (int8 [8 cy, 8 cx]: CtDepth per
        8x8 cell, whole CTUs, 0 outside the picture), cu_syntax (uint8 [CTUs, 16]: the snapshot after each CTU), node_cu (int32 [CTUs, 85] as uploaded), gave_up (a wait
        on the row above gave up: every record then has decided = 0 and nothing is to be used)).
        The limit today: only the units that have a transform tree have a closed coding unit -- 32x32, and 16x16 / 8x8 along a partial edge -- so every 64x64 node is
        without a candidate and splits, every 32x32 unit stands without a comparison (no node below it has a candidate), a unit whose record cu_close refused refuses
        its CTU (decided = 0), and no full-against-split comparison is live until
        trees exist at every searched size.  What a picture does exercise: the forced splits and deleted quadtrees of a partial last row and column, the depth map,
        and the context chain over real rows.  unit_trees=True lifts the limit: the node table is built from the searched units (self.pus), a 64x64 node has a
        candidate, a node whose four sub-units were searched is compared, and every CTU is decided."""
        if not self.cqt:
            raise ValueError("cqt_decisions: the picture was made without cqt=True")
        if "cqt" not in self._cache:
            B = self._cqt_plan()
            work = self.hv.down(B["work"], np.int64)        # [CTUs]: the published words; then the row ticket (low half) and the give-up word (high half)
            self._cache["cqt"] = dict(node_cu=B["node_cu"], gave_up=bool(work[self.cx * self.cy] >> 32),
                                       **self.hv.cqt_download(B, self.W, self.H, self.CQT_CTB_LOG2, self.CQT_MIN_CB_LOG2))
        return self._cache["cqt"]

    # ---- acting on the decision: the final units of every decided CTU into one picture and a per-cell field (havoc_mi355x_cqt_commit) ----------------------------
    def cqt_commit_launch(self):
        """behind cqt_launch: of the searched units the final coding units of the decided quadtrees -- a unit left without residual or skipped as its block of the unit
        prediction planes, a coded unit as the candidate pieces of the transform depth that stands -- into cqt_recon / cqt_crecon, and cqt_cells.  Everything is read
        where the launches before left it.  One call (a fill and a launch); asynchronous"""
        hv, P, U, Q, B = self.hv, self._pu_plan(), self._unit_tree_plan(), self._cu_plan(), self._cqt_plan()
        if "d_pred_off" not in U:
            U["d_pred_off"] = hv.up(np.ascontiguousarray(U["select_jobs"]["dst_off"], np.int32).reshape(-1))
        piece = lambda groups, sizes: [groups[s]["piece"] if s in groups else None for s in sizes]
        hv.cqt_commit_d(self.bd, self.W, self.H, self.CQT_CTB_LOG2, self.CQT_MIN_CB_LOG2, U["d_units"], B["d_node_cu"], B["ctu"], B["node"], Q["d_out"], U["d_out"],
                        U["d_tree_out"], U["d_zero_at"], U["d_one_at"], U["d_chroma_at"], piece(U["sizes"], (2, 3, 4, 5)), piece(U["csizes"], (2, 3, 4)), U["pred"],
                        self.W, U["cpred"], self.W // 2, U["d_pred_off"], P["d_best"], U["d_unit_cand"], P["d_cand_mv"], self.cqt_recon, self.origin, self.stride,
                        self.cqt_crecon, self.corigin, self.cpe + self.corigin, self.cstride, self.cqt_cells)

    def cqt_commit_results(self):
        """what cqt_commit_launch() left on the device, as numpy, cropped to the picture: dict(recon dt [H, W], crecon dt [2, H / 2, W / 2], cells (havoc.CQT_CELL_DT
        [H / 8, W / 8]: unit -1 in an undecided CTU))"""
        if not self.commit:
            raise ValueError("cqt_commit_results: the picture was made without commit=True")
        if self.finish:
            raise ValueError("cqt_commit_results: with finish=True the committed planes are filtered in place: cqt_finish_results() has them")
        if "commit" not in self._cache:
            hv, pad, c2 = self.hv, self.PAD, self.PAD // 2
            y = hv.down(self.cqt_recon, self.dt)[:self.n].reshape(-1, self.stride)[pad:pad + self.H, pad:pad + self.W]
            c = hv.down(self.cqt_crecon, self.dt)
            c = np.stack([c[k * self.cpe:k * self.cpe + self.cn].reshape(-1, self.cstride)[c2:c2 + self.H // 2, c2:c2 + self.W // 2] for k in range(2)])
            self._cache["commit"] = dict(recon=y.copy(), crecon=c, cells=hv.cqt_cells_download(self.cqt_cells, self.W, self.H, self.CQT_MIN_CB_LOG2))
        return self._cache["commit"]

    # ---- the committed picture's motion as the next picture's collocated store (turing/StateCollocatedMotion.h:51-122) -------------------------------------------
    def cqt_motion_launch(self):
        """directly behind cqt_commit_launch: cqt_cells as the collocated motion store, into cqt_store.  It reads cqt_cells only -- with or without finish.  One
        launch; asynchronous"""
        poc, ref_poc0, ref_poc1 = self.motion
        self.hv.cqt_motion_store_d(self.W, self.H, self.CQT_MIN_CB_LOG2, poc, ref_poc0, ref_poc1, self.cqt_cells, self.cqt_store)

    def cqt_motion_results(self):
        """what cqt_motion_launch() left on the device, as numpy: havoc.COL_CELL_DT [(H + 15) // 16, (W + 15) // 16]"""
        if self.motion is None:
            raise ValueError("cqt_motion_results: the picture was made without motion=(poc, ref_poc0, ref_poc1)")
        if "motion" not in self._cache:
            self._cache["motion"] = self.hv.down(self.cqt_store, np.uint8).view(self.hmod.COL_CELL_DT).reshape((self.H + 15) // 16, (self.W + 15) // 16).copy()
        return self._cache["motion"]

    # ---- this picture's temporal candidates from another picture's store (turing/Mvp.h:44-181) --------------------------------------------------------------------
    def temporal_launch(self):
        """the temporal candidate of every unit of self.pus, per list, from col["store"] (dense rows).  It reads nothing this picture's step writes.  One launch;
        asynchronous.  Ordering against the step that writes the store is the caller's (see __init__)"""
        self.hv.temporal_candidates_d(self._temporal_params, self.col["store"], (self.W + 15) // 16, self._pus_table(), len(self.pus), self._d_temporal)

    def temporal_candidates(self):
        """what temporal_launch() left on the device, as numpy: havoc.TEMPORAL_CAND_DT [len(self.pus), 2] (unit, list)"""
        if self.col is None:
            raise ValueError("temporal_candidates: the picture was made without col=")
        if "col" not in self._cache:
            n = len(self.pus)
            self._cache["col"] = self.hv.down(self._d_temporal, np.uint8)[:2 * n * self.hmod.TEMPORAL_CAND_DT.itemsize].view(self.hmod.TEMPORAL_CAND_DT).reshape(n, 2).copy()
        return self._cache["col"]

    # ---- the committed picture's merge candidate lists (turing/Mvp.h:486-716) -----------------------------------------------------------------------------------
    def cqt_merge_launch(self):
        """behind cqt_commit_launch and, with col=, behind temporal_launch: the merge candidate list of every final coding unit from cqt_cells (the neighbours in their
        final state) and this picture's temporal records, into cqt_merge.  One launch; asynchronous"""
        self.hv.cqt_merge_lists_d(self._merge_params, self.cqt_cells, self._pus_table(), len(self.pus), self._d_temporal if self.col is not None else None,
                                  self.cqt_merge)

    def cqt_merge_results(self):
        """what cqt_merge_launch() left on the device, as numpy: havoc.MERGE_LIST_DT [len(self.pus)] -- a final unit's list, n_real and match; any other unit: zero
        bytes with match -1"""
        if self.merge_lists is None:
            raise ValueError("cqt_merge_results: the picture was made without merge_lists=max_cand")
        if "merge_lists" not in self._cache:
            self._cache["merge_lists"] = self.hv.cqt_merge_lists_download(self.cqt_merge, len(self.pus))
        return self._cache["merge_lists"]

    # ---- the committed picture finished: block structure, boundary strengths, deblocking, padding (turing/TaskDeblock.cpp:105-167) --------------------------------
    def cqt_finish_launch(self):
        """behind cqt_commit_launch: the committed cells as 4x4 cells (lists 0 and 1 are two different decoded pictures: dpb indices 0 and 1), the boundary strengths
        derived from them, deblocking of cqt_recon / cqt_crecon in place, padding of the three planes on all four sides.  Seven launches; asynchronous"""
        hv, W, H, c2 = self.hv, self.W, self.H, self.PAD // 2
        o, co, cs = self.origin, self.corigin, self.cstride
        hv.cqt_block_cells_d(W, H, self.CQT_MIN_CB_LOG2, self.qp, 0, 1, self.cqt_cells, self.cqt_block, W // 4)
        hv.derive_bs_d(self.cqt_block, W // 4, W, H, self.cqt_data, self.cqt_bs)
        hv.deblock_d(self.bd, self.cqt_recon, o, self.stride, self.cqt_crecon, co, self.cpe + co, cs, W, H, self.cqt_data, self.cqt_bs)
        hv.pad_block_d(self.cqt_recon, o, W, H, self.stride, self.PAD)
        hv.pad_block_d(self.cqt_crecon, co, W // 2, H // 2, cs, c2)
        hv.pad_block_d(self.cqt_crecon, self.cpe + co, W // 2, H // 2, cs, c2)

    def cqt_finish_results(self):
        """what cqt_finish_launch() left on the device, as numpy: dict(recon dt [rows, stride]: the whole padded luma plane; crecon dt [2, chroma rows, cstride]: both
        whole padded chroma planes; cells havoc.CELL_DT [H / 4, W / 4]; data int8, bs uint8: the region grid's edge data)"""
        if not self.finish:
            raise ValueError("cqt_finish_results: the picture was made without finish=True")
        if "finish" not in self._cache:
            hv = self.hv
            c = hv.down(self.cqt_crecon, self.dt)
            self._cache["finish"] = dict(recon=hv.down(self.cqt_recon, self.dt)[:self.n].reshape(-1, self.stride).copy(),
                                    crecon=np.stack([c[k * self.cpe:k * self.cpe + self.cn].reshape(-1, self.cstride) for k in range(2)]),
                                    cells=hv.down(self.cqt_block, np.uint8).view(self.hmod.CELL_DT).reshape(self.H // 4, self.W // 4).copy(),
                                    data=hv.down(self.cqt_data, np.int8).copy(), bs=hv.down(self.cqt_bs, np.uint8).copy())
        return self._cache["finish"]

    def chroma_chain(self, field):
        """the inter residual of the chroma planes at the decided vectors (turing/Reconstruct.cpp:1274-1286 with cIdx 1, 2): HavocPredUni 4-tap of every unit's
        Cb and Cr block at its list-0 vector (eighth-sample phase = the luma vector's low three bits), then the chain (Rdoq::runQuantisation with cIdx), one per
        chroma transform size and component, into the chroma reconstruction planes.  Asynchronous."""
        self.chroma_predict()
        self._chain(self.cgroups, self.d_cpic, self.cstride, self.cpred, self.W // 2, self.crecon, self.cstride)

    def chroma_predict(self):
        """the prediction half of chroma_chain alone: every unit's Cb and Cr block at its decided vector into cpred (tree_rates=True: the chroma candidates of both
        depths are evaluated from it)"""
        hv = self.hv
        self._chroma_groups()
        for g in self.cgroups:
            hv.pred_jobs_d(self.layout, self.d_field, 0, g["d_x0"], g["d_y0"], g["log2"] + 1, g["comp"], g["d_dst"], g["d_pj"])
            hv.pred_uni_d(4, self.bd, self.cpred, self.W // 2, self.d_cpic, self.cstride, g["d_pj"].view(-1, 8), g["nn"], g["nn"])

    def _chroma_groups(self):
        """chroma_chain's job tables and buffers per (unit size, component), built once"""
        if hasattr(self, "cgroups"):
            return
        hv, u = self.hv, self.units
        hw, hh, c2 = self.W // 2, self.H // 2, self.PAD // 2
        self.cgroups = []
        for log2 in (5, 4, 3):
            sel = np.flatnonzero(u["log2_size"] == log2)
            if not len(sel):
                continue
            cl, m = log2 - 1, len(sel)
            x0, y0 = u["x0"][sel].astype(np.int64) // 2, u["y0"][sel].astype(np.int64) // 2
            at = (y0 + c2) * self.cstride + x0 + c2
            for comp in (1, 2):
                # the block's slot; its source in d_cpic, its prediction in cpred, its reconstruction in crecon
                fj = np.stack([np.arange(m) << 2 * cl, 3 * (comp - 1) * self.cpe + at, (comp - 1) * hw * hh + y0 * hw + x0, (comp - 1) * self.cpe + at], 1).astype(np.int32)
                # (cn: the block size under the name the readers of this list know it by; every group has it as nn)
                self.cgroups.append(dict(self._chain_group(cl, fj, u["ctx_index"][sel], comp), cn=1 << cl, comp=comp, sel=sel, d_x0=hv.up(u["x0"][sel].astype(np.int32)),
                                         d_y0=hv.up(u["y0"][sel].astype(np.int32)), d_dst=hv.up(fj[:, 2]), d_pj=hv.zeros(m * 8, np.int32)))

    def tu_chain(self, field, predicted=False):
        """prediction at the decided vectors, then the residual-quadtree decisions and the reconstruction; returns (decisions, stats)"""
        if not predicted:
            self.predict(field)
        base = self.d_pic.data_ptr()
        self.rqt_results, st = rqt(self.hv.h, self.S, self.bd, base, self.origin, self.stride, self.pred.data_ptr(), self.W, self.recon.data_ptr(), self.origin,
                                   self.stride, self.d_states.data_ptr(), self.quant, self.lam, 1.0 / self.lam, self.units)
        self.rqt_stats = st
        return self.rqt_results, st

    # ---- round 4: the transform-tree decision and the block structure on the device -- nothing of the picture's step waits for the host after its searches ----
    def _tree_tables(self, u, plane, chroma, final=False, stats=False, rates=False):
        """the tables and buffers of the transform-tree decisions of the units u (RQT_CU_DT), built ONCE (the units of a picture do not move): per transform size the
        luma candidates' group, with chroma per chroma transform size the Cb / Cr candidates' group and the tree-rate jobs per (unit size, depth) -- laid out by
        tu_plan.candidate_layout -- where each unit finds its candidates, and the decision's tables and outputs.  plane[i]: which of the unit prediction planes holds
        unit i's prediction (plane p of luma at p W H, of Cb / Cr at 2 p and 2 p + 1 chroma planes; 0: the picture's own pred / cpred)"""
        hv, n = self.hv, len(u)
        W, hw, c2 = self.W, self.W // 2, self.PAD // 2
        ypl, cpl = W * self.H, hw * (self.H // 2)
        lay = tu_plan.candidate_layout(u["log2_size"])
        x0, y0, ctx = u["x0"].astype(np.int64), u["y0"].astype(np.int64), u["ctx_index"]
        row = lambda g: [g[k].data_ptr() if k in g else 0 for k in ("cbf", "ssd", "stats", "d_jobs", "d_fin")]      # (havoc_rqt_size; absent: not made on this route)
        plan = dict(units=u, zero_at=lay["zero_at"], one_at=lay["one_at"], sizes={}, table=np.zeros((4, 5), np.uint64), rl_q16=int((1.0 / self.lam) * 65536 + 0.5),
                    d_units=hv.up(np.ascontiguousarray(u).view(np.int32)), d_zero_at=hv.up(lay["zero_at"]), d_one_at=hv.up(lay["one_at"]),
                    d_out=hv.zeros(n * 26, np.int32))
        for log2, c in lay["luma"].items():
            x, y = tu_plan.candidate_xy(x0, y0, c, log2)
            slot = np.arange(len(c)) << 2 * log2
            jobs = np.stack([slot, self.origin + y * self.stride + x, plane[c[:, 0]] * ypl + y * W + x, slot], 1).astype(np.int32)
            g = plan["sizes"][log2] = dict(self._chain_group(log2, jobs, ctx[c[:, 0]], pieces=True, final=final, stats=stats, rates=rates), cand=c)
            plan["table"][log2 - 2] = row(g)
        if not chroma:
            return plan
        plan.update(csizes={}, ctable=np.zeros((4, 5), np.uint64), chroma_at=lay["chroma_at"], d_chroma_at=hv.up(np.ascontiguousarray(lay["chroma_at"]).view(np.int32)),
                    tree_rate=self._zeros64(2 * n), tree_cbf=hv.zeros(2 * n, np.int32), d_tree_out=hv.zeros(4 * n, np.int32))
        for cl, c in lay["chroma"].items():
            x, y = tu_plan.candidate_xy(x0, y0, c, cl, chroma=True)
            comp, slot = c[:, 2], np.arange(len(c)) << 2 * cl
            jobs = np.stack([slot, 3 * (comp - 1) * self.cpe + (y + c2) * self.cstride + x + c2, (2 * plane[c[:, 0]] + comp - 1) * cpl + y * hw + x, slot], 1).astype(np.int32)
            g = plan["csizes"][cl] = dict(self._chain_group(cl, jobs, ctx[c[:, 0]], comp, pieces=True, final=final), cand=c)
            plan["ctable"][cl - 2] = row(g)
        plan["tree_jobs"] = {key: dict(jobs=tj, d_jobs=self._up_records(tj), luma=luma, chroma=chroma_size)
                             for key, (tj, luma, chroma_size) in tu_plan.tree_rate_jobs(lay, u["log2_size"], ctx).items()}
        return plan

    def _rqt_plan(self):
        """the tree plan of self.units, the prediction in pred / cpred: what havoc_search_rqt builds per call.  The default route has the level statistics of the
        stand-in rate; residual_rates=True a CABAC rate per luma candidate; tree_rates=True the chroma candidates and the whole trees' rates.  Every route
        reconstructs the chosen candidates into the picture: final records"""
        hmod, u = self.hmod, self.units
        plan = self._tree_tables(u, np.zeros(len(u), np.int64), self.tree_rates, final=True, stats=not (self.residual_rates or self.tree_rates), rates=self.residual_rates)
        plan["rates"] = np.zeros(4, np.uint64)
        if self.residual_rates:
            for log2, g in plan["sizes"].items():
                # a depth-0 candidate is a job of its own; the four depth-1 candidates of a unit lie one after the other: ONE job that walks them in z-order with
                # the contexts running on, as the reference codes them -- each from the unit's snapshot, like the RDOQ jobs
                c = g["cand"]
                lead = np.flatnonzero(c[:, 2] == 0)
                qj = np.zeros(len(lead), hmod.RESIDUAL_RATE_JOB_DT)
                qj["level_off"], qj["rate_index"], qj["ctx_index"] = g["jobs"][lead, 0], lead, u["ctx_index"][c[lead, 0]]
                qj["sdh"], qj["count"] = 1, np.where(c[lead, 1] == 1, 4, 1)
                g["rate_jobs"], g["d_qj"] = qj, self._up_records(qj)
                plan["rates"][log2 - 2] = g["rates"].data_ptr()
        plan["launches"] = 5 * len(plan["sizes"]) + 1
        # a block-sized area nobody reads, inside the reconstruction's bottom border (rewritten by the padding that ends the step): where the candidates that lost go
        plan["dump"] = (self.H + self.PAD + 16) * self.stride + self.PAD
        if self.tree_rates:
            # ... and the chroma candidates that lost: inside the chroma reconstruction's bottom border (nothing reads it)
            plan["cdump"] = (self.H // 2 + self.PAD // 2 + 8) * self.cstride + self.PAD // 2
            # (4 per chroma size, 1 per tree job, chroma prediction: 2 per unit size and component; no level_stats)
            plan["launches"] += 4 * len(plan["csizes"]) + len(plan["tree_jobs"]) + 4 * len(np.unique(u["log2_size"])) - len(plan["sizes"])
        return plan

    def _filter_buffers(self):
        """the block structure and the loop filter's edge data on the region grid: one set per picture, whatever decides its units -- the whole-picture plan, the band
        views or the host route -- and with finish=True a second set for the committed picture (cqt_block: havoc.CELL_DT per 4x4 cell)"""
        hv, torch = self.hv, self.torch
        self.region_stride = (self.W + 63) // 64 * 8 + 1
        n, cells = self.region_stride * ((self.H + 63) // 64 * 8 + 1), (self.H // 4) * (self.W // 4) * self.hmod.CELL_DT.itemsize
        with torch.cuda.stream(hv.tstream):
            self.d_data = torch.zeros(n, dtype=torch.int8, device=hv.device)
            self.d_bs = torch.zeros(n, dtype=torch.uint8, device=hv.device)
            self.d_cells = torch.zeros(cells, dtype=torch.uint8, device=hv.device)
        self.d_chroma = hv.up(np.full(2 * (self.H // 2) * (self.W // 2), 128 << (self.bd - 8), self.dt))
        if self.finish:
            self.cqt_block, self.cqt_data, self.cqt_bs = hv.zeros(cells, np.uint8), hv.zeros(n, np.uint8), hv.zeros(n, np.uint8)     # (data: int8 values)

    def tree_and_filter_on_device(self):
        """the transform-tree decisions of every inter unit (both depths through residual + DCT -> RDOQ -> IQ + IDCT + add -> SSD, the decision by k_rqt_decide, every
        candidate reconstructed again -- the chosen trees into the picture), the block structure (k_block_cells), boundary strengths, deblocking, padding: launches only"""
        hv, bd = self.hv, self.bd
        P = self.tree_decisions()
        hv.block_cells_d(self.W, self.H, self.qp, 0, self.d_field, P["d_units"].view(-1, 4), P["d_out"], self.d_cells)
        hv.derive_bs_d(self.d_cells, self.W // 4, self.W, self.H, self.d_data, self.d_bs)
        hv.deblock_d(bd, self.recon, self.origin, self.stride, self.d_chroma, 0, (self.H // 2) * (self.W // 2), self.W // 2, self.W, self.H, self.d_data, self.d_bs)
        hv.pad_block_d(self.recon, self.origin, self.W, self.H, self.stride, self.PAD)

    # ---- in-loop SAO (sao=True): deblocked picture -> sao_estimate -> sao_decide -> sao_apply -> padded reference (turing/TaskSao.cpp:96-154) ---------------
    def sao_filter_inputs(self, field):
        """what the loop filter of a sao=True step reads: the transform-tree decisions, the block structure, the boundary strengths, and the chroma chain's
        reconstruction (crecon).  Launches only."""
        hv = self.hv
        P = self.tree_decisions()
        hv.block_cells_d(self.W, self.H, self.qp, 0, self.d_field, P["d_units"].view(-1, 4), P["d_out"], self.d_cells)
        hv.derive_bs_d(self.d_cells, self.W // 4, self.W, self.H, self.d_data, self.d_bs)
        self.chroma_chain(field)

    def _sao_buffers(self):
        """the deblocked copies, the scratch destination of the SAO decision, its records and workspaces and the CTU table over this picture's layout: source
        luma at plane 0 of d_pic, source Cb / Cr at planes 0 / 3 of d_cpic; deblocked picture and destination in the layout of recon / crecon (Cr at cpe)"""
        if hasattr(self, "deblocked"):
            return
        hv, torch, hmod = self.hv, self.torch, self.hmod
        self.deblocked, self.cdeblocked = hv.zeros(self.pe, self.dt), hv.zeros(2 * self.cpe, self.dt)
        self.sao_dst, self.csao_dst = hv.zeros(self.pe, self.dt), hv.zeros(2 * self.cpe, self.dt)
        rows = []
        c2 = self.PAD // 2
        for y in range(0, self.H, 64):
            for x in range(0, self.W, 64):
                oy = (y + self.PAD) * self.stride + x + self.PAD
                oc = (y // 2 + c2) * self.cstride + x // 2 + c2
                w, h = min(64, self.W - x), min(64, self.H - y)
                rows.append((oy, oc, 3 * self.cpe + oc, oy, oc, self.cpe + oc, oy, oc, self.cpe + oc, w, h, 0, oc, 3 * self.cpe + oc, oc, self.cpe + oc))
        self.sao_ctus = np.array(rows, np.int32).view(hmod.SAO_CTU_DT).reshape(-1)
        n = len(self.sao_ctus)
        with torch.cuda.stream(hv.tstream):
            self.d_sao_ctus = torch.from_numpy(self.sao_ctus.view(np.uint8).reshape(-1).copy()).to(hv.device)
            self.d_sao_params = torch.zeros(n * hmod.SAO_PARAMS_DT.itemsize, dtype=torch.uint8, device=hv.device)
            self.d_sao_decisions = torch.zeros(n * hmod.SAO_DECISION_DT.itemsize, dtype=torch.uint8, device=hv.device)
        self.sao_work, self.sao_decide_work = hv.sao_workspace(n), hv.sao_decide_workspace(n)
        self.sao_ctx = hmod.sao_context_init(self.qp, 2)          # a B slice

    def sao_loop_filter(self):
        """one deblocking call over the luma and the real chroma reconstruction; a copy of the deblocked planes padded by edge replication (the decision
        filters one sample beyond the picture); sao_estimate -> sao_decide (WPP, the picture's lambda) into scratch planes; sao_apply from the deblocked
        copy into recon / crecon; padding.  Launches only."""
        self._sao_buffers()
        hv, bd, W, H, c2 = self.hv, self.bd, self.W, self.H, self.PAD // 2
        o, co, cs = self.origin, self.corigin, self.cstride
        hv.deblock_d(bd, self.recon, o, self.stride, self.crecon, co, self.cpe + co, cs, W, H, self.d_data, self.d_bs)
        # the copy: sao_apply with both slice flags 0 copies every picture sample
        hv.sao_apply_d(bd, 0, W, H, 6, self.recon, o, self.crecon, co, self.cpe + co, self.stride, cs, self.deblocked, o, self.cdeblocked, co,
                       self.cpe + co, self.stride, cs, self.d_sao_decisions)
        hv.pad_block_d(self.deblocked, o, W, H, self.stride, self.PAD)
        hv.pad_block_d(self.cdeblocked, co, W // 2, H // 2, cs, c2)
        hv.pad_block_d(self.cdeblocked, self.cpe + co, W // 2, H // 2, cs, c2)
        q16 = self.rqt_plan["rl_q16"]
        sl = (self.stride, cs)
        hv.sao_estimate_d(bd, q16, 3, self.d_pic, self.d_cpic, *sl, self.deblocked, self.cdeblocked, *sl, self.sao_dst, self.csao_dst, *sl, self.d_sao_ctus,
                          self.sao_work, self.d_sao_params)
        hv.sao_decide_d(bd, q16, 7, self.d_pic, self.d_cpic, *sl, self.deblocked, self.cdeblocked, *sl, self.sao_dst, self.csao_dst, *sl, self.d_sao_ctus,
                        self.cx, self.d_sao_params, self.sao_ctx[0], self.sao_ctx[1], self.sao_decide_work, self.d_sao_decisions)
        hv.sao_apply_d(bd, 3, W, H, 6, self.deblocked, o, self.cdeblocked, co, self.cpe + co, self.stride, cs, self.recon, o, self.crecon, co, self.cpe + co,
                       self.stride, cs, self.d_sao_decisions, None, self.d_data, self.region_stride)
        hv.pad_block_d(self.recon, o, W, H, self.stride, self.PAD)
        hv.pad_block_d(self.crecon, co, W // 2, H // 2, cs, c2)
        hv.pad_block_d(self.crecon, self.cpe + co, W // 2, H // 2, cs, c2)

    @property
    def sao_decisions(self):
        """the SAO decisions of the last sao=True step (SAO_DECISION_DT per 64x64 CTU in raster order): downloaded when asked for"""
        if "sao" not in self._cache:
            self._cache["sao"] = self.hv.down(self.d_sao_decisions, np.uint8).view(self.hmod.SAO_DECISION_DT).copy()
        return self._cache["sao"]

    def tree_decisions(self):
        """the transform-tree part of tree_and_filter_on_device for self.units: the luma candidates of both depths through the chain into pieces, each size followed by
        its level statistics (residual_rates=True: its CABAC rates), and the decision; tree_rates=True: chroma prediction, the luma and then the chroma candidates
        (cIdx 1 / 2), the whole-tree rate and cbf mask per (unit size, depth), and the decision over three planes.  Then every candidate reconstructed again -- the
        chosen trees' luma into recon and, with tree_rates, their chroma into crecon.  Returns the plan (its d_units / d_out are what the block structure is made from)"""
        hv = self.hv
        if not hasattr(self, "rqt_plan"):
            self.rqt_plan = self._rqt_plan()
        P = self.rqt_plan
        luma, chroma = (self.d_pic, self.stride, self.pred, self.W), (self.d_cpic, self.cstride, self.cpred, self.W // 2)
        units = (P["d_units"].view(-1, 4), P["d_zero_at"], P["d_one_at"], P["table"])
        if self.tree_rates:
            self.chroma_predict()
            self._chain(P["sizes"].values(), *luma)
            self._chain(P["csizes"].values(), *chroma)
            self._tree_rates(P)
            hv.rqt_decide_tree_d(*units, P["ctable"], P["d_chroma_at"], P["tree_rate"], P["tree_cbf"], self.origin, self.stride, P["dump"], self.corigin,
                                 self.cpe + self.corigin, self.cstride, P["cdump"], P["rl_q16"], P["d_out"], P["d_tree_out"])
            self._chain_final(P["sizes"].values(), *luma, self.recon, self.stride)
            self._chain_final(P["csizes"].values(), *chroma, self.crecon, self.cstride)
        elif self.residual_rates:
            self._chain(P["sizes"].values(), *luma, then=lambda g: hv.residual_rate_d(g["log2"], g["level"], self.d_states, g["d_qj"], g["rates"]))
            hv.rqt_decide_rated_d(*units, P["rates"], self.origin, self.stride, P["dump"], P["rl_q16"], P["d_out"])
            self._chain_final(P["sizes"].values(), *luma, self.recon, self.stride)
        else:
            self._chain(P["sizes"].values(), *luma, then=lambda g: hv.level_stats_d(g["level"], g["d_sj"], g["m"], g["stats"]))
            hv.rqt_decide_d(*units, self.origin, self.stride, P["dump"], P["rl_q16"], P["d_out"])
            self._chain_final(P["sizes"].values(), *luma, self.recon, self.stride)
        return P

    # ---- unit_trees=True: the transform tree of EVERY searched unit, made from the residual of its own winning prediction (what reconstructInter runs on after go2) ----
    def _unit_tree_plan(self):
        """unit_trees' tables and buffers, built once, beside rqt_plan (which still makes recon / crecon / cells from self.pred).  The units are self.pus in their own
        order -- 2Nx2N of 64 to 8, overlapping one another as the quadtree search meets them -- so index p means the same unit in pu_decisions, the tree records,
        cu_decisions and the node table.  Their predictions lie in UNIT PREDICTION PLANES: one luma allocation of four W x H planes and one chroma allocation of four
        (Cb, Cr) plane pairs, plane 6 - L for units of size 2^L, a unit's block at its picture position (stride W, W / 2 for chroma): a job of any launch names its
        block by a 32-bit offset, so one base pointer and stride serve a launch that mixes depth-0 blocks of size-L units with depth-1 blocks of size-(L + 1) units.
        The candidates are laid out as rqt_plan's are (_tree_tables); a 64x64 unit contributes its four 32x32 luma and four 16x16 Cb and Cr blocks only, and
        its one tree-rate job, (6, 1), has no flag bit.  No final job records: nothing of these trees goes into a picture before the quadtree is committed."""
        if hasattr(self, "unit_plan"):
            return self.unit_plan
        hv, hmod, P = self.hv, self.hmod, self._pu_plan()
        pus, n = self.pus, len(self.pus)
        W, hw, hh = self.W, self.W // 2, self.H // 2
        if ((pus["x0"].astype(np.int64) + pus["w"] > W) | (pus["y0"].astype(np.int64) + pus["h"] > self.H)).any():
            raise ValueError("unit_trees=True needs every searched unit inside the picture")
        u = np.zeros(n, RQT_CU_DT)
        u["x0"], u["y0"], u["ctx_index"] = pus["x0"], pus["y0"], (pus["y0"] // 64) * self.cx + pus["x0"] // 64
        for log2 in (6, 5, 4, 3):
            u["log2_size"][pus["w"] == 1 << log2] = log2
        ux, uy, uL = u["x0"].astype(np.int64), u["y0"].astype(np.int64), u["log2_size"].astype(np.int64)
        ypl, cpl = W * self.H, hw * hh                            # a luma plane, a chroma plane
        uplane = 6 - uL
        # where the winner's prediction of every unit goes (havoc_mi355x_unit_pred_select) and where cu_close's ssdPrediction reads it
        sel = np.zeros(n, hmod.PRED_SELECT_JOB_DT)
        for g in P["groups"]:
            i = np.arange(len(g["sel"]))
            sel["cand_off"][g["sel"]] = np.stack([q["base"] + self.PU_CANDIDATES * i * q["size"] ** 2 for q in g["planes"]], 1)
        sel["dst_off"] = np.stack([uplane * ypl + uy * W + ux, 2 * uplane * cpl + (uy // 2) * hw + ux // 2, (2 * uplane + 1) * cpl + (uy // 2) * hw + ux // 2], 1)
        sel["log2_size"], sel["unit"] = uL, np.arange(n)
        plan = self._tree_tables(u, uplane, True)
        plan.update(select_jobs=sel, d_select_jobs=self._up_records(sel), pred=hv.zeros(4 * ypl, self.dt), cpred=hv.zeros(8 * cpl, self.dt),
                    d_unit_cand=hv.zeros(n, np.int32), d_unit_rate=self._zeros64(n),
                    launches=2 + 3 * (len(plan["sizes"]) + len(plan["csizes"])) + len(plan["tree_jobs"]))      # (select and decide; a chain per size; a launch per tree job)
        self.unit_plan = plan
        return plan

    def unit_tree_launches(self):
        """behind pu_mode_launches: the winner's prediction of every searched unit into the unit prediction planes with its rate (one launch for every size), then per
        transform size the luma candidates and per chroma size the Cb / Cr candidates (residual + DCT -> RDOQ from the CTU's snapshot -> IQ + IDCT + add -> SSD, into
        pieces), the whole-tree rate and cbf mask per (unit size, depth), and the decision over three planes without final records.  Asynchronous"""
        hv, P, U = self.hv, self._pu_plan(), self._unit_tree_plan()
        hw = self.W // 2
        hv.unit_pred_select_d(self.bd, P["d_cand_y"], P["d_cand_c"], U["pred"], self.W, U["cpred"], hw, P["d_first"], P["d_best"], P["d_rate"], U["d_select_jobs"],
                              U["d_unit_rate"], U["d_unit_cand"])
        self._chain(U["sizes"].values(), self.d_pic, self.stride, U["pred"], self.W)
        self._chain(U["csizes"].values(), self.d_cpic, self.cstride, U["cpred"], hw)
        self._tree_rates(U)
        hv.rqt_decide_units_d(U["d_units"].view(-1, 4), U["d_zero_at"], U["d_one_at"], U["table"], U["ctable"], U["d_chroma_at"], U["tree_rate"], U["tree_cbf"],
                              U["rl_q16"], U["d_out"], U["d_tree_out"])

    def unit_tree_decisions(self, planes=False):
        """what unit_tree_launches() left on the device, as numpy, per unit of self.pus: dict(units (RQT_CU_DT), choice (RQT_RESULT_DT: rqt_decide_units' records -- a
        64x64 unit has depth 1 when its one tree is coded, else 0, depth 0 untried), tree_choice (havoc.RQT_TREE_RESULT_DT), tree_rate int64 [n, 2] and tree_cbf uint32
        [n, 2] (per depth; entry 0 of a 64x64 unit is nobody's), unit_rate int64 [n] and unit_cand int32 [n] (the winner's PU rate and candidate index, -1 without a
        winner)); planes=True adds pred (dt [4, H, W]: plane 6 - L holds the units of size 2^L) and cpred (dt [4, 2, H / 2, W / 2])"""
        if not self.unit_trees:
            raise ValueError("unit_tree_decisions: the picture was made without unit_trees=True")
        hv, U, hmod = self.hv, self._unit_tree_plan(), self.hmod
        if "unit_trees" not in self._cache:
            with self.torch.cuda.stream(hv.tstream):
                rate, unit_rate = U["tree_rate"].cpu().numpy().reshape(-1, 2), U["d_unit_rate"].cpu().numpy()
            self._cache["unit_trees"] = dict(units=U["units"], choice=hv.down(U["d_out"], np.int32).view(RQT_RESULT_DT).copy(),
                                             tree_choice=hv.down(U["d_tree_out"], np.int32).view(hmod.RQT_TREE_RESULT_DT).copy(), tree_rate=rate,
                                             tree_cbf=hv.down(U["tree_cbf"], np.int32).view(np.uint32).reshape(-1, 2), unit_rate=unit_rate,
                                             unit_cand=hv.down(U["d_unit_cand"], np.int32))
        if not planes:
            return self._cache["unit_trees"]
        return dict(self._cache["unit_trees"], pred=hv.down(U["pred"], self.dt).reshape(4, self.H, self.W),
                    cpred=hv.down(U["cpred"], self.dt).reshape(4, 2, self.H // 2, self.W // 2))

    @property
    def rqt_tree_results(self):
        """tree_rates=True: what the decision over three planes adds per unit (havoc.RQT_TREE_RESULT_DT: both cbf masks, both sums ssdCb + ssdCr): downloaded when
        asked for"""
        if not self.tree_rates:
            raise ValueError("rqt_tree_results: the picture was made without tree_rates=True")
        if "rqt_tree" not in self._cache:
            self._cache["rqt_tree"] = self.hv.down(self.rqt_plan["d_tree_out"], np.int32).view(self.hmod.RQT_TREE_RESULT_DT).copy()
        return self._cache["rqt_tree"]

    @property
    def rqt_results(self):
        """the transform-tree decisions of the last step (RQT_RESULT_DT per unit): downloaded when asked for"""
        if "rqt" not in self._cache:
            self._cache["rqt"] = self.hv.down(self.rqt_plan["d_out"], np.int32).view(RQT_RESULT_DT).copy()
        return self._cache["rqt"]

    @rqt_results.setter
    def rqt_results(self, v):
        self._cache["rqt"] = v

    @property
    def rqt_rates(self):
        """residual_rates=True: {log2: int64 Q16 rate of every candidate of that transform size} of the last step (the order of rqt_plan["sizes"][log2]'s jobs):
        downloaded when asked for"""
        if self.tree_rates:      # ... tree_rates=True: {(unit size, depth): the whole-tree rate of every unit of that size, in the order of rqt_plan["tree_jobs"]}
            if "rqt_rates" not in self._cache:
                with self.torch.cuda.stream(self.hv.tstream):
                    flat = self.rqt_plan["tree_rate"].cpu().numpy()
                self._cache["rqt_rates"] = {key: flat[t["jobs"]["out_index"]].copy() for key, t in self.rqt_plan["tree_jobs"].items()}
            return self._cache["rqt_rates"]
        if not self.residual_rates:
            raise ValueError("rqt_rates: the picture was made without residual_rates=True or tree_rates=True")
        if "rqt_rates" not in self._cache:
            self._cache["rqt_rates"] = {log2: self.hv.down(g["rates"], np.int64).copy() for log2, g in self.rqt_plan["sizes"].items()}
        return self._cache["rqt_rates"]

    @property
    def cells(self):
        """the picture's block structure of the last step (CELL_DT [H / 4, W / 4]): on the device route k_block_cells leaves it in HBM and it is
        downloaded when asked for; the host route (search_on_device=False) made it on the host"""
        if "cells" not in self._cache:
            from .havoc import CELL_DT
            self._cache["cells"] = self.hv.down(self.d_cells, np.uint8).view(CELL_DT).reshape(self.H // 4, self.W // 4).copy()
        return self._cache["cells"]

    @cells.setter
    def cells(self, v):
        self._cache["cells"] = v

    def block_cells(self, field, decisions):
        """the picture's block structure after the decisions, as the 4x4 cells havoc_mi355x_derive_bs reads: every unit one inter 2Nx2N
        prediction unit from list 0 at the vector decided at its origin, its transform tree as decided (coded flags per block)"""
        from .havoc import CELL_DT
        cells = np.zeros((self.H // 4, self.W // 4), CELL_DT)
        field = np.ascontiguousarray(field)
        decisions = np.ascontiguousarray(decisions)
        rc = lib().havoc_search_block_cells(self.W, self.H, self.qp, 0, field.ctypes.data, self.units.ctypes.data, decisions.ctypes.data, len(self.units),
                                            cells.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"havoc_search_block_cells failed ({rc})")
        return cells

    def loop_filter(self, cells):
        """boundary strengths derived on the device from the block structure, in-loop deblocking of the reconstruction (luma; flat chroma planes
        stand in), padding: the reconstruction is then a reference picture.  Asynchronous."""
        hv, torch = self.hv, self.torch
        with torch.cuda.stream(hv.tstream):
            self.d_cells.copy_(torch.from_numpy(cells.view(np.uint8).reshape(-1)), non_blocking=True)
        hv.derive_bs_d(self.d_cells, cells.shape[1], self.W, self.H, self.d_data, self.d_bs)
        hv.deblock_d(self.bd, self.recon, self.origin, self.stride, self.d_chroma, 0, (self.H // 2) * (self.W // 2), self.W // 2, self.W, self.H, self.d_data, self.d_bs)
        hv.pad_block_d(self.recon, self.origin, self.W, self.H, self.stride, self.PAD)

    def tu_chain_fixed(self, field):
        """prediction at the decided list-0 vectors, then residual -> T -> RDOQ -> IQ -> IT + add -> SSD on fixed 16x16 (8x8) blocks; asynchronous"""
        hv, bd, pe = self.hv, self.bd, self.pe
        ref0 = self.d_pic[pe:2 * pe]
        src = self.d_pic[:pe]
        for g in self.groups:
            mv = field[0, g["y0"] >> 2, g["x0"] >> 2].astype(np.int64)          # quarter samples, [m, 2]
            pj = g["pj"]
            pj[:, 0] = g["y0"] * self.W + g["x0"]
            pj[:, 1] = (g["y0"] + (mv[:, 1] >> 2) + self.PAD) * self.stride + g["x0"] + (mv[:, 0] >> 2) + self.PAD
            pj[:, 2] = pj[:, 3] = g["nn"]
            pj[:, 4], pj[:, 5] = mv[:, 0] & 3, mv[:, 1] & 3
            with self.torch.cuda.stream(hv.tstream):
                g["d_pj"].copy_(self.torch.from_numpy(pj.reshape(-1)), non_blocking=True)
            hv.pred_uni_d(8, bd, self.pred, self.W, ref0, self.stride, g["d_pj"].view(-1, 8), g["nn"], g["nn"])
            self._chain([g], src, self.stride, self.pred, self.W, self.recon, self.stride)

    def intra_decisions(self, on_device=True):
        """the intra side of the picture: per partition size the 35-mode SATD stage and its refinement order, then the RD refinement of every
        candidate mode and the champions.  on_device: the order, the candidates' job records and the champions are decided by kernels between the
        launches (havoc_search_intra_device: one call for all sizes, 40 bytes per partition come back); otherwise the two-call route with the
        decisions on the host (havoc_search_intra_modes + havoc_search_intra_rd; the tests' link to the per-call loops).
        Leaves {log2: (order or None, RD champions)} in self.intra_results and the calls' statistics in self.intra_stats"""
        hv = self.hv
        base = self.d_pic.data_ptr()
        out, self.intra_stats = {}, []
        if on_device:
            groups = [dict(log2=log2, n=len(g["jobs"]), d_nb=g["d_nb"].data_ptr(), d_jobs=g["d_jobs"].data_ptr(), d_ictx=g["d_ictx"].data_ptr(), d_ctu=g["d_ctu"].data_ptr(),
                           d_rec=g["d_rec"].data_ptr()) for log2, g in sorted(self.intra_parts.items(), reverse=True)]
            best, st = intra_device(hv.h, self.S, self.bd, base, self.stride, groups, self.d_states.data_ptr(), self.quant, self.rsl, self.lam, 1.0 / self.lam)
            out = {log2: (None, b) for log2, b in best.items()}
            self.intra_stats.append(st)
        else:
            for log2, g in sorted(self.intra_parts.items(), reverse=True):
                order = intra_modes(hv.h, self.S, self.bd, log2, base, self.stride, g["d_nb"].data_ptr(), g["d_jobs"].data_ptr(), len(g["jobs"]), g["ictx"], self.rsl)
                best, st = intra_rd(hv.h, self.S, self.bd, log2, base, self.stride, g["d_nb"].data_ptr(), g["jobs"], order, g["ictx"], g["ctu"], self.d_states.data_ptr(),
                                    self.quant[log2 - 2], self.lam, 1.0 / self.lam, g["d_rec"].data_ptr())
                st.launches += 1      # the 35-mode stage
                out[log2] = (order, best)
                self.intra_stats.append(st)
        self.intra_results = out
        return out

    def _replayed(self, key, fn):
        """run a FIXED sequence of launches (same kernels, same device buffers every picture: the job tables that depend on the decisions are made on the
        device) -- the first time as it is (it allocates), the second time recorded into a HIP graph, from then on as one graph launch: a picture's ~70
        launches after its searches cost their issuing thread ~100 us each with 8 pictures in flight (profiles/r04/inflight8_timeline.txt)"""
        state = self._graphs.get(key)
        if not self.use_graphs or state is None:
            fn()
            self._graphs[key] = False
        else:
            if state is False:
                state = self._graphs[key] = self.hv.graph_capture(fn)
            self.hv.graph_launch(state)

    def _stages(self):
        """the stages of STAGES this picture was made with, in step()'s order"""
        return [s for s in STAGES if _on(s.option, getattr(self, s.option))]

    def _forget(self):
        """a step has run (or is about to be queued): nothing downloaded from the step before stands, of the picture or of its band views"""
        self._cache.clear()
        for v in getattr(self, "_views", ()):
            v._cache.clear()

    def step(self):
        self.phase_planes()
        if self.temporal_mvp:
            # the candidates before the searches that read them, on the same stream; the table is the context's only while this picture's walk runs
            self.temporal_launch()
            self.hv.search_temporal_d(self._d_temporal, len(self.pus))
            try:
                res, field, stats = self.search()
            finally:
                self.hv.search_temporal_d(None, 0)
        else:
            res, field, stats = self.search()
        if self.intra_parts:
            # (running this on a second context / stream beside the searches -- it reads nothing they decide -- was measured: one picture alone 15.7 -> 15.5 ms, but
            # 294 -> 268 / 383 -> 237 pictures/s with 8 / 16 in flight: a second issuing thread per picture costs more than the overlap gives)
            self.intra_decisions()
        self._forget()
        if self.pu_modes:
            self.pu_candidates(res)
        if self.search_on_device:
            # everything after the searches is a FIXED sequence of launches over device-resident tables (the decided field never leaves the device, the decisions
            # between the launches are kernels): recorded once into a HIP graph, one launch per picture, one wait at the end
            stages = [getattr(self, s.launch) for s in self._stages() if not (s.option == "col" and self.temporal_mvp)]      # (it ran before the searches)
            if self.sao:
                trees = lambda: (self.sao_filter_inputs(field), self.sao_loop_filter())
            elif self.tree_rates:      # (the chroma reconstruction is the tree decision's own: chroma_chain, which codes chroma at depth 0 always, does not run)
                trees = self.tree_and_filter_on_device
            else:
                trees = lambda: (self.tree_and_filter_on_device(), self.chroma_chain(field))
            self._replayed("after the searches", lambda: (self.merge_candidates(field), self.predict(field), trees(), [launch() for launch in stages]))
            self.rqt_stats = RqtStats()
            self.rqt_stats.launches, self.rqt_stats.candidates = self.rqt_plan["launches"], 5 * len(self.units)
        else:
            self._replayed("merge + predict", lambda: (self.merge_candidates(field), self.predict(field)))
            decisions, _ = self.tu_chain(field, predicted=True)
            self._replayed("chroma", lambda: self.chroma_chain(field))
            self.cells = self.block_cells(field, decisions)
            self.loop_filter(self.cells)
        self.hv.sync()
        return res, field, stats

    # ---- round 5: the PRODUCER's half of CTU-row bands (turing/TaskDeblock.cpp:151-167: a picture's rows are deblocked, padded and published while the rows below are
    # still being encoded; the consumer's half is havoc_mi355x_search_gate) ---------------------------------------------------------------------------------------
    def _band_views(self, band_ctu_rows, side):
        """the picture's units cut into bands of whole CTU rows: per band a shallow copy of this object that owns the band's units, job tables and buffers and shares the
        picture's planes, field and block structure; its launches go to `side` (a Havoc context on a stream of another priority than the searches')"""
        key = (band_ctu_rows, id(side))
        if getattr(self, "_views_key", None) != key:
            rows = band_ctu_rows * 64
            views = []
            for y0 in range(0, self.H, rows):
                # the picture as its constructor left it -- planes, field, snapshots, block structure: shared -- without anything built or downloaded since (plans,
                # job tables, graphs, results: a view makes its own for its units)
                v = object.__new__(type(self))
                v.__dict__.update({name: self.__dict__[name] for name in self._constructed})
                v.hv, v._graphs, v.use_graphs, v._cache = side, {}, True, {}
                v.units = self.units[(self.units["y0"] >= y0) & (self.units["y0"] < y0 + rows)]
                v.band_span = (y0, min(self.H, y0 + rows))
                views.append(v)
            self._views, self._views_key = views, key
        return self._views

    def band_rows(self, band_ctu_rows):
        """[first, last) luma rows of the bands step_banded cuts the picture into"""
        rows = band_ctu_rows * 64
        return [(y0, min(self.H, y0 + rows)) for y0 in range(0, self.H, rows)]

    def step_banded(self, side, band_ctu_rows=4, rows_final=None, on_band=None, before_band=None, on_queued=None, make_phase_planes=True, wait=True):
        """step() with everything after the searches done BAND BY BAND while the rows below are still searched: the search kernel is launched on this picture's stream
        and nothing waits for it on the host; on `side` (a Havoc context on a stream of ANOTHER PRIORITY, so that it has its own hardware queue) every band of
        band_ctu_rows CTU rows is queued behind a launch that ends when the band's rows and the row below them are searched (havoc_mi355x_search_wait_rows; the merge
        candidate below-left of a unit lies in the next CTU row): merge candidates, prediction, transform trees, chroma, then the band's block structure, boundary
        strengths, deblocking (its own edges and the edge on its top: the three rows above it change once more) and padding.  rows_final (optional int32 device tensor
        of 1): raised after every band to the number of luma rows of the reconstruction that are final, padding included -- what a dependent picture's search_gate can be
        built on (after the filtering of its taps' rows).  on_band(b, final_rows) (optional) is called when band b's launches are queued: what it queues on `side`
        runs when the band is final (hand the rows on to a dependent picture: tests/test_step_banded.py); before_band(b) is called before band b's launches are queued
        (what it queues on `side` runs before them: bring in the rows of the references the band reads); on_queued() when everything of the picture is queued and
        nothing has been waited for.  make_phase_planes = False: the fractional planes of the references are somebody else's business (a pipeline whose follow steps make
        them band by band: a whole-plane pass here would race with those).  wait = False: nothing is waited for and nothing downloaded -- the call only queues (the intra
        candidates, whose call is synchronous, are then left out); the caller orders what follows with events.  Same results as step(), returned the same way."""
        hv, torch, W, H = self.hv, self.torch, self.W, self.H
        if not self.search_on_device:
            raise ValueError("step_banded needs the device search")
        if self.residual_rates:
            raise ValueError("step_banded does not price residuals with CABAC rates: use step() with residual_rates=True")
        if self.tree_rates:
            raise ValueError("step_banded does not price transform trees with CABAC rates: use step() with tree_rates=True")
        for s in self._stages():
            if s.banded is not None:
                raise ValueError(s.banded)
        if self.sao:
            # SAO of band b reads the deblocked rows of band b + 1 (turing/TaskSao.cpp:46-56): not built
            raise ValueError("step_banded does not run SAO: use step() with sao=True")
        views = self._band_views(band_ctu_rows, side)
        self._forget()
        if make_phase_planes:
            self.phase_planes()
        if not hasattr(self, "_dsearch"):
            n = len(self.pus)
            self._dsearch = dict(pus=self._pus_table(), first=hv.up(np.ascontiguousarray(self.ctu_first, np.int32)),
                                 out=hv.zeros(2 * n * RESULT_DT.itemsize, np.uint8), bi=hv.zeros(2 * n * RESULT_DT.itemsize, np.uint8),
                                 work=hv.zeros((self.hmod.search_workspace(W, H) + 3) // 4, np.int32), gave_up=hv.zeros(1, np.int32))
        D = self._dsearch
        with torch.cuda.stream(hv.tstream):
            D["work"].zero_()      # (the rows' progress counters of the previous picture: gone before anything on `side` can read them)
            D["gave_up"].zero_()
            if rows_final is not None:
                rows_final.zero_()
            cleared = torch.cuda.Event()
            cleared.record(hv.tstream)
        pe, o = self.pe, self.origin
        hv.search_picture_uni_d(self.S, self.params, self.mvp_rate, self.d_pic, o, self.stride, self.d_pic, (pe + o, 2 * pe + o), self.stride, self.d_phase, pe, (o, 16 * pe + o),
                                D["pus"], D["first"], self.cx, self.cy, len(self.pus), D["out"], D["bi"], self.d_field, D["work"])
        side.tstream.wait_event(cleared)
        none = side.zeros(4, np.int32).view(-1, 4)[:0]
        side.block_cells_d(W, H, self.qp, 0, self.d_field, none, none, self.d_cells)      # blank cells, once; the bands add theirs
        bstride = self.region_stride
        half = (H // 2) * (W // 2)
        for b, v in enumerate(views):
            y0, y1 = v.band_span
            last = b == len(views) - 1
            if before_band is not None:
                before_band(b)

            def band(v=v, b=b, y0=y0, y1=y1, last=last):
                side.search_wait_rows(D["work"], W, H, min(self.cy - 1, (y1 - 1) // 64 + 1), D["gave_up"])
                v.merge_candidates(None)
                v.predict(None)
                P = v.tree_decisions()
                v.chroma_chain(None)
                side.block_cells_add_d(W, H, self.qp, 0, self.d_field, P["d_units"].view(-1, 4), P["d_out"], self.d_cells)
                side.derive_bs_d(self.d_cells, W // 4, W, H, self.d_data, self.d_bs)
                side.deblock_d(self.bd, self.recon, self.origin + y0 * self.stride, self.stride, self.d_chroma, (y0 // 2) * (W // 2), half + (y0 // 2) * (W // 2), W // 2, W, y1 - y0,
                               self.d_data[(y0 // 8) * bstride:], self.d_bs[(y0 // 8) * bstride:])
                lo = max(0, y0 - 8)
                side.pad_block_d(self.recon, self.origin + lo * self.stride, W, y1 - lo, self.stride, self.PAD, top=b == 0, bottom=last)

            # a band's ~170 launches are the same every picture (its job tables are made on the device): one graph launch from the third picture on -- with eight pictures
            # in flight a launch costs its issuing thread ~100 us (the plain form ran one 1080p sequence at 45 pictures/s instead of 108)
            v._replayed("band", band)
            final = H + self.PAD if last else y1 - 4
            if rows_final is not None:
                with torch.cuda.stream(side.tstream):
                    rows_final.fill_(final)
            if on_band is not None:
                on_band(b, final)
        if on_queued is not None:
            on_queued()
        if not wait:
            return None      # the caller MUST call check_banded() after its own synchronisation: a wait that gave up leaves a wrong reconstruction and no error
        if self.intra_parts:
            self.intra_decisions()
        hv.sync()
        side.sync()
        self.check_banded()
        res = hv.down(D["out"], np.uint8).view(RESULT_DT)
        self.bi_results = hv.down(D["bi"], np.uint8).view(RESULT_DT)
        field = hv.down(self.d_field, np.int16).reshape(2, (H + 3) // 4, (W + 3) // 4, 2)
        return res, field, None

    def check_banded(self):
        """after step_banded (wait=False: after the caller's own synchronisation of both streams): raises if a device-side wait on the search's progress gave up (a side
        stream sharing a hardware queue with the search it waits for, ~4-8 s) -- the band's launches then ran on unfinished rows"""
        D = getattr(self, "_dsearch", None)
        if D is None:
            return
        if int(self.hv.down(D["gave_up"], np.int32)[0]) or int(self.hv.down(D["work"], np.int32)[-1]):
            raise RuntimeError("step_banded: a wait on the search's progress gave up; the picture's reconstruction is not to be used")

    def results(self):
        """what the TU chain left on the device, as numpy (per group): coefficients, levels, flags, SSDs; and the reconstruction; with pu_modes=True a third entry,
        dict(pu_modes=self.pu_decisions), with cu_close=True also cu_close=self.cu_decisions, with cqt=True also cqt=self.cqt_decisions, with unit_trees=True also
        unit_trees=self.unit_tree_decisions()"""
        hv = self.hv
        out = [dict(log2=g["log2"], coef=hv.down(g["coef"], np.int16), level=hv.down(g["level"], np.int16), cbf=hv.down(g["cbf"], np.int32),
                    ssd=hv.down(g["ssd"], np.uint32)) for g in self.groups]
        if self.pu_modes:
            extra = {}
            for s in self._stages():
                if s.extra is not None:
                    value = getattr(self, s.extra)
                    extra[s.option] = value() if callable(value) else value      # (unit_tree_decisions is a method: it takes planes=)
            return out, hv.down(self.recon, self.dt), extra
        return out, hv.down(self.recon, self.dt)
