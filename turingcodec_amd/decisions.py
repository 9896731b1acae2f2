"""Host-side binding of libhavoc_search.so's PICTURE client (turingcodec_amd/search/picture_search.cpp): a whole picture's
uni-directional motion searches in wavefront order with predictors derived from earlier decisions (search/picture_order.hpp).

Plain ctypes over raw device pointers and a havoc_mi355x context handle, so that the same binding drives the real library (bench.py,
-m gpu tests) and the CPU stand-in device of the host-logic tests.  There is no CPU path here: the library it loads launches kernels.
"""
import ctypes as C
import os

import numpy as np

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
    from . import workload
    q = np.zeros((4, 4), np.int32)
    for log2 in (2, 3, 4, 5):
        qs, qshift, _ = workload.quant_params(qp, log2, bit_depth, False)
        inv, dshift = workload.dequant_params(qp, log2, bit_depth)
        q[log2 - 2] = (qs, qshift, inv, dshift)
    return q


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
        if merge_lists is not None and (not commit or motion is None):
            raise ValueError("merge_lists=max_cand derives the committed picture's merge candidate lists: it needs commit=True and motion=(poc, ref_poc0, ref_poc1)")
        if motion is not None and not commit:
            raise ValueError("motion=(poc, ref_poc0, ref_poc1) makes the collocated motion store of the committed picture: it needs commit=True")
        if merge_lists is not None:
            if isinstance(merge_lists, bool) or int(merge_lists) != merge_lists or not 1 <= int(merge_lists) <= 5:
                raise ValueError("merge_lists must be the number of merge candidates, 1..5")
            if col is not None and "target_poc" in col and tuple(int(v) for v in col["target_poc"]) != tuple(int(v) for v in tuple(motion)[1:3]):
                raise ValueError("merge_lists: col['target_poc'] differs from motion's two references (the temporal candidates were scaled towards other pictures)")
        if col is not None and not search_on_device:
            raise ValueError("col= needs the device route (search_on_device=True)")
        if temporal_mvp and col is None:
            raise ValueError("temporal_mvp=True feeds the temporal candidates of col= into the search walk's predictors: it needs col=")
        if finish and not commit:
            raise ValueError("finish=True deblocks and pads the committed picture: it needs commit=True")
        if commit and not (unit_trees and cqt):
            raise ValueError("commit=True commits the quadtree decided over the searched units into one picture: it needs unit_trees=True and cqt=True")
        if unit_trees and not search_on_device:
            raise ValueError("unit_trees=True needs the device route (search_on_device=True)")
        if unit_trees and not (tree_rates and pu_modes and cu_close):
            raise ValueError("unit_trees=True gives every searched unit the tree of its winning prediction and closes it: it needs tree_rates=True, pu_modes=True "
                             "and cu_close=True")
        if unit_trees and (width % 8 or height % 8):
            raise ValueError("unit_trees=True needs a width and a height that are multiples of 8 (the unit prediction planes are addressed in 8-byte pieces)")
        if cqt and not search_on_device:
            raise ValueError("cqt=True needs the device route (search_on_device=True)")
        if cqt and not cu_close:
            raise ValueError("cqt=True decides the coding quadtree over closed coding units: it needs cu_close=True")
        if cqt and (width % 8 or height % 8):
            raise ValueError("cqt=True needs a width and a height that are multiples of the minimum coding block size, 8")
        if cu_close and not search_on_device:
            raise ValueError("cu_close=True needs the device route (search_on_device=True)")
        if cu_close and not (tree_rates and pu_modes):
            raise ValueError("cu_close=True closes a unit over its tree's and its prediction unit's CABAC bits: it needs tree_rates=True and pu_modes=True")
        if pu_modes and not search_on_device:
            raise ValueError("pu_modes=True needs the device route (search_on_device=True)")
        if sao and not search_on_device:
            raise ValueError("sao=True needs the device route (search_on_device=True)")
        if residual_rates and not search_on_device:
            raise ValueError("residual_rates=True needs the device route (search_on_device=True)")
        if tree_rates and not search_on_device:
            raise ValueError("tree_rates=True needs the device route (search_on_device=True)")
        if tree_rates and residual_rates:
            raise ValueError("tree_rates=True prices the whole transform tree, residuals included: not together with residual_rates=True")
        if tree_rates and sao:
            raise ValueError("tree_rates=True together with sao=True is not built")
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
            m = len(x0)
            qs, qshift, _ = workload.quant_params(qp, log2, bit_depth, False)
            inv, dshift = workload.dequant_params(qp, log2, bit_depth)
            fj = np.zeros((m, 4), np.int32)
            fj[:, 0] = np.arange(m) * nn * nn
            fj[:, 1] = fj[:, 3] = (y0 + self.PAD) * self.stride + x0 + self.PAD
            fj[:, 2] = y0 * width + x0
            jobs = np.zeros(m, hmod.RDOQ_JOB_DT)
            jobs["dst_off"] = jobs["src_off"] = fj[:, 0]
            jobs["quant_scale"], jobs["quant_shift"], jobs["inv_scale"] = qs, qshift, inv
            jobs["lambda_q16"], jobs["sdh_factor"] = hmod.rdoq_lambda(lam, inv)
            jobs["sdh"] = 1
            jobs["ctx_index"] = (y0 // 64) * self.cx + x0 // 64
            with torch.cuda.stream(hv.tstream):
                d_rj = torch.from_numpy(jobs.view(np.uint8).reshape(-1)).to(hv.device)
            self.groups.append(dict(log2=log2, nn=nn, x0=x0, y0=y0, m=m, inv=inv, dshift=dshift, d_fj=hv.up(fj), d_rj=d_rj,
                                    pj=np.zeros((m, 8), np.int32), d_pj=hv.zeros(m * 8, np.int32), coef=hv.zeros(m * nn * nn, np.int16),
                                    level=hv.zeros(m * nn * nn, np.int16), cbf=hv.zeros(m, np.int32), ssd=hv.zeros(m, np.uint32),
                                    work=hv.rdoq_workspace(m)))
        srng = np.random.default_rng(seed + 7919)
        base = srng.integers(4, 100, 128)
        self.rdoq_states = np.clip(base[None, :] + srng.integers(-6, 7, (self.cx * self.cy, 128)), 0, 125).astype(np.uint8)
        self.d_states = hv.up(self.rdoq_states.reshape(-1))
        if tree_rates:      # the contexts outside the 128-byte snapshot (HAVOC_INTRA_SYNTAX_CTX_*: split_transform_flag's), per CTU, seeded the same way
            yrng = np.random.default_rng(seed + 7927)
            self.syntax_states = np.clip(yrng.integers(4, 100, 4)[None, :] + yrng.integers(-6, 7, (self.cx * self.cy, 4)), 0, 125).astype(np.uint8)
            self.d_syntax_states = hv.up(self.syntax_states.reshape(-1))
        if pu_modes:        # prediction_unit()'s contexts (HAVOC_PU_SYNTAX_CTX_*), per CTU, seeded the same way
            prng = np.random.default_rng(seed + 7933)
            self.pu_syntax_states = np.clip(prng.integers(4, 100, hmod.PU_SYNTAX_CTX_BYTES)[None, :] +
                                            prng.integers(-6, 7, (self.cx * self.cy, hmod.PU_SYNTAX_CTX_BYTES)), 0, 125).astype(np.uint8)
            self.d_pu_syntax_states = hv.up(self.pu_syntax_states.reshape(-1))
        if cu_close:        # coding_unit()'s contexts (HAVOC_CU_SYNTAX_CTX_*), per CTU, seeded the same way
            crng = np.random.default_rng(seed + 7937)
            self.cu_syntax_states = np.clip(crng.integers(4, 100, hmod.CU_SYNTAX_CTX_BYTES)[None, :] +
                                            crng.integers(-6, 7, (self.cx * self.cy, hmod.CU_SYNTAX_CTX_BYTES)), 0, 125).astype(np.uint8)
            self.d_cu_syntax_states = hv.up(self.cu_syntax_states.reshape(-1))
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
        if finish:          # the decided picture's block structure (havoc.CELL_DT per 4x4 cell) and the loop filter's edge data on the region grid (as d_data / d_bs)
            regions = ((width + 63) // 64 * 8 + 1) * ((height + 63) // 64 * 8 + 1)
            self.cqt_block = hv.zeros((height // 4) * (width // 4) * hmod.CELL_DT.itemsize, np.uint8)
            self.cqt_data, self.cqt_bs = hv.zeros(regions, np.uint8), hv.zeros(regions, np.uint8)     # (data: int8 values)
        if self.motion is not None:     # the decided picture's collocated motion store: havoc.COL_CELL_DT per 16x16 luma samples, dense rows
            if len(self.motion) != 3:
                raise ValueError("motion must be (poc, ref_poc0, ref_poc1)")
            self.cqt_store = hv.zeros(((height + 15) // 16) * ((width + 15) // 16) * hmod.COL_CELL_DT.itemsize, np.uint8)
        if self.col is not None:        # the units' table on the device (as the search's own copy of it is laid out) and a record per (unit, list)
            missing = {"store", "col_poc", "cur_poc", "target_poc", "all_backwards", "collocated_from_l0"} ^ set(self.col)
            if missing:
                raise ValueError("col= takes exactly store, col_poc, cur_poc, target_poc, all_backwards, collocated_from_l0: %s" % sorted(missing))
            c = self.col
            self._temporal_params = hmod.temporal_params(width, height, self.CQT_CTB_LOG2, c["col_poc"], c["cur_poc"], c["target_poc"], c["all_backwards"],
                                                         c["collocated_from_l0"])
            self._d_temporal_pus = hv.up(np.ascontiguousarray(self.pus).view(np.uint8).reshape(-1))
            self._d_temporal = hv.zeros(max(1, 2 * len(self.pus)) * hmod.TEMPORAL_CAND_DT.itemsize, np.uint8)
        if self.merge_lists is not None:    # a record per searched unit; the units' table as the temporal candidates read it (shared with col= where both are given)
            self._merge_params = hmod.merge_params(width, height, self.CQT_CTB_LOG2, self.CQT_MIN_CB_LOG2, self.merge_lists, self.motion[1:3])
            self._d_merge_pus = self._d_temporal_pus if self.col is not None else hv.up(np.ascontiguousarray(self.pus).view(np.uint8).reshape(-1))
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
        hv.sync()

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
        self._merge = None

    @property
    def merge(self):
        """what merge_candidates() left on the device, as numpy: dict(vectors int16 [units, 5, 2 lists, 2], satd [units, 5, 3 planes], cost [units, 5] (Q16),
        best [units])"""
        if getattr(self, "_merge", None) is None:
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
            self._merge = dict(vectors=vec, satd=satd, cost=cost, best=best)
        return self._merge

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
        self._pu_decisions = None

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
        if getattr(self, "_pu_decisions", None) is None:
            hv, P, K = self.hv, self._pu_plan(), self.PU_CANDIDATES
            M, at = P["M"], P["first"][:, None] + np.arange(K)[None, :]
            satd = hv.down(P["d_satd"], np.int32).reshape(3, M)
            self._pu_decisions = dict(mode=hv.down(P["d_best"], np.int32), cost=hv.down(P["d_best_cost"], np.int64), costs=hv.down(P["d_cost"], np.int64)[at],
                                      syntax=hv.down(P["d_best_syntax"], np.uint8).reshape(-1, self.hmod.PU_SYNTAX_CTX_BYTES),
                                      rates=hv.down(P["d_rate"], np.int64)[at], satd=np.stack([satd[c][at] for c in range(3)], 2),
                                      jobs=hv.down(P["d_jobs"], np.uint8).view(self.hmod.PU_RATE_JOB_DT)[at])
        return self._pu_decisions

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
        if getattr(self, "_cu_decisions", None) is None:
            hv, Q, hmod = self.hv, self._cu_plan(), self.hmod
            self._cu_decisions = dict(records=hv.down(Q["d_out"], np.uint8).view(hmod.CU_CHOICE_DT).copy(),
                                      cu_syntax=hv.down(Q["d_cu_after"], np.uint8).reshape(-1, hmod.CU_SYNTAX_CTX_BYTES),
                                      pu_syntax=hv.down(Q["d_pu_after"], np.uint8).reshape(-1, hmod.PU_SYNTAX_CTX_BYTES),
                                      pred_ssd=hv.down(Q["d_pred_ssd"], np.int32).reshape(-1, 3), jobs=Q["jobs"], searched=Q["match"])
        return self._cu_decisions

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
        if getattr(self, "_cqt_decisions", None) is None:
            B = self._cqt_plan()
            work = self.hv.down(B["work"], np.int64)        # [CTUs]: the published words; then the row ticket (low half) and the give-up word (high half)
            self._cqt_decisions = dict(node_cu=B["node_cu"], gave_up=bool(work[self.cx * self.cy] >> 32),
                                       **self.hv.cqt_download(B, self.W, self.H, self.CQT_CTB_LOG2, self.CQT_MIN_CB_LOG2))
        return self._cqt_decisions

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
        if getattr(self, "_cqt_commit", None) is None:
            hv, pad, c2 = self.hv, self.PAD, self.PAD // 2
            y = hv.down(self.cqt_recon, self.dt)[:self.n].reshape(-1, self.stride)[pad:pad + self.H, pad:pad + self.W]
            c = hv.down(self.cqt_crecon, self.dt)
            c = np.stack([c[k * self.cpe:k * self.cpe + self.cn].reshape(-1, self.cstride)[c2:c2 + self.H // 2, c2:c2 + self.W // 2] for k in range(2)])
            self._cqt_commit = dict(recon=y.copy(), crecon=c, cells=hv.cqt_cells_download(self.cqt_cells, self.W, self.H, self.CQT_MIN_CB_LOG2))
        return self._cqt_commit

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
        if getattr(self, "_cqt_motion", None) is None:
            self._cqt_motion = self.hv.down(self.cqt_store, np.uint8).view(self.hmod.COL_CELL_DT).reshape((self.H + 15) // 16, (self.W + 15) // 16).copy()
        return self._cqt_motion

    # ---- this picture's temporal candidates from another picture's store (turing/Mvp.h:44-181) --------------------------------------------------------------------
    def temporal_launch(self):
        """the temporal candidate of every unit of self.pus, per list, from col["store"] (dense rows).  It reads nothing this picture's step writes.  One launch;
        asynchronous.  Ordering against the step that writes the store is the caller's (see __init__)"""
        self.hv.temporal_candidates_d(self._temporal_params, self.col["store"], (self.W + 15) // 16, self._d_temporal_pus, len(self.pus), self._d_temporal)

    def temporal_candidates(self):
        """what temporal_launch() left on the device, as numpy: havoc.TEMPORAL_CAND_DT [len(self.pus), 2] (unit, list)"""
        if self.col is None:
            raise ValueError("temporal_candidates: the picture was made without col=")
        if getattr(self, "_temporal", None) is None:
            n = len(self.pus)
            self._temporal = self.hv.down(self._d_temporal, np.uint8)[:2 * n * self.hmod.TEMPORAL_CAND_DT.itemsize].view(self.hmod.TEMPORAL_CAND_DT).reshape(n, 2).copy()
        return self._temporal

    # ---- the committed picture's merge candidate lists (turing/Mvp.h:486-716) -----------------------------------------------------------------------------------
    def cqt_merge_launch(self):
        """behind cqt_commit_launch and, with col=, behind temporal_launch: the merge candidate list of every final coding unit from cqt_cells (the neighbours in their
        final state) and this picture's temporal records, into cqt_merge.  One launch; asynchronous"""
        self.hv.cqt_merge_lists_d(self._merge_params, self.cqt_cells, self._d_merge_pus, len(self.pus), self._d_temporal if self.col is not None else None,
                                  self.cqt_merge)

    def cqt_merge_results(self):
        """what cqt_merge_launch() left on the device, as numpy: havoc.MERGE_LIST_DT [len(self.pus)] -- a final unit's list, n_real and match; any other unit: zero
        bytes with match -1"""
        if self.merge_lists is None:
            raise ValueError("cqt_merge_results: the picture was made without merge_lists=max_cand")
        if getattr(self, "_cqt_merge", None) is None:
            self._cqt_merge = self.hv.cqt_merge_lists_download(self.cqt_merge, len(self.pus))
        return self._cqt_merge

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
        if getattr(self, "_cqt_finish", None) is None:
            hv = self.hv
            c = hv.down(self.cqt_crecon, self.dt)
            self._cqt_finish = dict(recon=hv.down(self.cqt_recon, self.dt)[:self.n].reshape(-1, self.stride).copy(),
                                    crecon=np.stack([c[k * self.cpe:k * self.cpe + self.cn].reshape(-1, self.cstride) for k in range(2)]),
                                    cells=hv.down(self.cqt_block, np.uint8).view(self.hmod.CELL_DT).reshape(self.H // 4, self.W // 4).copy(),
                                    data=hv.down(self.cqt_data, np.int8).copy(), bs=hv.down(self.cqt_bs, np.uint8).copy())
        return self._cqt_finish

    def chroma_chain(self, field):
        """the inter residual of the chroma planes at the decided vectors (turing/Reconstruct.cpp:1274-1286 with cIdx 1, 2): HavocPredUni 4-tap of every unit's
        Cb and Cr block at its list-0 vector (eighth-sample phase = the luma vector's low three bits), then residual + DCT -> Rdoq::runQuantisation (cIdx) ->
        de-quantise + inverse DCT + add -> SSD, one chain per chroma transform size, into the chroma reconstruction planes.  Asynchronous."""
        hv, bd = self.hv, self.bd
        hw = self.W // 2
        self.chroma_predict()
        for g in self.cgroups:
            hv.tu_forward_d(bd, 0, g["log2"], g["coef"], self.d_cpic, self.cstride, self.cpred, hw, g["d_fj"])
            hv.rdoq_d(bd, g["log2"], g["level"], g["coef"], self.d_states, g["d_rj"], g["cbf"], g["work"])
            hv.tu_reconstruct_d(bd, 0, g["log2"], g["inv"], g["dshift"], self.crecon, self.cstride, self.cpred, hw, self.d_cpic, self.cstride, g["level"], g["d_fj"], g["ssd"])

    def chroma_predict(self):
        """the prediction half of chroma_chain alone: every unit's Cb and Cr block at its decided vector into cpred (tree_rates=True: the chroma candidates of both
        depths are evaluated from it)"""
        hv = self.hv
        self._chroma_groups()
        for g in self.cgroups:
            hv.pred_jobs_d(self.layout, self.d_field, 0, g["d_x0"], g["d_y0"], g["log2"] + 1, g["comp"], g["d_dst"], g["d_pj"])
            hv.pred_uni_d(4, self.bd, self.cpred, self.W // 2, self.d_cpic, self.cstride, g["d_pj"].view(-1, 8), g["cn"], g["cn"])

    def _chroma_groups(self):
        """chroma_chain's job tables and buffers per (unit size, component), built once"""
        hv, bd, torch, hmod = self.hv, self.bd, self.torch, self.hmod
        from . import workload
        u = self.units
        hw, hh = self.W // 2, self.H // 2
        if not hasattr(self, "cgroups"):
            self.cgroups = []
            for log2 in (5, 4, 3):
                sel = np.flatnonzero(u["log2_size"] == log2)
                if not len(sel):
                    continue
                cl, cn, m = log2 - 1, 1 << (log2 - 1), len(sel)
                x0, y0 = u["x0"][sel].astype(np.int64) // 2, u["y0"][sel].astype(np.int64) // 2
                qs, qshift, _ = workload.quant_params(self.qp, cl, bd, False)
                inv, dshift = workload.dequant_params(self.qp, cl, bd)
                lq, sf = hmod.rdoq_lambda(self.lam, inv)
                for comp in (1, 2):
                    fj = np.zeros((m, 4), np.int32)
                    fj[:, 0] = np.arange(m) * cn * cn
                    fj[:, 1] = 3 * (comp - 1) * self.cpe + (y0 + self.PAD // 2) * self.cstride + x0 + self.PAD // 2          # source block in d_cpic
                    fj[:, 2] = (comp - 1) * hw * hh + y0 * hw + x0                                                           # prediction block in cpred
                    fj[:, 3] = (comp - 1) * self.cpe + (y0 + self.PAD // 2) * self.cstride + x0 + self.PAD // 2              # reconstruction in crecon
                    jobs = np.zeros(m, hmod.RDOQ_JOB_DT)
                    jobs["dst_off"] = jobs["src_off"] = fj[:, 0]
                    jobs["quant_scale"], jobs["quant_shift"], jobs["inv_scale"], jobs["lambda_q16"], jobs["sdh_factor"] = qs, qshift, inv, lq, sf
                    jobs["sdh"], jobs["c_idx"] = 1, comp
                    jobs["ctx_index"] = (u["y0"][sel] // 64) * self.cx + u["x0"][sel] // 64
                    with torch.cuda.stream(hv.tstream):
                        d_rj = torch.from_numpy(jobs.view(np.uint8).reshape(-1)).to(hv.device)
                    self.cgroups.append(dict(log2=cl, cn=cn, comp=comp, m=m, sel=sel, inv=inv, dshift=dshift, d_fj=hv.up(fj), d_rj=d_rj,
                                             d_x0=hv.up(u["x0"][sel].astype(np.int32)), d_y0=hv.up(u["y0"][sel].astype(np.int32)), d_dst=hv.up(fj[:, 2]),
                                             d_pj=hv.zeros(m * 8, np.int32), coef=hv.zeros(m * cn * cn, np.int16),
                                             level=hv.zeros(m * cn * cn, np.int16), cbf=hv.zeros(m, np.int32), ssd=hv.zeros(m, np.uint32), work=hv.rdoq_workspace(m)))

    def tu_chain(self, field, predicted=False):
        """prediction at the decided vectors, then the residual-quadtree decisions and the reconstruction; returns (decisions, stats)"""
        if not predicted:
            self.predict(field)
        base = self.d_pic.data_ptr()
        self._rqt, st = rqt(self.hv.h, self.S, self.bd, base, self.origin, self.stride, self.pred.data_ptr(), self.W, self.recon.data_ptr(), self.origin,
                                   self.stride, self.d_states.data_ptr(), self.quant, self.lam, 1.0 / self.lam, self.units)
        self.rqt_stats = st
        return self._rqt, st

    # ---- round 4: the transform-tree decision and the block structure on the device -- nothing of the picture's step waits for the host after its searches ----
    def _rqt_plan(self):
        """what havoc_search_rqt builds per call, built ONCE (the units of a picture do not move): per transform size the candidates' job records (depth 0 of every unit
        of that size, then the four depth-1 blocks of every unit of the next larger size, unit by unit), their buffers, and where each unit finds its candidates"""
        hv, hmod, torch = self.hv, self.hmod, self.torch
        from . import workload
        u = self.units
        lists = {s: [] for s in (2, 3, 4, 5)}
        zero_at, one_at = np.zeros(len(u), np.int32), np.zeros(len(u), np.int32)
        for i in range(len(u)):
            L = int(u["log2_size"][i])
            zero_at[i] = len(lists[L])
            lists[L].append((i, 0, 0))
            one_at[i] = len(lists[L - 1])
            lists[L - 1] += [(i, 1, k) for k in range(4)]
        plan = dict(sizes={}, d_units=hv.up(np.ascontiguousarray(u).view(np.int32)), d_zero_at=hv.up(zero_at), d_one_at=hv.up(one_at),
                    d_out=hv.zeros(len(u) * 26, np.int32), table=np.zeros((4, 5), np.uint64), rates=np.zeros(4, np.uint64), launches=0)
        for log2, cand in lists.items():
            m = len(cand)
            if not m:
                continue
            nn = 1 << log2
            area = nn * nn
            c = np.array(cand, np.int64)
            x = u["x0"][c[:, 0]].astype(np.int64) + np.where(c[:, 1] == 1, (c[:, 2] & 1) * nn, 0)
            y = u["y0"][c[:, 0]].astype(np.int64) + np.where(c[:, 1] == 1, (c[:, 2] >> 1) * nn, 0)
            jobs = np.stack([np.arange(m) * area, self.origin + y * self.stride + x, y * self.W + x, np.arange(m) * area], 1).astype(np.int32)
            qs, qshift, inv, dshift = (int(v) for v in self.quant[log2 - 2])
            rj = np.zeros(m, hmod.RDOQ_JOB_DT)
            rj["dst_off"] = rj["src_off"] = jobs[:, 0]
            rj["quant_scale"], rj["quant_shift"], rj["inv_scale"] = qs, qshift, inv
            rj["lambda_q16"], rj["sdh_factor"] = hmod.rdoq_lambda(self.lam, inv)
            rj["sdh"] = 1
            rj["ctx_index"] = u["ctx_index"][c[:, 0]]
            with torch.cuda.stream(hv.tstream):
                d_rj = torch.from_numpy(rj.view(np.uint8).reshape(-1)).to(hv.device)
            g = dict(log2=log2, nn=nn, m=m, inv=inv, dshift=dshift, d_jobs=hv.up(jobs), d_fin=hv.zeros(m * 4, np.int32), d_rj=d_rj,
                     d_sj=hv.up(np.stack([jobs[:, 0], np.full(m, area)], 1).astype(np.int32)), coef=hv.zeros(m * area, np.int16), level=hv.zeros(m * area, np.int16),
                     piece=hv.zeros(m * area, self.dt), work=hv.rdoq_workspace(m), cbf=hv.zeros(m, np.int32), ssd=hv.zeros(m, np.uint32), stats=hv.zeros(2 * m, np.int32),
                     ssd2=hv.zeros(m, np.uint32))
            plan["sizes"][log2] = g
            plan["table"][log2 - 2] = [g["cbf"].data_ptr(), g["ssd"].data_ptr(), g["stats"].data_ptr(), g["d_jobs"].data_ptr(), g["d_fin"].data_ptr()]
            if self.residual_rates:
                # a depth-0 candidate is a job of its own; the four depth-1 candidates of a unit lie one after the other: ONE job that walks them in z-order with the
                # contexts running on, as the reference codes them -- each from the unit's snapshot, like the RDOQ jobs
                lead = np.flatnonzero(c[:, 2] == 0)
                qj = np.zeros(len(lead), hmod.RESIDUAL_RATE_JOB_DT)
                qj["level_off"], qj["rate_index"], qj["ctx_index"] = jobs[lead, 0], lead, u["ctx_index"][c[lead, 0]]
                qj["sdh"], qj["count"] = 1, np.where(c[lead, 1] == 1, 4, 1)
                with torch.cuda.stream(hv.tstream):
                    g["d_qj"] = torch.from_numpy(qj.view(np.uint8).reshape(-1).copy()).to(hv.device)
                    g["rates"] = torch.zeros(m, dtype=torch.int64, device=hv.device)
                g["rate_jobs"] = qj
                plan["table"][log2 - 2, 2] = 0      # (no level statistics: nonzero / sum_abs of the results are 0)
                plan["rates"][log2 - 2] = g["rates"].data_ptr()
            plan["launches"] += 5
        plan["launches"] += 1
        # a block-sized area nobody reads, inside the reconstruction's bottom border (rewritten by the padding that ends the step): where the candidates that lost go
        plan["dump"] = (self.H + self.PAD + 16) * self.stride + self.PAD
        plan["rl_q16"] = int((1.0 / self.lam) * 65536 + 0.5)
        if self.tree_rates:
            self._tree_plan(plan, zero_at, one_at)
        self._filter_buffers()
        return plan

    def _tree_plan(self, plan, zero_at, one_at):
        """tree_rates=True, beside the luma candidates of _rqt_plan: the chroma candidates of both depths per chroma transform size (a unit's depth-0 Cb and Cr block
        of max(L - 1, 2); for L > 3 its four depth-1 Cb blocks, then its four Cr blocks, of L - 2, z-order; an 8x8 unit's one 4x4 block per component serves both
        depths), where each unit finds them, and the tree_rate jobs per (unit size, depth) -- every tree from the unit's snapshot, out_index = 2 * unit + depth"""
        hv, hmod, torch, bd = self.hv, self.hmod, self.torch, self.bd
        from . import workload
        u = self.units
        hw, hh, c2 = self.W // 2, self.H // 2, self.PAD // 2
        clists = {s: [] for s in (2, 3, 4)}
        chroma_at = np.zeros(len(u), hmod.RQT_CHROMA_AT_DT)
        for i in range(len(u)):
            L = int(u["log2_size"][i])
            c0 = max(L - 1, 2)
            chroma_at[i]["cb_zero"], chroma_at[i]["cr_zero"] = len(clists[c0]), len(clists[c0]) + 1
            clists[c0] += [(i, 0, 1, 0), (i, 0, 2, 0)]
            if L > 3:
                chroma_at[i]["cb_one"], chroma_at[i]["cr_one"] = len(clists[L - 2]), len(clists[L - 2]) + 4
                clists[L - 2] += [(i, 1, comp, k) for comp in (1, 2) for k in range(4)]
            else:
                chroma_at[i]["cb_one"], chroma_at[i]["cr_one"] = chroma_at[i]["cb_zero"], chroma_at[i]["cr_zero"]
        plan["chroma_at"], plan["d_chroma_at"] = chroma_at, hv.up(np.ascontiguousarray(chroma_at).view(np.int32))
        plan["csizes"], plan["ctable"] = {}, np.zeros((4, 5), np.uint64)
        for cl, cand in clists.items():
            m = len(cand)
            if not m:
                continue
            cn = 1 << cl
            area = cn * cn
            c = np.array(cand, np.int64)
            x = u["x0"][c[:, 0]].astype(np.int64) // 2 + np.where(c[:, 1] == 1, (c[:, 3] & 1) * cn, 0)
            y = u["y0"][c[:, 0]].astype(np.int64) // 2 + np.where(c[:, 1] == 1, (c[:, 3] >> 1) * cn, 0)
            comp = c[:, 2]
            jobs = np.stack([np.arange(m) * area, 3 * (comp - 1) * self.cpe + (y + c2) * self.cstride + x + c2, (comp - 1) * hw * hh + y * hw + x,
                             np.arange(m) * area], 1).astype(np.int32)
            qs, qshift, _ = workload.quant_params(self.qp, cl, bd, False)
            inv, dshift = workload.dequant_params(self.qp, cl, bd)
            rj = np.zeros(m, hmod.RDOQ_JOB_DT)
            rj["dst_off"] = rj["src_off"] = jobs[:, 0]
            rj["quant_scale"], rj["quant_shift"], rj["inv_scale"] = qs, qshift, inv
            rj["lambda_q16"], rj["sdh_factor"] = hmod.rdoq_lambda(self.lam, inv)
            rj["sdh"], rj["c_idx"] = 1, comp
            rj["ctx_index"] = u["ctx_index"][c[:, 0]]
            with torch.cuda.stream(hv.tstream):
                d_rj = torch.from_numpy(rj.view(np.uint8).reshape(-1)).to(hv.device)
            g = dict(log2=cl, nn=cn, m=m, inv=inv, dshift=dshift, cand=c, d_jobs=hv.up(jobs), d_fin=hv.zeros(m * 4, np.int32), d_rj=d_rj, coef=hv.zeros(m * area, np.int16),
                     level=hv.zeros(m * area, np.int16), piece=hv.zeros(m * area, self.dt), work=hv.rdoq_workspace(m), cbf=hv.zeros(m, np.int32), ssd=hv.zeros(m, np.uint32),
                     ssd2=hv.zeros(m, np.uint32))
            plan["csizes"][cl] = g
            plan["ctable"][cl - 2] = [g["cbf"].data_ptr(), g["ssd"].data_ptr(), 0, g["d_jobs"].data_ptr(), g["d_fin"].data_ptr()]
            plan["launches"] += 4
        plan["table"][:, 2] = 0          # (no level statistics on this route: nonzero / sum_abs of the results are 0)
        plan["tree_jobs"] = {}
        for L in (5, 4, 3):
            sel = np.flatnonzero(u["log2_size"] == L)
            if not len(sel):
                continue
            c0, c1 = max(L - 1, 2), max(L - 2, 2)
            for depth in (0, 1):
                tj = np.zeros(len(sel), hmod.TREE_RATE_JOB_DT)
                if depth == 0:
                    tj["luma_off"], tj["cb_off"], tj["cr_off"] = zero_at[sel] << 2 * L, chroma_at["cb_zero"][sel] << 2 * c0, chroma_at["cr_zero"][sel] << 2 * c0
                else:
                    tj["luma_off"], tj["cb_off"], tj["cr_off"] = one_at[sel] << 2 * (L - 1), chroma_at["cb_one"][sel] << 2 * c1, chroma_at["cr_one"][sel] << 2 * c1
                tj["ctx_index"], tj["out_index"], tj["sdh"] = u["ctx_index"][sel], 2 * sel + depth, 1
                tj["flags"] = hmod.TREE_RATE_SPLIT_FLAG_CODED      # MaxTrafoDepth 1, MinTbLog2SizeY 2, MaxTbLog2SizeY 5: coded for every unit of 8 .. 32
                with torch.cuda.stream(hv.tstream):
                    d_tj = torch.from_numpy(tj.view(np.uint8).reshape(-1).copy()).to(hv.device)
                plan["tree_jobs"][L, depth] = dict(jobs=tj, d_jobs=d_tj, luma=L - depth, chroma=c1 if depth else c0)
                plan["launches"] += 1
        with torch.cuda.stream(hv.tstream):
            plan["tree_rate"] = torch.zeros(2 * len(u), dtype=torch.int64, device=hv.device)
        plan["tree_cbf"], plan["d_tree_out"] = hv.zeros(2 * len(u), np.int32), hv.zeros(4 * len(u), np.int32)
        # where the chroma candidates that lost go: inside the chroma reconstruction's bottom border (nothing reads it)
        plan["cdump"] = (hh + c2 + 8) * self.cstride + c2
        plan["launches"] += 4 * len(np.unique(u["log2_size"])) - len(plan["sizes"])      # (chroma prediction: 2 per unit size and component; no level_stats)

    def _filter_buffers(self):
        """the block structure and the loop filter's edge data of the picture (one set per picture, whatever decides its units -- the whole-picture plan or the band views)"""
        if hasattr(self, "d_cells"):
            return
        hv, torch = self.hv, self.torch
        n = ((self.W + 63) // 64 * 8 + 1) * ((self.H + 63) // 64 * 8 + 1)
        with torch.cuda.stream(hv.tstream):
            self.d_data = torch.zeros(n, dtype=torch.int8, device=hv.device)
            self.d_bs = torch.zeros(n, dtype=torch.uint8, device=hv.device)
            self.d_cells = torch.zeros((self.H // 4) * (self.W // 4) * 16, dtype=torch.uint8, device=hv.device)
        self.d_chroma = hv.up(np.full(2 * (self.H // 2) * (self.W // 2), 128 << (self.bd - 8), self.dt))

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
        n64 = (W + 63) // 64 * 8 + 1
        hv.sao_apply_d(bd, 3, W, H, 6, self.deblocked, o, self.cdeblocked, co, self.cpe + co, self.stride, cs, self.recon, o, self.crecon, co, self.cpe + co,
                       self.stride, cs, self.d_sao_decisions, None, self.d_data, n64)
        hv.pad_block_d(self.recon, o, W, H, self.stride, self.PAD)
        hv.pad_block_d(self.crecon, co, W // 2, H // 2, cs, c2)
        hv.pad_block_d(self.crecon, self.cpe + co, W // 2, H // 2, cs, c2)

    @property
    def sao_decisions(self):
        """the SAO decisions of the last sao=True step (SAO_DECISION_DT per 64x64 CTU in raster order): downloaded when asked for"""
        if getattr(self, "_sao_decisions", None) is None:
            self._sao_decisions = self.hv.down(self.d_sao_decisions, np.uint8).view(self.hmod.SAO_DECISION_DT).copy()
        return self._sao_decisions

    def tree_decisions(self):
        """the transform-tree part of tree_and_filter_on_device for self.units; returns the plan (its d_units / d_out are what the block structure is made from)"""
        hv, bd = self.hv, self.bd
        if not hasattr(self, "rqt_plan"):
            self.rqt_plan = self._rqt_plan()
        P = self.rqt_plan
        src = self.d_pic
        if self.tree_rates:
            return self._tree_decisions_three_planes(P)
        for g in P["sizes"].values():
            hv.tu_forward_d(bd, 0, g["log2"], g["coef"], src, self.stride, self.pred, self.W, g["d_jobs"].view(-1, 4))
            hv.rdoq_d(bd, g["log2"], g["level"], g["coef"], self.d_states, g["d_rj"], g["cbf"], g["work"])
            hv.tu_reconstruct_d(bd, 0, g["log2"], g["inv"], g["dshift"], g["piece"], g["nn"], self.pred, self.W, src, self.stride, g["level"], g["d_jobs"].view(-1, 4), g["ssd"])
            if self.residual_rates:
                hv.residual_rate_d(g["log2"], g["level"], self.d_states, g["d_qj"], g["rates"])
            else:
                hv.level_stats_d(g["level"], g["d_sj"], g["m"], g["stats"])
        if self.residual_rates:
            self._rqt_rates = None
            hv.rqt_decide_rated_d(P["d_units"].view(-1, 4), P["d_zero_at"], P["d_one_at"], P["table"], P["rates"], self.origin, self.stride, P["dump"], P["rl_q16"], P["d_out"])
        else:
            hv.rqt_decide_d(P["d_units"].view(-1, 4), P["d_zero_at"], P["d_one_at"], P["table"], self.origin, self.stride, P["dump"], P["rl_q16"], P["d_out"])
        for g in P["sizes"].values():
            hv.tu_reconstruct_d(bd, 0, g["log2"], g["inv"], g["dshift"], self.recon, self.stride, self.pred, self.W, src, self.stride, g["level"], g["d_fin"].view(-1, 4), g["ssd2"])
        return P

    def _tree_decisions_three_planes(self, P):
        """tree_rates=True: chroma prediction; the luma candidates as on the default route; the chroma candidates of both depths per chroma size (residual + DCT ->
        RDOQ with cIdx 1 / 2 from the unit's snapshot -> IQ + IDCT + add -> SSD, into pieces); the whole-tree rate and cbf mask per (unit size, depth); the decision
        over three planes; every candidate reconstructed again -- the chosen trees' luma into recon AND chroma into crecon"""
        hv, bd, src, hw = self.hv, self.bd, self.d_pic, self.W // 2
        self.chroma_predict()
        for g in P["sizes"].values():
            hv.tu_forward_d(bd, 0, g["log2"], g["coef"], src, self.stride, self.pred, self.W, g["d_jobs"].view(-1, 4))
            hv.rdoq_d(bd, g["log2"], g["level"], g["coef"], self.d_states, g["d_rj"], g["cbf"], g["work"])
            hv.tu_reconstruct_d(bd, 0, g["log2"], g["inv"], g["dshift"], g["piece"], g["nn"], self.pred, self.W, src, self.stride, g["level"], g["d_jobs"].view(-1, 4), g["ssd"])
        for g in P["csizes"].values():
            hv.tu_forward_d(bd, 0, g["log2"], g["coef"], self.d_cpic, self.cstride, self.cpred, hw, g["d_jobs"].view(-1, 4))
            hv.rdoq_d(bd, g["log2"], g["level"], g["coef"], self.d_states, g["d_rj"], g["cbf"], g["work"])
            hv.tu_reconstruct_d(bd, 0, g["log2"], g["inv"], g["dshift"], g["piece"], g["nn"], self.cpred, hw, self.d_cpic, self.cstride, g["level"], g["d_jobs"].view(-1, 4),
                                g["ssd"])
        for (L, depth), t in P["tree_jobs"].items():
            hv.tree_rate_d(L, depth, P["sizes"][t["luma"]]["level"], P["csizes"][t["chroma"]]["level"], self.d_states, self.d_syntax_states, t["d_jobs"], P["tree_rate"],
                           P["tree_cbf"])
        self._rqt_rates = self._rqt_tree = None
        hv.rqt_decide_tree_d(P["d_units"].view(-1, 4), P["d_zero_at"], P["d_one_at"], P["table"], P["ctable"], P["d_chroma_at"], P["tree_rate"], P["tree_cbf"], self.origin,
                             self.stride, P["dump"], self.corigin, self.cpe + self.corigin, self.cstride, P["cdump"], P["rl_q16"], P["d_out"], P["d_tree_out"])
        for g in P["sizes"].values():
            hv.tu_reconstruct_d(bd, 0, g["log2"], g["inv"], g["dshift"], self.recon, self.stride, self.pred, self.W, src, self.stride, g["level"], g["d_fin"].view(-1, 4), g["ssd2"])
        for g in P["csizes"].values():
            hv.tu_reconstruct_d(bd, 0, g["log2"], g["inv"], g["dshift"], self.crecon, self.cstride, self.cpred, hw, self.d_cpic, self.cstride, g["level"], g["d_fin"].view(-1, 4),
                                g["ssd2"])
        return P

    # ---- unit_trees=True: the transform tree of EVERY searched unit, made from the residual of its own winning prediction (what reconstructInter runs on after go2) ----
    def _unit_tree_plan(self):
        """unit_trees' tables and buffers, built once, beside rqt_plan (which still makes recon / crecon / cells from self.pred).  The units are self.pus in their own
        order -- 2Nx2N of 64 to 8, overlapping one another as the quadtree search meets them -- so index p means the same unit in pu_decisions, the tree records,
        cu_decisions and the node table.  Their predictions lie in UNIT PREDICTION PLANES: one luma allocation of four W x H planes and one chroma allocation of four
        (Cb, Cr) plane pairs, plane 6 - L for units of size 2^L, a unit's block at its picture position (stride W, W / 2 for chroma): a job of any launch names its
        block by a 32-bit offset, so one base pointer and stride serve a launch that mixes depth-0 blocks of size-L units with depth-1 blocks of size-(L + 1) units.
        Per transform size the luma candidates (depth 0 of every unit of that size up to 32, then the four depth-1 blocks of every unit of the next larger size, 64
        included); per chroma size the Cb / Cr candidates as _tree_plan lays them out; a 64x64 unit contributes its four 32x32 luma and four 16x16 Cb and Cr blocks
        only.  tree_rate jobs per (L, depth): (6, 1) without the flag bit, 5..3 at both depths with it; out_index = 2 * unit + depth.  No final job records."""
        if hasattr(self, "unit_plan"):
            return self.unit_plan
        hv, hmod, torch, bd = self.hv, self.hmod, self.torch, self.bd
        from . import workload
        P = self._pu_plan()
        pus, n = self.pus, len(self.pus)
        W, hw, hh, c2 = self.W, self.W // 2, self.H // 2, self.PAD // 2
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
        lists, clists = {s: [] for s in (2, 3, 4, 5)}, {s: [] for s in (2, 3, 4)}
        zero_at, one_at, chroma_at = np.full(n, -1, np.int32), np.zeros(n, np.int32), np.zeros(n, hmod.RQT_CHROMA_AT_DT)
        for i in range(n):
            L, a = int(uL[i]), chroma_at[i]
            if L < 6:
                zero_at[i] = len(lists[L])
                lists[L].append((i, 0, 0))
                c0 = max(L - 1, 2)
                a["cb_zero"], a["cr_zero"] = len(clists[c0]), len(clists[c0]) + 1
                clists[c0] += [(i, 0, 1, 0), (i, 0, 2, 0)]
            else:       # a 64x64 unit has no depth-0 candidate in any plane (its split is inferred)
                a["cb_zero"], a["cr_zero"] = -1, -1
            one_at[i] = len(lists[L - 1])
            lists[L - 1] += [(i, 1, k) for k in range(4)]
            if L > 3:
                a["cb_one"], a["cr_one"] = len(clists[L - 2]), len(clists[L - 2]) + 4
                clists[L - 2] += [(i, 1, comp, k) for comp in (1, 2) for k in range(4)]
            else:
                a["cb_one"], a["cr_one"] = a["cb_zero"], a["cr_zero"]
        plan = dict(units=u, select_jobs=sel, zero_at=zero_at, one_at=one_at, chroma_at=chroma_at, sizes={}, csizes={}, tree_jobs={}, table=np.zeros((4, 5), np.uint64),
                    ctable=np.zeros((4, 5), np.uint64), rl_q16=int((1.0 / self.lam) * 65536 + 0.5), launches=2,
                    pred=hv.zeros(4 * ypl, self.dt), cpred=hv.zeros(8 * cpl, self.dt), d_units=hv.up(np.ascontiguousarray(u).view(np.int32)), d_zero_at=hv.up(zero_at),
                    d_one_at=hv.up(one_at), d_chroma_at=hv.up(np.ascontiguousarray(chroma_at).view(np.int32)), d_out=hv.zeros(n * 26, np.int32),
                    d_tree_out=hv.zeros(4 * n, np.int32), tree_cbf=hv.zeros(2 * n, np.int32), d_unit_cand=hv.zeros(n, np.int32))

        def group(log2, jobs, ctx, c_idx):
            m, area = len(jobs), 1 << 2 * log2
            qs, qshift, _ = workload.quant_params(self.qp, log2, bd, False)
            inv, dshift = workload.dequant_params(self.qp, log2, bd)
            if c_idx is None:
                qs, qshift, inv, dshift = (int(v) for v in self.quant[log2 - 2])
            rj = np.zeros(m, hmod.RDOQ_JOB_DT)
            rj["dst_off"] = rj["src_off"] = jobs[:, 0]
            rj["quant_scale"], rj["quant_shift"], rj["inv_scale"] = qs, qshift, inv
            rj["lambda_q16"], rj["sdh_factor"] = hmod.rdoq_lambda(self.lam, inv)
            rj["sdh"], rj["ctx_index"] = 1, ctx
            if c_idx is not None:
                rj["c_idx"] = c_idx
            with torch.cuda.stream(hv.tstream):
                d_rj = torch.from_numpy(rj.view(np.uint8).reshape(-1)).to(hv.device)
            return dict(log2=log2, nn=1 << log2, m=m, inv=inv, dshift=dshift, jobs=jobs, d_jobs=hv.up(jobs), d_rj=d_rj, coef=hv.zeros(m * area, np.int16),
                        level=hv.zeros(m * area, np.int16), piece=hv.zeros(m * area, self.dt), work=hv.rdoq_workspace(m), cbf=hv.zeros(m, np.int32),
                        ssd=hv.zeros(m, np.uint32))

        for log2, cand in lists.items():
            if not cand:
                continue
            nn, c = 1 << log2, np.array(cand, np.int64)
            x = ux[c[:, 0]] + np.where(c[:, 1] == 1, (c[:, 2] & 1) * nn, 0)
            y = uy[c[:, 0]] + np.where(c[:, 1] == 1, (c[:, 2] >> 1) * nn, 0)
            at = np.arange(len(c)) << 2 * log2
            jobs = np.stack([at, self.origin + y * self.stride + x, uplane[c[:, 0]] * ypl + y * W + x, at], 1).astype(np.int32)
            g = plan["sizes"][log2] = group(log2, jobs, u["ctx_index"][c[:, 0]], None)
            plan["table"][log2 - 2] = [g["cbf"].data_ptr(), g["ssd"].data_ptr(), 0, g["d_jobs"].data_ptr(), 0]
            plan["launches"] += 3
        for cl, cand in clists.items():
            if not cand:
                continue
            cn, c = 1 << cl, np.array(cand, np.int64)
            x = ux[c[:, 0]] // 2 + np.where(c[:, 1] == 1, (c[:, 3] & 1) * cn, 0)
            y = uy[c[:, 0]] // 2 + np.where(c[:, 1] == 1, (c[:, 3] >> 1) * cn, 0)
            comp, at = c[:, 2], np.arange(len(c)) << 2 * cl
            jobs = np.stack([at, 3 * (comp - 1) * self.cpe + (y + c2) * self.cstride + x + c2, (2 * uplane[c[:, 0]] + comp - 1) * cpl + y * hw + x, at], 1).astype(np.int32)
            g = plan["csizes"][cl] = group(cl, jobs, u["ctx_index"][c[:, 0]], comp)
            g["cand"] = c
            plan["ctable"][cl - 2] = [g["cbf"].data_ptr(), g["ssd"].data_ptr(), 0, g["d_jobs"].data_ptr(), 0]
            plan["launches"] += 3
        for L in (6, 5, 4, 3):
            at = np.flatnonzero(uL == L)
            if not len(at):
                continue
            c0, c1 = max(L - 1, 2), max(L - 2, 2)
            for depth in ((1,) if L == 6 else (0, 1)):
                tj = np.zeros(len(at), hmod.TREE_RATE_JOB_DT)
                if depth == 0:
                    tj["luma_off"], tj["cb_off"], tj["cr_off"] = zero_at[at] << 2 * L, chroma_at["cb_zero"][at] << 2 * c0, chroma_at["cr_zero"][at] << 2 * c0
                else:
                    tj["luma_off"], tj["cb_off"], tj["cr_off"] = one_at[at] << 2 * (L - 1), chroma_at["cb_one"][at] << 2 * c1, chroma_at["cr_one"][at] << 2 * c1
                tj["ctx_index"], tj["out_index"], tj["sdh"] = u["ctx_index"][at], 2 * at + depth, 1
                tj["flags"] = hmod.TREE_RATE_SPLIT_FLAG_CODED if L < 6 else 0      # above MaxTbLog2SizeY the split is inferred: no bin
                with torch.cuda.stream(hv.tstream):
                    d_tj = torch.from_numpy(tj.view(np.uint8).reshape(-1).copy()).to(hv.device)
                plan["tree_jobs"][L, depth] = dict(jobs=tj, d_jobs=d_tj, luma=L - depth, chroma=c1 if depth else c0)
                plan["launches"] += 1
        with torch.cuda.stream(hv.tstream):
            plan["tree_rate"] = torch.zeros(2 * n, dtype=torch.int64, device=hv.device)
            plan["d_unit_rate"] = torch.zeros(n, dtype=torch.int64, device=hv.device)
            plan["d_select_jobs"] = torch.from_numpy(sel.view(np.uint8).reshape(-1).copy()).to(hv.device)
        self.unit_plan = plan
        return plan

    def unit_tree_launches(self):
        """behind pu_mode_launches: the winner's prediction of every searched unit into the unit prediction planes with its rate (one launch for every size), then per
        transform size the luma candidates and per chroma size the Cb / Cr candidates (residual + DCT -> RDOQ from the CTU's snapshot -> IQ + IDCT + add -> SSD, into
        pieces), the whole-tree rate and cbf mask per (unit size, depth), and the decision over three planes without final records.  Asynchronous"""
        hv, bd, P, U = self.hv, self.bd, self._pu_plan(), self._unit_tree_plan()
        hw = self.W // 2
        hv.unit_pred_select_d(bd, P["d_cand_y"], P["d_cand_c"], U["pred"], self.W, U["cpred"], hw, P["d_first"], P["d_best"], P["d_rate"], U["d_select_jobs"],
                              U["d_unit_rate"], U["d_unit_cand"])
        for groups, src, stride, pred, pstride in ((U["sizes"], self.d_pic, self.stride, U["pred"], self.W), (U["csizes"], self.d_cpic, self.cstride, U["cpred"], hw)):
            for g in groups.values():
                hv.tu_forward_d(bd, 0, g["log2"], g["coef"], src, stride, pred, pstride, g["d_jobs"].view(-1, 4))
                hv.rdoq_d(bd, g["log2"], g["level"], g["coef"], self.d_states, g["d_rj"], g["cbf"], g["work"])
                hv.tu_reconstruct_d(bd, 0, g["log2"], g["inv"], g["dshift"], g["piece"], g["nn"], pred, pstride, src, stride, g["level"], g["d_jobs"].view(-1, 4), g["ssd"])
        for (L, depth), t in U["tree_jobs"].items():
            hv.tree_rate_d(L, depth, U["sizes"][t["luma"]]["level"], U["csizes"][t["chroma"]]["level"], self.d_states, self.d_syntax_states, t["d_jobs"], U["tree_rate"],
                           U["tree_cbf"])
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
        if getattr(self, "_unit_tree_decisions", None) is None:
            with self.torch.cuda.stream(hv.tstream):
                rate, unit_rate = U["tree_rate"].cpu().numpy().reshape(-1, 2), U["d_unit_rate"].cpu().numpy()
            self._unit_tree_decisions = dict(units=U["units"], choice=hv.down(U["d_out"], np.int32).view(RQT_RESULT_DT).copy(),
                                             tree_choice=hv.down(U["d_tree_out"], np.int32).view(hmod.RQT_TREE_RESULT_DT).copy(), tree_rate=rate,
                                             tree_cbf=hv.down(U["tree_cbf"], np.int32).view(np.uint32).reshape(-1, 2), unit_rate=unit_rate,
                                             unit_cand=hv.down(U["d_unit_cand"], np.int32))
        if not planes:
            return self._unit_tree_decisions
        return dict(self._unit_tree_decisions, pred=hv.down(U["pred"], self.dt).reshape(4, self.H, self.W),
                    cpred=hv.down(U["cpred"], self.dt).reshape(4, 2, self.H // 2, self.W // 2))

    @property
    def rqt_tree_results(self):
        """tree_rates=True: what the decision over three planes adds per unit (havoc.RQT_TREE_RESULT_DT: both cbf masks, both sums ssdCb + ssdCr): downloaded when
        asked for"""
        if not self.tree_rates:
            raise ValueError("rqt_tree_results: the picture was made without tree_rates=True")
        if getattr(self, "_rqt_tree", None) is None:
            self._rqt_tree = self.hv.down(self.rqt_plan["d_tree_out"], np.int32).view(self.hmod.RQT_TREE_RESULT_DT).copy()
        return self._rqt_tree

    @property
    def rqt_results(self):
        """the transform-tree decisions of the last step (RQT_RESULT_DT per unit): downloaded when asked for"""
        if getattr(self, "_rqt", None) is None:
            self._rqt = self.hv.down(self.rqt_plan["d_out"], np.int32).view(RQT_RESULT_DT).copy()
        return self._rqt

    @rqt_results.setter
    def rqt_results(self, v):
        self._rqt = v

    @property
    def rqt_rates(self):
        """residual_rates=True: {log2: int64 Q16 rate of every candidate of that transform size} of the last step (the order of rqt_plan["sizes"][log2]'s jobs):
        downloaded when asked for"""
        if self.tree_rates:      # ... tree_rates=True: {(unit size, depth): the whole-tree rate of every unit of that size, in the order of rqt_plan["tree_jobs"]}
            if getattr(self, "_rqt_rates", None) is None:
                with self.torch.cuda.stream(self.hv.tstream):
                    flat = self.rqt_plan["tree_rate"].cpu().numpy()
                self._rqt_rates = {key: flat[t["jobs"]["out_index"]].copy() for key, t in self.rqt_plan["tree_jobs"].items()}
            return self._rqt_rates
        if not self.residual_rates:
            raise ValueError("rqt_rates: the picture was made without residual_rates=True or tree_rates=True")
        if getattr(self, "_rqt_rates", None) is None:
            self._rqt_rates = {log2: self.hv.down(g["rates"], np.int64).copy() for log2, g in self.rqt_plan["sizes"].items()}
        return self._rqt_rates

    @property
    def cells(self):
        """the picture's block structure of the last step (CELL_DT [H / 4, W / 4]): on the device route k_block_cells leaves it in HBM and it is
        downloaded when asked for; the host route (search_on_device=False) made it on the host"""
        if getattr(self, "_cells", None) is None:
            from .havoc import CELL_DT
            self._cells = self.hv.down(self.d_cells, np.uint8).view(CELL_DT).reshape(self.H // 4, self.W // 4).copy()
        return self._cells

    @cells.setter
    def cells(self, v):
        self._cells = v

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
        n = ((self.W + 63) // 64 * 8 + 1) * ((self.H + 63) // 64 * 8 + 1)
        if not hasattr(self, "d_bs"):
            with torch.cuda.stream(hv.tstream):
                self.d_data = torch.zeros(n, dtype=torch.int8, device=hv.device)
                self.d_bs = torch.zeros(n, dtype=torch.uint8, device=hv.device)
                self.d_cells = torch.zeros(cells.size * 16, dtype=torch.uint8, device=hv.device)
            self.d_chroma = hv.up(np.full(2 * (self.H // 2) * (self.W // 2), 128 << (self.bd - 8), self.dt))
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
            hv.tu_forward_d(bd, 0, g["log2"], g["coef"], src, self.stride, self.pred, self.W, g["d_fj"])
            hv.rdoq_d(bd, g["log2"], g["level"], g["coef"], self.d_states, g["d_rj"], g["cbf"], g["work"])
            hv.tu_reconstruct_d(bd, 0, g["log2"], g["inv"], g["dshift"], self.recon, self.stride, self.pred, self.W, src, self.stride, g["level"], g["d_fj"], g["ssd"])

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
        self._merge = None
        if self.pu_modes:
            self.pu_candidates(res)
        if self.search_on_device:
            # everything after the searches is a FIXED sequence of launches over device-resident tables (the decided field never leaves the device, the decisions
            # between the launches are kernels): recorded once into a HIP graph, one launch per picture, one wait at the end
            self._rqt = self._cells = self._sao_decisions = self._rqt_rates = self._rqt_tree = self._cu_decisions = self._cqt_decisions = None
            self._unit_tree_decisions = self._cqt_commit = self._cqt_finish = self._cqt_motion = self._temporal = self._cqt_merge = None
            pu = (self.pu_mode_launches,) if self.pu_modes else ()      # (the tables its launches read went up before the replay: pu_candidates)
            pu += (self.unit_tree_launches,) if self.unit_trees else ()  # (behind pu_decide: it reads the winners in place; before cu_close, which reads its records)
            pu += (self.cu_close_launches,) if self.cu_close else ()     # (after the tree decisions AND the prediction units' rates: it reads both in place)
            pu += (self.cqt_launch,) if self.cqt else ()                 # (behind cu_close: it reads its records in place)
            pu += (self.cqt_commit_launch,) if self.commit else ()       # (directly behind the quadtree: it acts on its records, into buffers of its own)
            pu += (self.cqt_motion_launch,) if self.motion is not None else ()      # (directly behind the commit: it reads the cells that wrote, nothing else)
            pu += (self.cqt_finish_launch,) if self.finish else ()       # (behind the commit: it filters and pads what that wrote, in place)
            pu += (self.temporal_launch,) if self.col is not None and not self.temporal_mvp else ()      # (reads another picture's store and this picture's unit table
                                                                                                         # only; with temporal_mvp it ran before the searches)
            pu += (self.cqt_merge_launch,) if self.merge_lists is not None else ()      # (behind the commit, whose cells it reads, and the temporal candidates)
            if self.sao:
                self._replayed("after the searches", lambda: (self.merge_candidates(field), self.predict(field), self.sao_filter_inputs(field),
                                                              self.sao_loop_filter(), [f() for f in pu]))
            elif self.tree_rates:      # (the chroma reconstruction is the tree decision's own: chroma_chain, which codes chroma at depth 0 always, does not run)
                self._replayed("after the searches", lambda: (self.merge_candidates(field), self.predict(field), self.tree_and_filter_on_device(),
                                                              [f() for f in pu]))
            else:
                self._replayed("after the searches", lambda: (self.merge_candidates(field), self.predict(field), self.tree_and_filter_on_device(),
                                                              self.chroma_chain(field), [f() for f in pu]))
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
        import copy
        key = (band_ctu_rows, id(side))
        if getattr(self, "_views_key", None) != key:
            self._filter_buffers()
            rows = band_ctu_rows * 64
            views = []
            for y0 in range(0, self.H, rows):
                v = copy.copy(self)
                for name in ("mgroups", "pgroups", "cgroups", "rqt_plan", "d_merge_satd", "_merge", "_rqt", "_cells", "_views", "_views_key", "_graphs"):
                    v.__dict__.pop(name, None)
                v.hv, v._graphs, v.use_graphs = side, {}, True
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
        if self.pu_modes:
            raise ValueError("step_banded does not decide the prediction units' modes: use step() with pu_modes=True")
        if self.cu_close:
            raise ValueError("step_banded does not close coding units: use step() with cu_close=True")
        if self.cqt:
            raise ValueError("step_banded does not decide coding quadtrees: use step() with cqt=True")
        if self.unit_trees:
            raise ValueError("step_banded does not build the searched units' trees: use step() with unit_trees=True")
        if self.col is not None:
            raise ValueError("step_banded does not derive temporal candidates: use step() with col=")
        if self.sao:
            # SAO of band b reads the deblocked rows of band b + 1 (turing/TaskSao.cpp:46-56): not built
            raise ValueError("step_banded does not run SAO: use step() with sao=True")
        views = self._band_views(band_ctu_rows, side)
        if make_phase_planes:
            self.phase_planes()
        if not hasattr(self, "_dsearch"):
            n = len(self.pus)
            self._dsearch = dict(pus=hv.up(np.ascontiguousarray(self.pus).view(np.uint8).reshape(-1)), first=hv.up(np.ascontiguousarray(self.ctu_first, np.int32)),
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
        bstride = (W + 63) // 64 * 8 + 1
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
        self._merge = self._rqt = self._cells = None
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
            extra = dict(pu_modes=self.pu_decisions)
            if self.cu_close:
                extra["cu_close"] = self.cu_decisions
            if self.cqt:
                extra["cqt"] = self.cqt_decisions
            if self.unit_trees:
                extra["unit_trees"] = self.unit_tree_decisions()
            return out, hv.down(self.recon, self.dt), extra
        return out, hv.down(self.recon, self.dt)
