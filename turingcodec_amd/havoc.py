"""Host-side binding of libhavoc_mi355x.so (C ABI: include/havoc_mi355x.h).

PyTorch is used only as plumbing: device buffers (torch.uint8/int16/int32 CUDA tensors) and the current HIP
stream.  Every compute call goes through the C ABI into the hand-written gfx950 kernels; if the shared library
is missing or there is no GPU this module raises -- there is no CPU/eager fallback.

Two layers:
  * ``Havoc.<primitive>_d(...)``  device-level: tensors already in HBM, asynchronous on the context stream
  * ``Havoc.<primitive>(...)``    numpy-level batch interface used by the parity suite (tests/suite.py): uploads
                                  inputs, launches once per primitive (per size class where the reference's table
                                  is indexed by size), downloads the result.
Names and argument meaning mirror the reference's function types (havoc/sad.h:58, pred_inter.h:35, ...).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HAVOC_MI355X_LIB") or os.path.join(_HERE, "libhavoc_mi355x.so")      # the override: diagnostic builds of profiles/micro/ (timing variants)

_vp = C.c_void_p
_ip = C.c_ssize_t
_i = C.c_int



def search_workspace(width, height):
    """bytes of the device workspace a picture search of this size needs (havoc_mi355x_search_workspace)"""
    L, _ = _load()
    return int(L.havoc_mi355x_search_workspace(width, height))


class HavocError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise HavocError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(make -C turingcodec_amd/csrc).  There is no fallback path.")
    L = C.CDLL(LIB_PATH)
    L.havoc_mi355x_last_error.restype = C.c_char_p
    L.havoc_mi355x_version.restype = C.c_char_p
    sig = {
        "create": [C.POINTER(_vp), _i, _vp],
        "destroy": [_vp],
        "set_stream": [_vp, _vp],
        "sync": [_vp],
        "sync_spin": [_vp],
        "device_info": [_vp, C.POINTER(C.c_int64)],
        "malloc": [_vp, C.POINTER(_vp), C.c_size_t],
        "free": [_vp, _vp],
        "h2d": [_vp, _vp, _vp, C.c_size_t],
        "d2h": [_vp, _vp, _vp, C.c_size_t],
        "host_alloc": [_vp, C.c_size_t, C.POINTER(_vp), C.POINTER(_vp)],
        "host_free": [_vp, _vp],
        "h2d_async": [_vp, _vp, _vp, C.c_size_t],
        "d2h_async": [_vp, _vp, _vp, C.c_size_t],
        "copy_2d": [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t, _i],
        "picture_create": [_vp, _i, _i, _i, _i, _i, _i, C.POINTER(_vp)],
        "picture_destroy": [_vp, _vp],
        "picture_plane": [_vp, _i, C.POINTER(_vp), C.POINTER(C.c_int64), C.POINTER(_ip), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)],
        "picture_upload_yuv": [_vp, _vp, _vp, _i, _i, _i],
        "picture_upload_plane": [_vp, _vp, _i, _vp, _ip, _i],
        "picture_download_plane": [_vp, _vp, _i, _vp, _ip, _i],
        "picture_pad": [_vp, _vp],
        "picture_phase_planes": [_vp, _vp, C.POINTER(_vp), C.POINTER(_ip), C.POINTER(C.c_int64)],
        "timer_start": [_vp],
        "timer_stop_ms": [_vp, C.POINTER(C.c_float)],
        "graph_begin": [_vp],
        "graph_end": [_vp, C.POINTER(_vp)],
        "graph_launch": [_vp, _vp],
        "graph_destroy": [_vp],
        "fork": [_vp, _i],
        "lane": [_vp, _i],
        "join": [_vp],
        "sad": [_vp, _i, _vp, _ip, _vp, _ip, _vp, _i, _vp],
        "sad4": [_vp, _i, _vp, _ip, _vp, _ip, _vp, _i, _vp],
        "sad4_runs": [_vp, _i, _vp, _ip, _vp, _ip, _vp, _i, _vp, _i, _vp],
        "sad4_make_runs": [_vp, _i, _i, _ip, _i, _vp],
        "pad_block": [_vp, _i, _vp, C.c_int64, _i, _i, _ip, _i, _i, _i, _i, _i],
        "sad_surface": [_vp, _i, _i, _i, _i, _vp, _ip, _vp, _ip, _vp, _i, _vp],
        "deblock": [_vp, _i, _i, _vp, _ip, _vp, _vp, _ip, _i, _i, _vp, _vp, _i, _i, _i, _i],
        "derive_bs": [_vp, _vp, _ip, _i, _i, _vp, _vp],
        "ssd": [_vp, _i, _vp, _ip, _vp, _ip, _vp, _i, _vp],
        "satd": [_vp, _i, _i, _i, _vp, _ip, _vp, _ip, _vp, _i, _vp],
        "satd_multi": [_vp, _i, _i, _i, _vp, _ip, _vp, _ip, _vp, _i, _vp],
        "ssd_linear": [_vp, _vp, _vp, _i, _vp],
        "pred_uni": [_vp, _i, _i, _i, _i, _i, _vp, _ip, _vp, _ip, _vp, _i],
        "pred_bi": [_vp, _i, _i, _i, _i, _i, _vp, _ip, _vp, _ip, _vp, _i],
        "subtract_bi": [_vp, _i, _i, _vp, _ip, _vp, _ip, _vp, _ip, _vp, _i],
        "pred_uni_classes": [_vp, _i, _i, _i, _vp, _ip, _vp, _ip, _vp, C.POINTER(C.c_int32)],
        "pred_bi_classes": [_vp, _i, _i, _i, _vp, _ip, _vp, _ip, _vp, C.POINTER(C.c_int32)],
        "intra": [_vp, _i, _i, _i, _vp, _ip, _vp, _vp, _i],
        "intra_satd35": [_vp, _i, _i, _i, _vp, _ip, _vp, _vp, _i, _vp],
        "subpel_satd": [_vp, _i, _i, _i, _i, _i, _vp, _ip, _vp, _ip, _vp, _i, _vp],
        "interp_planes": [_vp, _i, _i, _vp, _ip, _vp, _ip, _i, _i, _i, _i],
        "residual": [_vp, _i, _vp, _ip, _vp, _vp, _ip, _vp, _ip, _vp, _i],
        "transform": [_vp, _i, _i, _i, _vp, _vp, _ip, _vp, _i],
        "inverse_transform": [_vp, _i, _i, _i, _vp, _vp, _vp, _i],
        "inverse_transform_add": [_vp, _i, _i, _i, _i, _vp, _ip, _vp, _ip, _vp, _vp, _i],
        "tu_forward": [_vp, _i, _i, _i, _i, _vp, _vp, _ip, _vp, _ip, _vp, _i],
        "tu_reconstruct": [_vp, _i, _i, _i, _i, _i, _i, _vp, _ip, _vp, _ip, _vp, _ip, _vp, _vp, _i, _vp],
        "intra_measure": [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _ip, _vp, _ip, _vp, _i, _i],
        "level_stats": [_vp, _vp, _vp, _i, _vp],
        "search_motion_uni": [_vp, _i, _vp, _vp, C.c_int64, _ip, _vp, C.c_int64, _ip, _vp, _ip, C.c_int64, _vp, _i, _vp],
        "rqt_decide": [_vp, _vp, _i, _vp, _vp, _vp, C.c_int64, C.c_ssize_t, _i, _i, _vp],
        "block_cells": [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp],
        "intra_gather": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp],
        "intra_commit": [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i],
        "intra_fill_spare": [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp],
        "merge_jobs": [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp],
        "merge_decide": [_vp, _vp, _vp, _vp, _i, C.c_int64, _vp, _vp],
        "pred_jobs": [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp],
        "search_motion_bi": [_vp, _i, _vp, _vp, C.c_int64, _ip, _vp, C.c_int64, _ip, _vp, _ip, C.c_int64, _vp, C.c_int64, _vp, _vp, _i, _vp],
        "search_picture_uni": [_vp, _i, _vp, _vp, _vp, C.c_int64, _ip, _vp, _vp, _ip, _vp, _ip, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i],
        "search_gate": [_vp, _vp],
        "search_temporal": [_vp, _vp, _i],
        "search_wait_rows": [_vp, _vp, _i, _i, _i, _vp],
        "block_cells_add": [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp],
        "intra_order": [_vp, _vp, _vp, _i, C.c_int32, _vp, _vp, _vp, _vp],
        "intra_expand": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp],
        "intra_decide": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, C.c_int32, _vp, _vp],
        "quantize": [_vp, _vp, _vp, _vp, _i, _vp],
        "quantize_inverse": [_vp, _vp, _vp, _vp, _i],
        "quantize_reconstruct": [_vp, _i, _vp, _ip, _vp, _ip, _vp, _vp, _i],
        "rdoq": [_vp, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, C.c_size_t],
        "tu_forward_scan": [_vp, _i, _i, _i, _vp, _vp, _ip, _vp, _ip, _vp, _i, _vp, _vp, _vp, C.c_size_t],
        "rdoq_prescanned": [_vp, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, C.c_size_t],
        "residual_rate": [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp],
        "intra_rate": [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp],
        "intra_rate_jobs": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp],
        "tree_rate": [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp],
        "pu_rate": [_vp, _vp, _vp, _i, _vp, _vp, _vp],
        "pu_decide": [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp],
        "cu_close": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, C.c_int32, _vp, _vp, _vp],
        "unit_pred_ssd": [_vp, _i, _vp, C.c_ssize_t, _vp, C.c_ssize_t, _vp, C.c_ssize_t, _vp, C.c_ssize_t, _vp, _i, _vp],
        "unit_pred_select": [_vp, _i, _vp, _vp, _vp, C.c_ssize_t, _vp, C.c_ssize_t, _vp, _vp, _vp, _vp, _i, _vp, _vp],
        "cqt_decide": [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, C.c_size_t, _vp, _vp, _vp, _vp],
        "cqt_commit": [_vp, _vp],
        "cqt_block_cells": [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _ip],
        "cqt_motion_store": [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp],
        "temporal_candidates": [_vp, _vp, _vp, _ip, _vp, _i, _vp],
        "cqt_merge_lists": [_vp, _vp, _vp, _vp, _i, _vp, _vp],
        "intra_decide_rated": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, C.c_int32, _vp, _vp],
        "rqt_decide_rated": [_vp, _vp, _i, _vp, _vp, _vp, _vp, C.c_int64, C.c_ssize_t, _i, _i, _vp],
        "rqt_decide_tree": [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_ssize_t, _i, C.c_int64, C.c_int64, C.c_ssize_t, _i, _i, _vp, _vp],
        "rqt_decide_units": [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp],
        "sao_stats": [_vp, _i, _i, _vp, _ip, _vp, _ip, _vp, _i, _vp],
        "sao_filter": [_vp, _i, _i, _vp, _ip, _vp, _ip, _vp, _i],
        "sao_band_chroma": [_vp, _i, _i, _vp, _ip, _vp, _ip, _vp, _i, _vp],
        "sao_estimate": [_vp, _i, _i, C.c_int32, _i, _vp, _vp, _ip, _ip, _vp, _vp, _ip, _ip, _vp, _vp, _ip, _ip, _vp, _i, _vp, C.c_size_t, _vp],
        "sao_decide": [_vp, _i, _i, C.c_int32, _i, _vp, _vp, _ip, _ip, _vp, _vp, _ip, _ip, _vp, _vp, _ip, _ip, _vp, _i, _i, _vp, _i, _i, _vp, C.c_size_t,
                       _vp],
        "sao_apply": [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _ip, _ip, _vp, _vp, _vp, _ip, _ip, _vp, _vp, _vp, _ip],
    }
    L.havoc_mi355x_rdoq_lambda.argtypes = [C.c_double, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.havoc_mi355x_rdoq_lambda.restype = None
    L.havoc_mi355x_rdoq_workspace.argtypes = [_i]
    L.havoc_mi355x_rdoq_workspace.restype = C.c_size_t
    L.havoc_mi355x_sao_workspace.argtypes = [_i]
    L.havoc_mi355x_sao_workspace.restype = C.c_size_t
    L.havoc_mi355x_sao_decide_workspace.argtypes = [_i]
    L.havoc_mi355x_sao_decide_workspace.restype = C.c_size_t
    L.havoc_mi355x_cqt_decide_workspace.argtypes = [_i]
    L.havoc_mi355x_cqt_decide_workspace.restype = C.c_size_t
    L.havoc_mi355x_search_workspace.argtypes = [_i, _i]
    L.havoc_mi355x_search_workspace.restype = C.c_size_t
    for name, args in sig.items():
        f = getattr(L, "havoc_mi355x_" + name)
        f.argtypes = args
        f.restype = None if name in ("destroy", "graph_destroy", "picture_destroy") else _i
    return L, sorted(sig)


def exported_symbols():
    """names the C ABI must export (checked against include/havoc_mi355x.h by the CPU tests)"""
    _, names = _load()
    return ["havoc_mi355x_" + n for n in names] + ["havoc_mi355x_last_error", "havoc_mi355x_version", "havoc_mi355x_rdoq_lambda", "havoc_mi355x_rdoq_workspace",
                                                "havoc_mi355x_search_workspace", "havoc_mi355x_sao_workspace", "havoc_mi355x_sao_decide_workspace",
                                                "havoc_mi355x_cqt_decide_workspace"]


# one havoc_mi355x_cell (include/havoc_mi355x.h), 16 bytes: a 4x4 luma cell of a picture's block structure
CELL_DT = np.dtype([("mv", "<i2", (2, 2)), ("dpb_index", "i1", (2,)), ("flags", "u1"), ("qp_y", "i1"), ("tu_log2", "u1"), ("reserved", "u1", (3,))])
assert CELL_DT.itemsize == 16
CELL_INTRA, CELL_CODED, CELL_NO_FILTER, CELL_PU_LEFT, CELL_PU_TOP = 1, 2, 4, 8, 16

# one havoc_mi355x_sao_job (include/havoc_mi355x.h), 96 bytes
SAO_JOB_DT = np.dtype([("dst_off", "<i4"), ("src_off", "<i4"), ("w", "<i4"), ("h", "<i4"), ("type", "<i4"), ("eo_class", "<i4"), ("offsets", "<i2", 32),
                       ("reserved", "<i4", 2)])
assert SAO_JOB_DT.itemsize == 96

# one havoc_mi355x_sao_ctu (include/havoc_mi355x.h), 64 bytes: a CTU's blocks in the source, reconstruction and destination planes
SAO_CTU_DT = np.dtype([("src_y", "<i4"), ("src_cb", "<i4"), ("src_cr", "<i4"), ("rec_y", "<i4"), ("rec_cb", "<i4"), ("rec_cr", "<i4"),
                       ("dst_y", "<i4"), ("dst_cb", "<i4"), ("dst_cr", "<i4"), ("w", "<i4"), ("h", "<i4"), ("reserved", "<i4"),
                       ("stat_src_cb", "<i4"), ("stat_src_cr", "<i4"), ("stat_rec_cb", "<i4"), ("stat_rec_cr", "<i4")])
assert SAO_CTU_DT.itemsize == 64

# one havoc_mi355x_sao_params (include/havoc_mi355x.h), 128 bytes: comp[0] luma, comp[1] chroma (Cb and Cr share it)
SAO_COMPONENT_DT = np.dtype([("type", "<i4"), ("eo_class", "<i4"), ("band_position", "<i4"), ("offset_abs", "<i4", 4), ("offset_sign", "<i4", 4)])
SAO_PARAMS_DT = np.dtype([("comp", SAO_COMPONENT_DT, 2), ("dist_sao", "<i4"), ("dist_off", "<i4"), ("ssd_sao", "<u4", 3), ("ssd_off", "<u4", 3),
                          ("reserved", "<i4", 2)])
assert SAO_COMPONENT_DT.itemsize == 44 and SAO_PARAMS_DT.itemsize == 128

# one havoc_mi355x_sao_decision (include/havoc_mi355x.h), 128 bytes: a CTU's final SAO parameters, merge flags, distortion and the
# states of the contexts sao_merge_X_flag and sao_type_idx_X before and after its SAO syntax
SAO_DECISION_DT = np.dtype([("comp", SAO_COMPONENT_DT, 2), ("merge_left", "<i4"), ("merge_up", "<i4"), ("dist", "<i4"), ("source", "<i4"),
                            ("ctx_merge_before", "u1"), ("ctx_type_before", "u1"), ("ctx_merge_after", "u1"), ("ctx_type_after", "u1"),
                            ("decided", "<i4"), ("reserved", "<i4", 4)])
assert SAO_DECISION_DT.itemsize == 128

# one havoc_mi355x_sao_bounds (include/havoc_mi355x.h), 32 bytes: LoopFilter::Ctu's bounds in luma samples and its corner flags
SAO_BOUNDS_DT = np.dtype([("left", "<i4"), ("top", "<i4"), ("right", "<i4"), ("bottom", "<i4"), ("corners", "<i4"), ("reserved", "<i4", 3)])
assert SAO_BOUNDS_DT.itemsize == 32
SAO_CORNER_TL, SAO_CORNER_TR, SAO_CORNER_BL, SAO_CORNER_BR = 1, 2, 4, 8


def sao_bounds_table(width, height, ctb_size, slice_starts=(0,), across_slices=(1,)):
    """SAO_BOUNDS_DT records of every CTU in raster order, as LoopFilter::Picture::processCtu and neighbourCtuAvailable derive them
    (turing/LoopFilter.h:462-537) for slices in raster order, one tile: slice s starts at CTU slice_starts[s] (ascending, the first 0) with
    slice_loop_filter_across_slices_enabled_flag across_slices[s].  A neighbour is unavailable outside the picture, or when it precedes
    the current CTU's slice and that slice's flag is 0.  A CTU's right / bottom and its bottomRight / bottomLeft are set by the LATER CTU,
    with that CTU's flag."""
    assert ctb_size in (16, 32, 64) and len(slice_starts) == len(across_slices) and slice_starts[0] == 0
    assert all(a < b for a, b in zip(slice_starts, slice_starts[1:]))
    cx, cy = -(-width // ctb_size), -(-height // ctb_size)
    out = np.zeros(cx * cy, SAO_BOUNDS_DT)
    slice_of = np.searchsorted(np.asarray(slice_starts), np.arange(cx * cy), side="right") - 1
    for a in range(cx * cy):
        rx, ry = a % cx, a // cx
        start, across = slice_starts[slice_of[a]], across_slices[slice_of[a]]

        def available(dx, dy):
            if not (0 <= rx + dx < cx and 0 <= ry + dy < cy):
                return False
            return a + dx + dy * cx >= start or bool(across)

        c = out[a]
        c["left"], c["top"], c["right"], c["bottom"] = 0, 0, width, height
        if not available(-1, 0):
            c["left"] = rx * ctb_size
            if rx:
                out[a - 1]["right"] = rx * ctb_size
        if not available(0, -1):
            c["top"] = ry * ctb_size
            if ry:
                out[a - cx]["bottom"] = ry * ctb_size
        corners = 0
        tl, tr = available(-1, -1), available(1, -1)
        corners |= SAO_CORNER_TL if tl else 0
        if rx and ry:
            out[a - 1 - cx]["corners"] = (out[a - 1 - cx]["corners"] & ~SAO_CORNER_BR) | (SAO_CORNER_BR if tl else 0)
        corners |= SAO_CORNER_TR if tr else 0
        if rx < cx - 1 and ry:
            out[a + 1 - cx]["corners"] = (out[a + 1 - cx]["corners"] & ~SAO_CORNER_BL) | (SAO_CORNER_BL if tr else 0)
        c["corners"] = corners        # bottomRight / bottomLeft false until a later CTU sets them
    return out


def sao_context_init(slice_qp, init_type):
    """-> (state of sao_merge_X_flag, state of sao_type_idx_X) at the start of a slice: H.265 9.3.2.2 with the initValues of Tables 9-5 /
    9-6 (sao_merge: 153 for every initType; sao_type_idx: 200, 185, 160), as ContextModel::state = 2 pStateIdx + valMps"""
    assert init_type in (0, 1, 2)

    def state(init_value):
        m, n = (init_value >> 4) * 5 - 45, ((init_value & 15) << 3) - 16
        pre = min(max(1, ((m * min(max(0, slice_qp), 51)) >> 4) + n), 126)
        return 2 * (pre - 64) + 1 if pre >= 64 else 2 * (63 - pre)
    return state(153), state((200, 185, 160)[init_type])


def sao_layout(width, height, pad=8):
    """A padded 4:2:0 picture layout for havoc_mi355x_sao_estimate: a luma plane of (height + 2 pad) rows of stride width + 2 pad, and one
    chroma plane holding Cb then Cr, each (height / 2 + pad) rows of stride width / 2 + pad.  The edge filter reads one sample beyond every
    CTU, so pad >= 2.  -> dict: pad, stride_y, stride_c, size_y (samples of the luma plane), size_c (samples of ONE chroma component)."""
    assert pad >= 2 and pad % 2 == 0 and width % 2 == 0 and height % 2 == 0
    sy, sc = width + 2 * pad, width // 2 + pad
    return dict(pad=pad, stride_y=sy, stride_c=sc, size_y=sy * (height + 2 * pad), size_c=sc * (height // 2 + pad))


def sao_ctu_table(width, height, ctb_size, pad=8, chroma_stats="ctu"):
    """SAO_CTU_DT records of every CTU of a width x height picture in raster order, for source, reconstruction and destination all in
    sao_layout(width, height, pad); the CTUs of the last column / row are clipped to the picture (EncSao.h:290-297).
    chroma_stats: where the chroma decision reads its statistics -- "ctu": the CTU's own Cb / Cr blocks; "reference": where
    saoRdEstimateChroma reads them (EncSao.h:534-546 halves the chroma position a second time through ThreePlanes::operator(),
    Picture.h:179-187: the block at (x / 4, y / 4) of the chroma plane, of the CTU's chroma size)."""
    assert ctb_size in (16, 32, 64) and chroma_stats in ("ctu", "reference")
    L = sao_layout(width, height, pad)
    sy, sc, p, pc = L["stride_y"], L["stride_c"], pad, pad // 2
    rows = []
    for y in range(0, height, ctb_size):
        for x in range(0, width, ctb_size):
            w, h = min(ctb_size, width - x), min(ctb_size, height - y)
            oy = (y + p) * sy + x + p
            ocb = (y // 2 + pc) * sc + x // 2 + pc
            ocr = L["size_c"] + ocb
            scb = ocb if chroma_stats == "ctu" else (y // 4 + pc) * sc + x // 4 + pc
            rows.append((oy, ocb, ocr, oy, ocb, ocr, oy, ocb, ocr, w, h, 0, scb, L["size_c"] + scb, scb, L["size_c"] + scb))
    return np.array(rows, np.int32).view(SAO_CTU_DT).reshape(-1)


# one havoc_mi355x_rdoq_job (include/havoc_mi355x.h), 48 bytes
RDOQ_JOB_DT = np.dtype([("dst_off", "<i4"), ("src_off", "<i4"), ("quant_scale", "<i4"), ("quant_shift", "<i4"), ("inv_scale", "<i4"),
                        ("lambda_q16", "<i4"), ("sdh_factor", "<i4"), ("ctx_index", "<i4"), ("c_idx", "u1"), ("scan_idx", "u1"),
                        ("is_intra", "u1"), ("sdh", "u1"), ("reserved", "<i4", 3)])
assert RDOQ_JOB_DT.itemsize == 48


# one havoc_mi355x_residual_rate_job (include/havoc_mi355x.h), 32 bytes
RESIDUAL_RATE_JOB_DT = np.dtype([("level_off", "<i4"), ("ctx_index", "<i4"), ("rate_index", "<i4"), ("c_idx", "u1"), ("scan_idx", "u1"), ("sdh", "u1"), ("count", "u1"),
                                 ("reserved", "<i4", 4)])
assert RESIDUAL_RATE_JOB_DT.itemsize == 32

# one havoc_mi355x_intra_rate_job (include/havoc_mi355x.h), 32 bytes; mpm_idx 3 = rem_intra_luma_pred_mode; flags: INTRA_RATE_*
INTRA_RATE_JOB_DT = np.dtype([("level_off", "<i4"), ("ctx_index", "<i4"), ("rate_index", "<i4"), ("scan_idx", "u1"), ("sdh", "u1"), ("mpm_idx", "u1"), ("flags", "u1"),
                              ("reserved", "<i4", 4)])
assert INTRA_RATE_JOB_DT.itemsize == 32
INTRA_RATE_SPLIT_FLAG_CODED, INTRA_RATE_DEPTH_NONZERO = 1, 2
INTRA_SYNTAX_CTX_BYTES = 4      # HAVOC_INTRA_SYNTAX_CTX_*: prev_intra_luma_pred_flag, split_transform_flag[0..2]

# one havoc_mi355x_tree_rate_job (include/havoc_mi355x.h), 32 bytes: one candidate transform tree of an inter unit at the launch's depth; flags: TREE_RATE_*
TREE_RATE_JOB_DT = np.dtype([("luma_off", "<i4"), ("cb_off", "<i4"), ("cr_off", "<i4"), ("ctx_index", "<i4"), ("out_index", "<i4"), ("sdh", "u1"), ("flags", "u1"),
                             ("pad", "u1", 2), ("reserved", "<i4", 2)])
assert TREE_RATE_JOB_DT.itemsize == 32
TREE_RATE_SPLIT_FLAG_CODED = 1
# one havoc_mi355x_pu_rate_job (include/havoc_mi355x.h), 32 bytes: one candidate of a prediction unit; mvd [list][x, y]; pred: PU_PRED_*; flags: PU_RATE_*
PU_RATE_JOB_DT = np.dtype([("ctx_index", "<i4"), ("out_index", "<i4"), ("mvd", "<i2", (2, 2)), ("merge_idx", "u1"), ("pred", "u1"), ("mvp_flag", "u1", 2),
                           ("ref_idx", "u1", 2), ("w", "u1"), ("h", "u1"), ("cqt_depth", "u1"), ("flags", "u1"), ("pad", "u1", 2), ("reserved", "<i4")])
assert PU_RATE_JOB_DT.itemsize == 32
PU_RATE_MERGE, PU_RATE_SKIP = 1, 2
PU_PRED_L0, PU_PRED_L1, PU_PRED_BI = 0, 1, 2
PU_SYNTAX_CTX_BYTES = 16        # HAVOC_PU_SYNTAX_CTX_*: merge_flag, merge_idx, inter_pred_idc[5], ref_idx_lX[2], abs_mvd_greater0 / 1_flag, mvp_lX_flag, 4 reserved


class PuSlice(C.Structure):
    """havoc_mi355x_pu_slice: the slice-level values Syntax<prediction_unit> reads"""
    _fields_ = [("slice_b", C.c_int32), ("max_num_merge_cand", C.c_int32), ("mvd_l1_zero_flag", C.c_int32), ("num_ref_idx_active_minus1", C.c_int32 * 2),
                ("reserved", C.c_int32 * 3)]

    def __init__(self, slice_b=1, max_num_merge_cand=5, mvd_l1_zero_flag=0, num_ref_idx_active_minus1=(0, 0)):
        super().__init__(int(slice_b), int(max_num_merge_cand), int(mvd_l1_zero_flag), (C.c_int32 * 2)(*[int(v) for v in num_ref_idx_active_minus1]))


assert C.sizeof(PuSlice) == 32

# one havoc_mi355x_cu_close_job / havoc_mi355x_cu_choice / havoc_mi355x_pred_ssd_job (include/havoc_mi355x.h): a candidate coding unit, what closing it gave, a unit's
# three blocks of source and prediction
CU_CLOSE_JOB_DT = np.dtype([("ctx_index", "<i4"), ("unit_index", "<i4"), ("pu_rate_index", "<i4"), ("pu_before_index", "<i4"), ("pu_after_index", "<i4"),
                            ("log2_cb_size", "u1"), ("part_mode", "u1"), ("skip_ctx_inc", "u1"), ("merge_idx", "u1"), ("flags", "u1"), ("pad", "u1", 3), ("reserved", "<i4")])
CU_CHOICE_DT = np.dtype([("outcome", "<i4"), ("have_residual", "<i4"), ("rate", "<i8"), ("lambda_distortion", "<i8"), ("cost", "<i8"), ("cost_coded", "<i8"),
                         ("cost_no_residual", "<i8")])
PRED_SSD_JOB_DT = np.dtype([("src_off", "<i4", 3), ("pred_off", "<i4", 3), ("log2_size", "<i4"), ("reserved", "<i4")])
assert CU_CLOSE_JOB_DT.itemsize == 32 and CU_CHOICE_DT.itemsize == 48 and PRED_SSD_JOB_DT.itemsize == 32
# one havoc_mi355x_pred_select_job, 32 bytes: where a unit's three candidate predictions lie and where the winner's goes (offsets in samples per plane: Y, Cb, Cr)
PRED_SELECT_JOB_DT = np.dtype([("cand_off", "<i4", 3), ("dst_off", "<i4", 3), ("log2_size", "<i4"), ("unit", "<i4")])
assert PRED_SELECT_JOB_DT.itemsize == 32
CU_CLOSE_MIN_CB, CU_CLOSE_AMP, CU_CLOSE_MERGE_2Nx2N = 1, 2, 4
CU_OUTCOME_REFUSED, CU_OUTCOME_CODED, CU_OUTCOME_NO_RESIDUAL, CU_OUTCOME_SKIPPED = -1, 0, 1, 2
CU_SYNTAX_CTX_BYTES = 16        # HAVOC_CU_SYNTAX_CTX_*: split_cu_flag[3], cu_skip_flag[3], pred_mode_flag, part_mode[4], rqt_root_cbf, 4 reserved
# one havoc_mi355x_cqt_ctu / havoc_mi355x_cqt_node (include/havoc_mi355x.h): a CTU's decided coding quadtree, one node of it
CQT_CTU_DT = np.dtype([("decided", "<i4"), ("n_cus", "<i4"), ("rate", "<i8"), ("flag_rate", "<i8"), ("lambda_distortion", "<i8"), ("cost", "<i8")])
CQT_NODE_DT = np.dtype([("choice", "u1"), ("flags", "u1"), ("ctx_inc", "u1"), ("pad", "u1", 5), ("cost_full", "<i8"), ("cost_split", "<i8")])
assert CQT_CTU_DT.itemsize == 40 and CQT_NODE_DT.itemsize == 24
CQT_WPP, CQT_ECU = 1, 2
CQT_NOT_VISITED, CQT_CU, CQT_SPLIT, CQT_DELETED = 0, 1, 2, 3
CQT_NODE_FINAL, CQT_NODE_FLAG_CODED, CQT_NODE_MUST_SPLIT, CQT_NODE_ECU_STOP, CQT_NODE_NO_CANDIDATE, CQT_NODE_NO_SPLIT_CANDIDATE = 1, 2, 4, 8, 16, 32
# one havoc_mi355x_cqt_cell (include/havoc_mi355x.h), 24 bytes: the decided coding unit that covers a MinCb cell; all-ones bytes (unit -1): none
CQT_CELL_DT = np.dtype([("unit", "<i4"), ("cand", "<i4"), ("mv", "<i2", (2, 2)), ("log2_size", "u1"), ("outcome", "u1"), ("pred", "u1"), ("tr_depth", "u1"), ("cbf", "<u4")])
assert CQT_CELL_DT.itemsize == 24
# one havoc_mi355x_col_cell, 24 bytes: an entry of the collocated motion store (one per 16x16 luma samples); one havoc_mi355x_temporal_params, 48 bytes; one
# havoc_mi355x_temporal_cand, 8 bytes: a prediction unit's temporal candidate for one list (source: 0 none, 1 the bottom-right cell, 2 the centre cell)
COL_CELL_DT = np.dtype([("mv", "<i2", (2, 2)), ("ref_poc", "<i4", (2,)), ("pred_flag", "u1", (2,)), ("long_term", "u1", (2,)), ("reserved", "<u4")])
TEMPORAL_PARAMS_DT = np.dtype([("pic_width", "<i4"), ("pic_height", "<i4"), ("ctb_log2", "<i4"), ("col_poc", "<i4"), ("cur_poc", "<i4"), ("target_poc", "<i4", (2,)),
                               ("all_backwards", "<i4"), ("collocated_from_l0", "<i4"), ("reserved", "<i4", (3,))])
TEMPORAL_CAND_DT = np.dtype([("mv", "<i2", (2,)), ("available", "<i2"), ("source", "<i2")])
assert COL_CELL_DT.itemsize == 24 and TEMPORAL_PARAMS_DT.itemsize == 48 and TEMPORAL_CAND_DT.itemsize == 8
TEMPORAL_NONE, TEMPORAL_BOTTOM_RIGHT, TEMPORAL_CENTRE = 0, 1, 2


# one havoc_mi355x_merge_cand, 12 bytes; one havoc_mi355x_merge_list, 64 bytes: a final coding unit's merge candidate list (n_cand places of cand are the list,
# n_real of them are not zero candidates, match: the lowest merge index that carries the unit's committed motion or -1); one havoc_mi355x_merge_params, 48 bytes
MERGE_CAND_DT = np.dtype([("mv", "<i2", (2, 2)), ("pred_flag", "u1", (2,)), ("ref_idx", "i1", (2,))])
MERGE_LIST_DT = np.dtype([("cand", MERGE_CAND_DT, (5,)), ("n_cand", "i1"), ("n_real", "i1"), ("match", "i1"), ("reserved", "u1")])
MERGE_PARAMS_DT = np.dtype([("pic_width", "<i4"), ("pic_height", "<i4"), ("ctb_log2", "<i4"), ("min_cb_log2", "<i4"), ("max_cand", "<i4"), ("ref_poc", "<i4", (2,)),
                            ("reserved", "<i4", (5,))])
assert MERGE_CAND_DT.itemsize == 12 and MERGE_LIST_DT.itemsize == 64 and MERGE_PARAMS_DT.itemsize == 48


def merge_params(pic_width, pic_height, ctb_log2, min_cb_log2, max_cand, ref_poc):
    """-> one MERGE_PARAMS_DT record"""
    p = np.zeros(1, MERGE_PARAMS_DT)
    p["pic_width"], p["pic_height"], p["ctb_log2"], p["min_cb_log2"], p["max_cand"], p["ref_poc"] = pic_width, pic_height, ctb_log2, min_cb_log2, max_cand, tuple(ref_poc)
    return p


def temporal_params(pic_width, pic_height, ctb_log2, col_poc, cur_poc, target_poc, all_backwards, collocated_from_l0):
    """-> one TEMPORAL_PARAMS_DT record"""
    p = np.zeros(1, TEMPORAL_PARAMS_DT)
    p["pic_width"], p["pic_height"], p["ctb_log2"], p["col_poc"], p["cur_poc"] = pic_width, pic_height, ctb_log2, col_poc, cur_poc
    p["target_poc"], p["all_backwards"], p["collocated_from_l0"] = tuple(target_poc), int(all_backwards), int(collocated_from_l0)
    return p


class CqtCommitArgs(C.Structure):
    """havoc_mi355x_cqt_commit_args: what havoc_mi355x_cqt_commit reads in place and where the decided picture and its cells go"""
    _fields_ = ([(k, C.c_int32) for k in ("bit_depth", "width", "height", "ctb_log2", "min_cb_log2", "n")] +
                [(k, _vp) for k in ("d_units", "d_node_cu", "d_ctu", "d_node", "d_cu", "d_choice", "d_tree_choice", "d_zero_at", "d_one_at", "d_chroma_at")] +
                [("luma_pieces", _vp * 4), ("chroma_pieces", _vp * 3), ("d_pred_y", _vp), ("d_pred_c", _vp), ("pred_stride", _ip), ("pred_stride_c", _ip),
                 ("d_pred_off", _vp), ("d_best", _vp), ("d_unit_cand", _vp), ("d_cand_mv", _vp), ("d_rec_y", _vp), ("rec_origin", C.c_int64), ("rec_stride", _ip),
                 ("d_rec_c", _vp), ("cb_origin", C.c_int64), ("cr_origin", C.c_int64), ("c_stride", _ip), ("d_cells", _vp)])


assert C.sizeof(CqtCommitArgs) == 288


def cqt_nodes(ctb_log2, min_cb_log2):
    """nodes of a CTU's coding quadtree: 1 + 4 + ... + 4^(ctb_log2 - min_cb_log2); node (d, z) has index (4^d - 1) / 3 + z"""
    return (4 ** (ctb_log2 - min_cb_log2 + 1) - 1) // 3


# havoc_mi355x_rqt_chroma_at / havoc_mi355x_rqt_tree_choice (include/havoc_mi355x.h), 16 bytes each: where a unit's chroma candidates are / what rqt_decide_tree adds
RQT_CHROMA_AT_DT = np.dtype([("cb_zero", "<i4"), ("cr_zero", "<i4"), ("cb_one", "<i4"), ("cr_one", "<i4")])
RQT_TREE_RESULT_DT = np.dtype([("mask_zero", "<u4"), ("mask_one", "<u4"), ("chroma_ssd_zero", "<i4"), ("chroma_ssd_one", "<i4")])


def rdoq_lambda(lam, inv_scale):
    """(lambda_q16, sdh_factor) of a job, as the reference's Rdoq constructor derives them (turing/Rdoq.h:163-167)"""
    L, _ = _load()
    a, b = C.c_int32(), C.c_int32()
    L.havoc_mi355x_rdoq_lambda(float(lam), int(inv_scale), C.byref(a), C.byref(b))
    return a.value, b.value


def _ptr(t):
    return t.data_ptr() if t is not None else None


class Havoc:
    """One context per process / GPU (the reference's `havoc_code`, havoc/havoc.h:138-147)."""

    def __init__(self, device=0, stream=None):
        import torch
        self.torch = torch
        self.L, _ = _load()
        if not torch.cuda.is_available():
            raise HavocError("no GPU visible: libhavoc_mi355x has no CPU path")
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        # stream: None -> torch's current stream; "new" -> a private non-blocking stream (needed for graph capture), made
        # through torch so that the numpy-level wrappers below can run their allocations, fills and copies on the SAME
        # stream as the kernels (`self.tstream`): nothing then depends on incidental synchronisation; an int -> that
        # hipStream_t (wrapped as an external torch stream for the same reason)
        if stream == "new":
            self.tstream = torch.cuda.Stream(device=self.device)
        elif stream is None:
            self.tstream = torch.cuda.current_stream(self.device)
        else:
            self.tstream = torch.cuda.ExternalStream(int(stream), device=self.device)
        s = _vp(self.tstream.cuda_stream)
        h = _vp()
        self._ck(self.L.havoc_mi355x_create(C.byref(h), device, s))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.havoc_mi355x_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise HavocError(f"libhavoc_mi355x error {rc}: {self.L.havoc_mi355x_last_error().decode()}")

    # ---------------------------------------------------------------- plumbing
    def sync(self):
        self._ck(self.L.havoc_mi355x_sync(self.h))

    def device_info(self):
        a = (C.c_int64 * 8)()
        self._ck(self.L.havoc_mi355x_device_info(self.h, a))
        keys = ["cus", "clock_khz", "mem_clock_khz", "bus_bits", "l2_bytes", "wave", "lds_per_wg", "mem_mib"]
        return dict(zip(keys, [int(x) for x in a]))

    def fork(self, nlanes):
        self._ck(self.L.havoc_mi355x_fork(self.h, nlanes))

    def lane(self, k):
        self._ck(self.L.havoc_mi355x_lane(self.h, k))

    def join(self):
        self._ck(self.L.havoc_mi355x_join(self.h))

    def graph_capture(self, fn):
        """record the launches `fn()` issues into a HIP graph; returns a handle for graph_launch"""
        self._ck(self.L.havoc_mi355x_graph_begin(self.h))
        try:
            fn()
        finally:
            g = _vp()
            rc = self.L.havoc_mi355x_graph_end(self.h, C.byref(g))
        self._ck(rc)
        return g

    def graph_launch(self, g):
        self._ck(self.L.havoc_mi355x_graph_launch(self.h, g))

    def graph_destroy(self, g):
        self.L.havoc_mi355x_graph_destroy(g)

    def timer_start(self):
        self._ck(self.L.havoc_mi355x_timer_start(self.h))

    def timer_stop_ms(self):
        ms = C.c_float()
        self._ck(self.L.havoc_mi355x_timer_stop_ms(self.h, C.byref(ms)))
        return ms.value

    def up(self, a):
        """numpy -> device tensor (uint16 travels as int16 bits: torch has no uint16 arithmetic, none is needed)"""
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint16:
            a = a.view(np.int16)
        if a.dtype == np.uint32:
            a = a.view(np.int32)
        with self.torch.cuda.stream(self.tstream):   # ordered with the kernels: same stream
            return self.torch.from_numpy(a).to(self.device)

    def zeros(self, n, dtype):
        t = {np.uint8: self.torch.uint8, np.uint16: self.torch.int16, np.int16: self.torch.int16,
             np.int32: self.torch.int32, np.uint32: self.torch.int32}[np.dtype(dtype).type]
        with self.torch.cuda.stream(self.tstream):
            return self.torch.zeros(int(n), dtype=t, device=self.device)

    def down(self, t, dtype):
        with self.torch.cuda.stream(self.tstream):   # the copy queues behind the kernels that produced `t`
            a = t.cpu().numpy()
        return a.view(dtype) if a.dtype != np.dtype(dtype) else a

    @staticmethod
    def _S(t):
        return t.element_size()

    # ---------------------------------------------------------------- device-level API (tensors in HBM)
    def sad_d(self, src, ss, ref, rs, jobs, out):
        self._ck(self.L.havoc_mi355x_sad(self.h, self._S(src), _ptr(src), ss, _ptr(ref), rs, _ptr(jobs), jobs.shape[0], _ptr(out)))

    def sad_surface_d(self, src, ss, ref, rs, rng, max_w, max_h, jobs, out):
        self._ck(self.L.havoc_mi355x_sad_surface(self.h, self._S(src), rng, max_w, max_h, _ptr(src), ss, _ptr(ref), rs, _ptr(jobs),
                                                 jobs.shape[0], _ptr(out)))

    def pad_block_d(self, plane, origin, w, h, stride, pad, top=True, bottom=True, left=True, right=True):
        self._ck(self.L.havoc_mi355x_pad_block(self.h, self._S(plane), _ptr(plane), origin, w, h, stride, pad, int(top), int(bottom), int(left),
                                               int(right)))

    def pad_block(self, plane, origin, w, h, stride, pad, top=True, bottom=True, left=True, right=True):
        d = self.up(plane)
        self.pad_block_d(d, origin, w, h, stride, pad, top, bottom, left, right)
        return self.down(d, plane.dtype)

    def deblock_d(self, bd, luma, luma_off, sy, chroma, cb_off, cr_off, sc, width, height, data, bs, tc2=0, beta2=0, cb_qp=0, cr_qp=0):
        """in place; luma / chroma = device tensors, *_off = element offset of sample (0, 0) of each plane"""
        S = self._S(luma)
        self._ck(self.L.havoc_mi355x_deblock(self.h, S, bd, luma.data_ptr() + luma_off * S, sy, chroma.data_ptr() + cb_off * S,
                                             chroma.data_ptr() + cr_off * S, sc, width, height, _ptr(data), _ptr(bs), tc2, beta2, cb_qp, cr_qp))

    def deblock(self, bd, luma, sy, cb, cr, sc, width, height, data, bs, tc2=0, beta2=0, cb_qp=0, cr_qp=0):
        """numpy level: planes WITHOUT padding (stride = row length); returns the three filtered planes"""
        y = self.up(luma)
        c = self.up(np.concatenate([cb.ravel(), cr.ravel()]))
        d = self.torch.from_numpy(np.ascontiguousarray(data, np.int8)).to(self.device)
        b = self.torch.from_numpy(np.ascontiguousarray(bs, np.uint8)).to(self.device)
        self.deblock_d(bd, y, 0, sy, c, 0, cb.size, sc, width, height, d, b, tc2, beta2, cb_qp, cr_qp)
        o = self.down(c, cb.dtype)
        return self.down(y, luma.dtype), o[:cb.size].reshape(cb.shape), o[cb.size:].reshape(cr.shape)

    def derive_bs_d(self, cells, cells_stride, width, height, data, bs):
        """cells: uint8 tensor holding CELL_DT records (cells_stride cells per row); data int8 / bs uint8 tensors of the region grid"""
        self._ck(self.L.havoc_mi355x_derive_bs(self.h, _ptr(cells), cells_stride, width, height, _ptr(data), _ptr(bs)))

    def derive_bs(self, cells, width, height):
        """numpy level: cells CELL_DT [height / 4, width / 4] -> (block_data int8, block_bs uint8) flat arrays of the region grid"""
        import torch
        cells = np.ascontiguousarray(cells)
        n = ((width + 63) // 64 * 8 + 1) * ((height + 63) // 64 * 8 + 1)
        with torch.cuda.stream(self.tstream):
            d_cells = torch.from_numpy(cells.view(np.uint8).reshape(-1)).to(self.device)
            data = torch.zeros(n, dtype=torch.int8, device=self.device)
            bs = torch.zeros(n, dtype=torch.uint8, device=self.device)
        self.derive_bs_d(d_cells, cells.shape[1], width, height, data, bs)
        with torch.cuda.stream(self.tstream):
            return data.cpu().numpy(), bs.cpu().numpy()

    def sad4_d(self, src, ss, ref, rs, jobs, out):
        self._ck(self.L.havoc_mi355x_sad4(self.h, self._S(src), _ptr(src), ss, _ptr(ref), rs, _ptr(jobs), jobs.shape[0], _ptr(out)))

    def sad4_runs_d(self, src, ss, ref, rs, jobs, runs, out):
        """the same calls by runs (include/havoc_mi355x.h: havoc_mi355x_sad4_runs); runs: int32 tensor [nruns, 8] = havoc_mi355x_sad4_run records"""
        assert runs.shape[1] == 8, "runs: [n, 8] havoc_mi355x_sad4_run records (sad4_make_runs makes them; as_runs widens [n, 2] = (first job, count) pairs)"
        self._ck(self.L.havoc_mi355x_sad4_runs(self.h, self._S(src), _ptr(src), ss, _ptr(ref), rs, _ptr(jobs), jobs.shape[0], _ptr(runs), runs.shape[0], _ptr(out)))

    @staticmethod
    def as_runs(pairs):
        """(first job, count) pairs -> havoc_mi355x_sad4_run records without a box (the kernel then finds each run's box itself)"""
        pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
        runs = np.zeros((len(pairs), 8), np.int32)
        runs[:, :2] = pairs
        return runs

    @staticmethod
    def sad4_make_runs(jobs, max_run=0, stride=None, S=1):
        """host: cut a sad4 job table (int32 [n, 8]) into runs of consecutive calls with equal source block and size -> int32 [nruns, 8] (first job, count, box offset,
        box width, box rows, 0, 0, 0).  stride = the reference plane's row stride in samples: with it every run gets the box of its candidates (and is cut where the box
        would outgrow the kernel's window); without it the runs have no box.  max_run 0 = by block size."""
        L, _ = _load()
        jobs = np.ascontiguousarray(jobs, np.int32)
        runs = np.zeros((max(1, len(jobs)), 8), np.int32)
        n = L.havoc_mi355x_sad4_make_runs(jobs.ctypes.data, len(jobs), max_run, stride if stride is not None else 0, S, runs.ctypes.data)
        if n < 0:
            raise HavocError("havoc_mi355x_sad4_make_runs failed")
        return np.ascontiguousarray(runs[:n])

    def ssd_d(self, a, sa, b, sb, jobs, out):
        self._ck(self.L.havoc_mi355x_ssd(self.h, self._S(a), _ptr(a), sa, _ptr(b), sb, _ptr(jobs), jobs.shape[0], _ptr(out)))

    def satd_d(self, a, sa, b, sb, jobs, out, max_w=64, max_h=64):
        self._ck(self.L.havoc_mi355x_satd(self.h, self._S(a), max_w, max_h, _ptr(a), sa, _ptr(b), sb, _ptr(jobs), jobs.shape[0], _ptr(out)))

    def satd_multi_d(self, a, sa, b, sb, jobs, out, max_w=64, max_h=64):
        self._ck(self.L.havoc_mi355x_satd_multi(self.h, self._S(a), max_w, max_h, _ptr(a), sa, _ptr(b), sb, _ptr(jobs), jobs.shape[0], _ptr(out)))

    def pred_uni_d(self, taps, bd, dst, sd, ref, sr, jobs, max_w=64, max_h=64):
        self._ck(self.L.havoc_mi355x_pred_uni(self.h, self._S(ref), taps, bd, max_w, max_h, _ptr(dst), sd, _ptr(ref), sr, _ptr(jobs), jobs.shape[0]))

    def pred_bi_d(self, taps, bd, dst, sd, ref, sr, jobs, max_w=64, max_h=64):
        self._ck(self.L.havoc_mi355x_pred_bi(self.h, self._S(ref), taps, bd, max_w, max_h, _ptr(dst), sd, _ptr(ref), sr, _ptr(jobs), jobs.shape[0]))

    # ---- job tables made on the device from the decided motion field (kernels_decide.hip: k_merge_jobs, k_pred_jobs, k_merge_decide) ----
    @staticmethod
    def field_layout(pic_width, pic_height, luma_stride, luma_pad, luma_plane_elems, chroma_stride, chroma_pad, chroma_plane_elems, search_range=64):
        return (C.c_int32 * 12)(pic_width, pic_height, search_range, (pic_width + 3) // 4, luma_stride, luma_pad, luma_plane_elems, chroma_stride, chroma_pad, chroma_plane_elems, 0, 0)

    # ---- the transform-tree decision and the block structure on the device (kernels_decide.hip: k_rqt_decide, k_block_cells) ----
    def rqt_decide_d(self, units, zero_at, one_at, sizes, rec_origin, rec_stride, dump_off, rl_q16, out):
        """sizes: numpy uint64 [4, 5] of device addresses (d_cbf, d_ssd, d_stats, d_jobs, d_final) per transform size 4, 8, 16, 32"""
        self._ck(self.L.havoc_mi355x_rqt_decide(self.h, _ptr(units), units.shape[0], _ptr(zero_at), _ptr(one_at), sizes.ctypes.data, int(rec_origin), int(rec_stride), int(dump_off),
                                                int(rl_q16), _ptr(out)))

    def rqt_decide_rated_d(self, units, zero_at, one_at, sizes, rates, rec_origin, rec_stride, dump_off, rl_q16, out):
        """rqt_decide_d with the residual term supplied: rates = numpy uint64 [4] of device addresses, the int64 Q16 rate of candidate j of each transform size
        (residual_rate_d); the d_stats column of `sizes` may be 0"""
        self._ck(self.L.havoc_mi355x_rqt_decide_rated(self.h, _ptr(units), units.shape[0], _ptr(zero_at), _ptr(one_at), sizes.ctypes.data, rates.ctypes.data, int(rec_origin),
                                                      int(rec_stride), int(dump_off), int(rl_q16), _ptr(out)))

    def rqt_decide_tree_d(self, units, zero_at, one_at, sizes, csizes, chroma_at, tree_rates, tree_cbf, rec_origin, rec_stride, dump_off, cb_origin, cr_origin, c_stride,
                          c_dump_off, rl_q16, out, tree_out):
        """the decision over three planes (havoc_mi355x_rqt_decide_tree): sizes / csizes = numpy uint64 [4, 5] of device addresses (luma / chroma candidate tables),
        chroma_at: int32 tensor [n, 4] (RQT_CHROMA_AT_DT), tree_rates / tree_cbf: int64 / int32 tensors [2 n] as tree_rate_d writes them with out_index = 2 * unit +
        depth; out: [n] havoc_mi355x_rqt_choice, tree_out: [n] RQT_TREE_RESULT_DT"""
        self._ck(self.L.havoc_mi355x_rqt_decide_tree(self.h, _ptr(units), units.shape[0], _ptr(zero_at), _ptr(one_at), sizes.ctypes.data, csizes.ctypes.data, _ptr(chroma_at),
                                                     _ptr(tree_rates), _ptr(tree_cbf), int(rec_origin), int(rec_stride), int(dump_off), int(cb_origin), int(cr_origin),
                                                     int(c_stride), int(c_dump_off), int(rl_q16), _ptr(out), _ptr(tree_out)))

    def rqt_decide_units_d(self, units, zero_at, one_at, sizes, csizes, chroma_at, tree_rates, tree_cbf, rl_q16, out, tree_out):
        """rqt_decide_tree_d for units that overlap one another (havoc_mi355x_rqt_decide_units): the same records, no final job records -- the d_stats, d_jobs and
        d_final columns of `sizes` / `csizes` may be 0 -- and units of log2_size 6, which have depth 1 only (four 32x32 luma candidates in sizes[3], four Cb and Cr
        16x16 in csizes[2]; rate and mask at entry 2 i + 1)"""
        self._ck(self.L.havoc_mi355x_rqt_decide_units(self.h, _ptr(units), units.shape[0], _ptr(zero_at), _ptr(one_at), sizes.ctypes.data, csizes.ctypes.data, _ptr(chroma_at),
                                                      _ptr(tree_rates), _ptr(tree_cbf), int(rl_q16), _ptr(out), _ptr(tree_out)))

    def block_cells_add_d(self, width, height, qp, dpb_index0, field, units, decisions, cells):
        """the cells of `units` into cells that keep what they hold elsewhere (havoc_mi355x_block_cells_add)"""
        self._ck(self.L.havoc_mi355x_block_cells_add(self.h, width, height, qp, dpb_index0, _ptr(field), _ptr(units), _ptr(decisions), units.shape[0], _ptr(cells)))

    def block_cells_d(self, width, height, qp, dpb_index0, field, units, decisions, cells):
        self._ck(self.L.havoc_mi355x_block_cells(self.h, width, height, qp, dpb_index0, _ptr(field), _ptr(units), _ptr(decisions), units.shape[0], _ptr(cells)))

    # ---- an intra picture's running state (kernels_decide.hip: k_intra_gather, k_intra_commit) ----
    @staticmethod
    def intra_chain_layout(pic_width, pic_height, stride, pad, cells_per_row, bit_depth, ctb_log2=6, strong_intra_smoothing=1):
        """strong_intra_smoothing: the reference encoder's default (turing/Encoder.cpp:688)"""
        return (C.c_int32 * 8)(pic_width, pic_height, stride, pad, cells_per_row, bit_depth, ctb_log2, int(bool(strong_intra_smoothing)))

    def intra_gather_a(self, S, layout, rec, owner, modes, parts, n, jobs, neighbours, mpm):
        """device ADDRESSES (ints): a level's slice of a size's tables"""
        self._ck(self.L.havoc_mi355x_intra_gather(self.h, S, layout, rec, owner, modes, parts, n, jobs, neighbours, mpm))

    def intra_commit_a(self, S, layout, rec, modes, parts, n, blocks, mode, mode_stride=1):
        self._ck(self.L.havoc_mi355x_intra_commit(self.h, S, layout, rec, modes, parts, n, blocks, mode, mode_stride))

    def merge_jobs_d(self, layout, field, x0, y0, log2, luma_jobs, cb_jobs, cr_jobs, vectors):
        self._ck(self.L.havoc_mi355x_merge_jobs(self.h, layout, _ptr(field), _ptr(x0), _ptr(y0), x0.shape[0], log2, _ptr(luma_jobs), _ptr(cb_jobs), _ptr(cr_jobs), _ptr(vectors)))

    def merge_decide_d(self, satd_y, satd_cb, satd_cr, n, lam_q16, cost, best):
        self._ck(self.L.havoc_mi355x_merge_decide(self.h, _ptr(satd_y), _ptr(satd_cb), _ptr(satd_cr), n, int(lam_q16), _ptr(cost), _ptr(best)))

    def pred_jobs_d(self, layout, field, lst, x0, y0, log2, plane, dst_off, jobs):
        self._ck(self.L.havoc_mi355x_pred_jobs(self.h, layout, _ptr(field), lst, _ptr(x0), _ptr(y0), x0.shape[0], log2, plane, _ptr(dst_off), _ptr(jobs)))

    @staticmethod
    def sort_by_class(jobs, w, h):
        """(jobs reordered so that the four size classes <= 8, 16, 32, 64 follow each other, counts[4], the permutation applied)"""
        big = np.maximum(np.asarray(w), np.asarray(h))
        cls = np.searchsorted([8, 16, 32], big, side="left")
        order = np.argsort(cls, kind="stable")
        counts = np.bincount(cls, minlength=4).astype(np.int32)
        return np.ascontiguousarray(np.asarray(jobs)[order]), counts, order

    def pred_classes_d(self, bi, taps, bd, dst, sd, ref, sr, jobs, counts):
        """all size classes of a (class-sorted) job table in one launch; counts: int32[4]"""
        c = (C.c_int32 * 4)(*[int(v) for v in counts])
        f = self.L.havoc_mi355x_pred_bi_classes if bi else self.L.havoc_mi355x_pred_uni_classes
        self._ck(f(self.h, self._S(ref), taps, bd, _ptr(dst), sd, _ptr(ref), sr, _ptr(jobs), c))

    @staticmethod
    def size_classes(w, h):
        """[(index array, max_w, max_h)]: the four block-size classes the interpolation kernels are instantiated for"""
        big = np.maximum(np.asarray(w), np.asarray(h))
        out = []
        for lo, hi in ((0, 8), (8, 16), (16, 32), (32, 64)):
            idx = np.flatnonzero((big > lo) & (big <= hi))
            if len(idx):
                out.append((idx, hi, hi))
        return out

    def subtract_bi_d(self, bd, dst, sd, pred, sp, src, ss, jobs):
        self._ck(self.L.havoc_mi355x_subtract_bi(self.h, self._S(src), bd, _ptr(dst), sd, _ptr(pred), sp, _ptr(src), ss, _ptr(jobs), jobs.shape[0]))

    def intra_d(self, bd, log2, dst, sd, nb, jobs):
        self._ck(self.L.havoc_mi355x_intra(self.h, self._S(nb), bd, log2, _ptr(dst), sd, _ptr(nb), _ptr(jobs), jobs.shape[0]))

    def search_gate(self, rows_ready=None):
        """havoc_mi355x_search_gate: the picture searches this context launches from now on wait, CTU row by CTU row, for their reference pictures -- rows_ready = an int32
        device tensor of 2 (rows of list 0 / list 1 that are final in the picture and its 16 phase planes, raised on another stream); None removes the gate"""
        self._gate = rows_ready      # (kept alive)
        self._ck(self.L.havoc_mi355x_search_gate(self.h, _ptr(rows_ready) if rows_ready is not None else None))

    def search_temporal_d(self, cands, n_pus):
        """havoc_mi355x_search_temporal: the picture searches this context launches from now on hand every derivation its temporal candidate -- cands = a uint8 device
        tensor of TEMPORAL_CAND_DT [2 * n_pus], index 2 * pu + list, as temporal_candidates_d wrote it for the same units (read, never written; complete in stream order
        before the search); None removes the table (n_pus is then ignored).  Nothing is launched.  Independent of search_gate."""
        self._temporal = cands      # (kept alive)
        self._ck(self.L.havoc_mi355x_search_temporal(self.h, _ptr(cands) if cands is not None else None, int(n_pus)))

    def search_wait_rows(self, work, width, height, ctu_row, gave_up):
        """havoc_mi355x_search_wait_rows: a launch on THIS context's stream that ends when CTU rows 0 .. ctu_row (both lists) of the picture search running over the workspace
        `work` on another stream are done"""
        self._ck(self.L.havoc_mi355x_search_wait_rows(self.h, _ptr(work), width, height, ctu_row, _ptr(gave_up)))

    def search_picture_uni_d(self, S, params, mvp_rate, src, src_origin, src_stride, ref, ref_origin, ref_stride, phase, plane_elems, phase_origin, pus, ctu_first, ctus_x, ctus_y,
                             n_pus, out, out_bi, field, work):
        """havoc_mi355x_search_picture_uni with everything on the device and NOTHING downloaded: asynchronous (d_* = device tensors, params = the ctypes parameter record)"""
        ro, po, mr = (C.c_int64 * 2)(*[int(v) for v in ref_origin]), (C.c_int64 * 2)(*[int(v) for v in phase_origin]), (C.c_int64 * 2)(*[int(v) for v in mvp_rate])
        self._ck(self.L.havoc_mi355x_search_picture_uni(self.h, S, C.byref(params), mr, _ptr(src), int(src_origin), src_stride, _ptr(ref), ro, ref_stride, _ptr(phase), plane_elems, po,
                                                        _ptr(pus), _ptr(ctu_first), ctus_x, ctus_y, n_pus, _ptr(out), _ptr(out_bi) if out_bi is not None else None, _ptr(field),
                                                        _ptr(work), 0))

    def interp_planes_d(self, bd, planes, plane_elems, ref, stride, x0, y0, width, height):
        self._ck(self.L.havoc_mi355x_interp_planes(self.h, self._S(ref), bd, _ptr(planes), plane_elems, _ptr(ref), stride, x0, y0, width, height))

    def interp_planes(self, bd, ref, stride, x0, y0, width, height):
        """numpy level: returns the 16 planes as an array [16, len(ref)] (plane 0 and everything outside the rectangle 0)"""
        planes = self.zeros(16 * len(ref), ref.dtype)
        self.interp_planes_d(bd, planes, len(ref), self.up(ref), stride, x0, y0, width, height)
        return self.down(planes, ref.dtype).reshape(16, -1)

    def subpel_satd_d(self, taps, bd, max_w, max_h, src, ss, ref, sr, jobs, cost):
        self._ck(self.L.havoc_mi355x_subpel_satd(self.h, self._S(ref), taps, bd, max_w, max_h, _ptr(src), ss, _ptr(ref), sr, _ptr(jobs),
                                                 jobs.shape[0], _ptr(cost)))

    def subpel_satd(self, taps, bd, src, ss, ref, sr, jobs):
        """jobs: int32 [n, 8] = (src_off, ref_off, w, h, xFrac, yFrac, 0, 0); one launch per size class"""
        jobs = np.asarray(jobs, np.int32)
        out = np.zeros(len(jobs), np.int32)
        s, r = self.up(src), self.up(ref)
        big = np.maximum(jobs[:, 2], jobs[:, 3])
        for lo, hi in ((0, 8), (8, 16), (16, 32), (32, 64)):
            idx = np.flatnonzero((big > lo) & (big <= hi))
            if len(idx):
                cost = self.zeros(len(idx), np.int32)
                self.subpel_satd_d(taps, bd, hi, hi, s, ss, r, sr, self._jobs(jobs[idx], 8), cost)
                out[idx] = self.down(cost, np.int32)
        return out

    def intra_satd35_d(self, bd, log2, src, ss, nb, jobs, cost):
        self._ck(self.L.havoc_mi355x_intra_satd35(self.h, self._S(src), bd, log2, _ptr(src), ss, _ptr(nb), _ptr(jobs), jobs.shape[0], _ptr(cost)))

    def residual_d(self, res, sres, res_off, src, ss, pred, sp, jobs):
        self._ck(self.L.havoc_mi355x_residual(self.h, self._S(src), _ptr(res), sres, _ptr(res_off), _ptr(src), ss, _ptr(pred), sp, _ptr(jobs), jobs.shape[0]))

    def transform_d(self, bd, tr, log2, coeffs, res, sres, jobs):
        self._ck(self.L.havoc_mi355x_transform(self.h, bd, tr, log2, _ptr(coeffs), _ptr(res), sres, _ptr(jobs), jobs.shape[0]))

    def inverse_transform_d(self, bd, tr, log2, res, coeffs, jobs):
        self._ck(self.L.havoc_mi355x_inverse_transform(self.h, bd, tr, log2, _ptr(res), _ptr(coeffs), _ptr(jobs), jobs.shape[0]))

    def inverse_transform_add_d(self, bd, tr, log2, dst, sd, pred, sp, coeffs, jobs):
        self._ck(self.L.havoc_mi355x_inverse_transform_add(self.h, self._S(pred), bd, tr, log2, _ptr(dst), sd, _ptr(pred), sp, _ptr(coeffs), _ptr(jobs), jobs.shape[0]))

    def tu_forward_d(self, bd, tr, log2, coeffs, src, ss, pred, sp, jobs):
        self._ck(self.L.havoc_mi355x_tu_forward(self.h, self._S(src), bd, tr, log2, _ptr(coeffs), _ptr(src), ss, _ptr(pred), sp, _ptr(jobs), jobs.shape[0]))

    def tu_reconstruct_d(self, bd, tr, log2, scale, shift, rec, sr, pred, sp, src, ss, levels, jobs, ssd):
        self._ck(self.L.havoc_mi355x_tu_reconstruct(self.h, self._S(src), bd, tr, log2, scale, shift, _ptr(rec), sr, _ptr(pred), sp, _ptr(src), ss,
                                                    _ptr(levels), _ptr(jobs), jobs.shape[0], _ptr(ssd)))

    def intra_measure_d(self, bd, log2, coeffs, coeffs_dct, satd, rec0, ssd0, src, ss, pred, sp, jobs, with_satd=True):
        """the 35-mode stage of one intra partition in one launch (csrc/kernels_tu_fused.hip k_intra_measure): per job the tile SATDs, the forward transform
        (DST-VII for 4x4, plus the 4x4 DCT in coeffs_dct), and the reconstruction from zero levels with its SSD"""
        self._ck(self.L.havoc_mi355x_intra_measure(self.h, self._S(src), bd, log2, _ptr(coeffs), _ptr(coeffs_dct) if coeffs_dct is not None else None,
                                                   _ptr(satd) if satd is not None else None, _ptr(rec0), _ptr(ssd0), _ptr(src), ss, _ptr(pred), sp, _ptr(jobs),
                                                   jobs.shape[0], 1 if with_satd else 0))

    def level_stats_d(self, levels, jobs, njobs, out):
        """jobs: int32 [njobs, 2] (offset, count) into `levels`; out: int32 [2 * njobs] (non-zero levels, sum of magnitudes)"""
        self._ck(self.L.havoc_mi355x_level_stats(self.h, _ptr(levels), _ptr(jobs), njobs, _ptr(out)))

    def tu_forward(self, bd, ncoef, src, ss, pred, sp, jobs):
        """jobs: int32 [n, 8] = (coef_off, src_off, pred_off, rec_off, log2, trType, 0, 0)"""
        co = self.zeros(ncoef, np.int16)
        s, p = self.up(src), self.up(pred)
        for log2, tr, sel in self._tu_groups(jobs):
            self.tu_forward_d(bd, tr, log2, co, s, ss, p, sp, self._jobs(sel, 4))
        return self.down(co, np.int16)

    def tu_reconstruct(self, bd, qp, rec_len, sr, pred, sp, src, ss, levels, jobs):
        """de-quantiser parameters from qp as turing/QpState.h:85-86 / Reconstruct.cpp:315; returns (rec, ssd)"""
        jobs = np.asarray(jobs, np.int32)
        rec = self.zeros(rec_len, src.dtype)
        ssd = np.zeros(len(jobs), np.uint32)
        s, p, lv = self.up(src), self.up(pred), self.up(levels)
        for log2, tr in ((2, 1), (2, 0), (3, 0), (4, 0), (5, 0)):
            idx = np.flatnonzero((jobs[:, 4] == log2) & (jobs[:, 5] == tr))
            if len(idx):
                scale, shift = [40, 45, 51, 57, 64, 72][qp % 6] << (qp // 6), log2 - 1 + bd - 8
                o = self.zeros(len(idx), np.uint32)
                self.tu_reconstruct_d(bd, tr, log2, scale, shift, rec, sr, p, sp, s, ss, lv, self._jobs(jobs[idx], 4), o)
                ssd[idx] = self.down(o, np.uint32)
        return self.down(rec, src.dtype), ssd

    def quantize_d(self, dst, src, jobs, cbf):
        self._ck(self.L.havoc_mi355x_quantize(self.h, _ptr(dst), _ptr(src), _ptr(jobs), jobs.shape[0], _ptr(cbf)))

    def quantize_inverse_d(self, dst, src, jobs):
        self._ck(self.L.havoc_mi355x_quantize_inverse(self.h, _ptr(dst), _ptr(src), _ptr(jobs), jobs.shape[0]))

    def quantize_reconstruct_d(self, log2, rec, sr, pred, sp, res, jobs):
        self._ck(self.L.havoc_mi355x_quantize_reconstruct(self.h, log2, _ptr(rec), sr, _ptr(pred), sp, _ptr(res), _ptr(jobs), jobs.shape[0]))

    def sao_stats(self, bd, src, ss, rec, rs, jobs):
        """numpy level: jobs int32 [n, 4] = (src_off, rec_off, w, h) -> int64 [n, 105]"""
        jobs = np.ascontiguousarray(jobs, np.int32)
        with self.torch.cuda.stream(self.tstream):
            out = self.torch.zeros(105 * len(jobs), dtype=self.torch.int64, device=self.device)
        s, r = self.up(src), self.up(rec)
        self._ck(self.L.havoc_mi355x_sao_stats(self.h, self._S(s), bd, _ptr(s), ss, _ptr(r), rs, _ptr(self.up(jobs)), len(jobs), _ptr(out)))
        return self.down(out, np.int64).reshape(-1, 105)

    def sao_band_chroma(self, bd, src, ss, rec, rs, jobs):
        """jobs int32 [n, 8] (src_u, src_v, rec_u, rec_v, w, h, 0, 0) -> int64 [n, 65]: E[32], count[32], band position (EncSao.h:62-109)"""
        torch = self.torch
        jobs = np.ascontiguousarray(jobs, np.int32)
        d_src, d_rec, d_jobs = self.up(src), self.up(rec), self.up(jobs)
        with torch.cuda.stream(self.tstream):
            out = torch.zeros(65 * len(jobs), dtype=torch.int64, device=self.device)
        self._ck(self.L.havoc_mi355x_sao_band_chroma(self.h, self._S(d_src), bd, _ptr(d_src), ss, _ptr(d_rec), rs, _ptr(d_jobs), len(jobs), _ptr(out)))
        with torch.cuda.stream(self.tstream):
            return out.cpu().numpy().reshape(-1, 65)

    def sao_filter(self, bd, dst_like, sd, src, ss, jobs):
        """numpy level: jobs = SAO_JOB_DT array; returns the destination plane (zeros where no job wrote)"""
        jobs = np.ascontiguousarray(jobs, SAO_JOB_DT)
        dst = self.zeros(len(dst_like), dst_like.dtype)
        s = self.up(src)
        with self.torch.cuda.stream(self.tstream):
            j = self.torch.from_numpy(jobs.view(np.uint8).reshape(-1)).to(self.device)
        self._ck(self.L.havoc_mi355x_sao_filter(self.h, self._S(s), bd, _ptr(dst), sd, _ptr(s), ss, _ptr(j), len(jobs)))
        return self.down(dst, dst_like.dtype)

    def sao_workspace(self, nctus):
        """device scratch for one sao_estimate call over `nctus` CTUs (an int64 tensor: 16-byte aligned)"""
        n = int(self.L.havoc_mi355x_sao_workspace(int(nctus)))
        with self.torch.cuda.stream(self.tstream):
            return self.torch.zeros((n + 7) // 8 + 2, dtype=self.torch.int64, device=self.device)

    def sao_estimate_d(self, bd, lambda_q16, flags, src_y, src_c, ssy, ssc, rec_y, rec_c, rsy, rsc, dst_y, dst_c, dsy, dsc, ctus, work, params):
        """device level: ctus = uint8 tensor of SAO_CTU_DT records, params = uint8 tensor of as many SAO_PARAMS_DT records; no
        synchronisation and no allocation (graph capture)"""
        self._ck(self.L.havoc_mi355x_sao_estimate(self.h, self._S(src_y), bd, int(lambda_q16), int(flags), _ptr(src_y), _ptr(src_c), ssy, ssc,
                                                  _ptr(rec_y), _ptr(rec_c), rsy, rsc, _ptr(dst_y), _ptr(dst_c), dsy, dsc,
                                                  _ptr(ctus), ctus.numel() // SAO_CTU_DT.itemsize, _ptr(work), work.numel() * 8, _ptr(params)))

    def sao_estimate(self, bd, lambda_q16, src_y, src_c, rec_y, rec_c, stride_y, stride_c, ctus, flags=3):
        """numpy level: the SAO parameters of every CTU of `ctus` (SAO_CTU_DT; one layout for source, reconstruction and destination,
        e.g. sao_ctu_table) -> (SAO_PARAMS_DT records, filtered luma plane, filtered chroma plane); the destination starts as a copy of
        the reconstruction, so samples outside every CTU keep it"""
        ctus = np.ascontiguousarray(ctus, SAO_CTU_DT)
        torch = self.torch
        sy, sc, ry, rc = self.up(src_y), self.up(src_c), self.up(rec_y), self.up(rec_c)
        with torch.cuda.stream(self.tstream):
            dy, dc = ry.clone(), rc.clone()
            d_ctus = torch.from_numpy(ctus.view(np.uint8).reshape(-1)).to(self.device)
            params = torch.zeros(len(ctus) * SAO_PARAMS_DT.itemsize, dtype=torch.uint8, device=self.device)
        self.sao_estimate_d(bd, lambda_q16, flags, sy, sc, stride_y, stride_c, ry, rc, stride_y, stride_c, dy, dc, stride_y, stride_c, d_ctus,
                            self.sao_workspace(len(ctus)), params)
        return self.down(params, np.uint8).view(SAO_PARAMS_DT), self.down(dy, rec_y.dtype), self.down(dc, rec_c.dtype)

    def sao_decide_workspace(self, nctus):
        """device scratch for one sao_decide call over `nctus` CTUs (an int64 tensor: 16-byte aligned)"""
        n = int(self.L.havoc_mi355x_sao_decide_workspace(int(nctus)))
        with self.torch.cuda.stream(self.tstream):
            return self.torch.zeros((n + 7) // 8 + 2, dtype=self.torch.int64, device=self.device)

    def sao_decide_d(self, bd, lambda_q16, flags, src_y, src_c, ssy, ssc, rec_y, rec_c, rsy, rsc, dst_y, dst_c, dsy, dsc, ctus, ctus_x, params, ctx_merge,
                     ctx_type, work, decisions):
        """device level: ctus = uint8 tensor of SAO_CTU_DT records, params = what sao_estimate_d wrote for them, decisions = uint8 tensor of as
        many SAO_DECISION_DT records; no synchronisation and no allocation (graph capture).  The caller checks `decided` after its own
        synchronisation: 0 means a wait inside the call gave up."""
        self._ck(self.L.havoc_mi355x_sao_decide(self.h, self._S(src_y), bd, int(lambda_q16), int(flags), _ptr(src_y), _ptr(src_c), ssy, ssc,
                                                _ptr(rec_y), _ptr(rec_c), rsy, rsc, _ptr(dst_y), _ptr(dst_c), dsy, dsc, _ptr(ctus),
                                                ctus.numel() // SAO_CTU_DT.itemsize, int(ctus_x), _ptr(params), int(ctx_merge), int(ctx_type), _ptr(work),
                                                work.numel() * 8, _ptr(decisions)))

    def sao_decide(self, bd, lambda_q16, src_y, src_c, rec_y, rec_c, stride_y, stride_c, ctus, ctus_x, ctx_merge, ctx_type, flags=3):
        """numpy level: sao_estimate, then the merge / off decision of every CTU of `ctus` (SAO_CTU_DT in raster order, `ctus_x` per row; one
        layout for source, reconstruction and destination, e.g. sao_ctu_table); flags bit 2 = WPP; ctx_merge / ctx_type: the slice's initial
        context states (sao_context_init).  -> (SAO_DECISION_DT records, SAO_PARAMS_DT estimate records, filtered luma plane, filtered chroma
        plane with the final parameters); raises HavocError if a wait inside the call gave up."""
        ctus = np.ascontiguousarray(ctus, SAO_CTU_DT)
        torch = self.torch
        sy, sc, ry, rc = self.up(src_y), self.up(src_c), self.up(rec_y), self.up(rec_c)
        with torch.cuda.stream(self.tstream):
            dy, dc = ry.clone(), rc.clone()
            d_ctus = torch.from_numpy(ctus.view(np.uint8).reshape(-1)).to(self.device)
            params = torch.zeros(len(ctus) * SAO_PARAMS_DT.itemsize, dtype=torch.uint8, device=self.device)
            decisions = torch.zeros(len(ctus) * SAO_DECISION_DT.itemsize, dtype=torch.uint8, device=self.device)
        self.sao_estimate_d(bd, lambda_q16, flags & 3, sy, sc, stride_y, stride_c, ry, rc, stride_y, stride_c, dy, dc, stride_y, stride_c, d_ctus,
                            self.sao_workspace(len(ctus)), params)
        self.sao_decide_d(bd, lambda_q16, flags, sy, sc, stride_y, stride_c, ry, rc, stride_y, stride_c, dy, dc, stride_y, stride_c, d_ctus, ctus_x,
                          params, ctx_merge, ctx_type, self.sao_decide_workspace(len(ctus)), decisions)
        dec = self.down(decisions, np.uint8).view(SAO_DECISION_DT)
        if len(dec) and not (dec["decided"] == 1).all():
            raise HavocError("sao_decide: a wait on the row above gave up; the decisions are not to be used")
        return dec, self.down(params, np.uint8).view(SAO_PARAMS_DT), self.down(dy, rec_y.dtype), self.down(dc, rec_c.dtype)

    def sao_apply_d(self, bd, flags, width, height, ctb_log2, rec_y, rec_y_off, rec_c, rec_cb_off, rec_cr_off, rsy, rsc, dst_y, dst_y_off, dst_c,
                    dst_cb_off, dst_cr_off, dsy, dsc, decisions, bounds=None, block_data=None, block_stride=0):
        """device level: the in-loop SAO of a picture from the deblocked planes (rec_*) into different ones (dst_*); *_off = element offset
        of sample (0, 0) of each plane; decisions = uint8 tensor of SAO_DECISION_DT records in raster order; bounds = uint8 tensor of
        SAO_BOUNDS_DT records or None (one slice); block_data = int8 tensor of deblocking bytes (row stride block_stride) or None.  No
        synchronisation and no allocation (graph capture)."""
        S = self._S(rec_y)
        self._ck(self.L.havoc_mi355x_sao_apply(self.h, S, bd, int(flags), int(width), int(height), int(ctb_log2), rec_y.data_ptr() + rec_y_off * S,
                                               rec_c.data_ptr() + rec_cb_off * S, rec_c.data_ptr() + rec_cr_off * S, rsy, rsc,
                                               dst_y.data_ptr() + dst_y_off * S, dst_c.data_ptr() + dst_cb_off * S, dst_c.data_ptr() + dst_cr_off * S,
                                               dsy, dsc, _ptr(decisions), _ptr(bounds), _ptr(block_data), int(block_stride)))

    def sao_apply(self, bd, flags, ctb_log2, rec_y, rec_cb, rec_cr, decisions, bounds=None, block_data=None):
        """numpy level: planes WITHOUT padding (2-D, stride = row length), decisions = SAO_DECISION_DT records in raster order, bounds =
        SAO_BOUNDS_DT records (e.g. sao_bounds_table) or None, block_data = 2-D int8 deblocking bytes or None -> the three filtered planes"""
        torch = self.torch
        height, width = rec_y.shape
        c = np.concatenate([rec_cb.ravel(), rec_cr.ravel()])
        ry, rc = self.up(np.ascontiguousarray(rec_y).ravel()), self.up(c)
        with torch.cuda.stream(self.tstream):
            dy, dc = torch.zeros_like(ry), torch.zeros_like(rc)
            d_dec = torch.from_numpy(np.ascontiguousarray(decisions, SAO_DECISION_DT).view(np.uint8).reshape(-1)).to(self.device)
            d_bounds = None if bounds is None else torch.from_numpy(np.ascontiguousarray(bounds, SAO_BOUNDS_DT).view(np.uint8).reshape(-1)).to(self.device)
            d_blk = None if block_data is None else torch.from_numpy(np.ascontiguousarray(block_data, np.int8).ravel()).to(self.device)
        self.sao_apply_d(bd, flags, width, height, ctb_log2, ry, 0, rc, 0, rec_cb.size, width, width // 2, dy, 0, dc, 0, rec_cb.size, width,
                         width // 2, d_dec, d_bounds, d_blk, 0 if block_data is None else block_data.shape[1])
        o = self.down(dc, rec_cb.dtype)
        return self.down(dy, rec_y.dtype).reshape(rec_y.shape), o[:rec_cb.size].reshape(rec_cb.shape), o[rec_cb.size:].reshape(rec_cr.shape)

    def rdoq_workspace(self, njobs):
        """device scratch for one rdoq launch of `njobs` blocks (an int64 tensor: 16-byte aligned)"""
        n = int(self.L.havoc_mi355x_rdoq_workspace(int(njobs)))
        with self.torch.cuda.stream(self.tstream):
            return self.torch.zeros((n + 7) // 8 + 2, dtype=self.torch.int64, device=self.device)

    def rdoq_d(self, bd, log2, dst, src, states, jobs, cbf, work):
        """jobs: uint8 tensor holding RDOQ_JOB_DT records; states: uint8 tensor of 128-byte snapshots; work: rdoq_workspace(njobs)"""
        self._ck(self.L.havoc_mi355x_rdoq(self.h, bd, log2, _ptr(dst), _ptr(src), _ptr(states), _ptr(jobs), jobs.numel() // RDOQ_JOB_DT.itemsize, _ptr(cbf),
                                          _ptr(work), work.numel() * 8))

    def tu_forward_scan_d(self, bd, log2, coeffs, src, ss, pred, sp, jobs, rdoq_jobs, levels, work):
        """tu_forward with the RDOQ scan folded in (16x16 / 32x32): coefficients + RdoqInfo per block in `work`, level blocks zeroed"""
        self._ck(self.L.havoc_mi355x_tu_forward_scan(self.h, self._S(src), bd, log2, _ptr(coeffs), _ptr(src), ss, _ptr(pred), sp, _ptr(jobs), jobs.shape[0],
                                                     _ptr(rdoq_jobs), _ptr(levels), _ptr(work), work.numel() * 8))

    def rdoq_prescanned_d(self, bd, log2, dst, src, states, jobs, cbf, work):
        self._ck(self.L.havoc_mi355x_rdoq_prescanned(self.h, bd, log2, _ptr(dst), _ptr(src), _ptr(states), _ptr(jobs), jobs.numel() // RDOQ_JOB_DT.itemsize,
                                                     _ptr(cbf), _ptr(work), work.numel() * 8))

    def rdoq(self, bd, log2, src, states, jobs):
        """numpy level: src int16 (all blocks), states uint8 [k, 128], jobs RDOQ_JOB_DT array -> (levels int16 like src, cbf int32[njobs])"""
        jobs = np.ascontiguousarray(jobs, RDOQ_JOB_DT)
        dst = self.zeros(len(src), np.int16)
        cbf = self.zeros(len(jobs), np.int32)
        with self.torch.cuda.stream(self.tstream):
            st = self.torch.from_numpy(np.ascontiguousarray(states, np.uint8).reshape(-1)).to(self.device)
            j = self.torch.from_numpy(jobs.view(np.uint8).reshape(-1)).to(self.device)
        self.rdoq_d(bd, log2, dst, self.up(src), st, j, cbf, self.rdoq_workspace(len(jobs)))
        return self.down(dst, np.int16), self.down(cbf, np.int32)

    def residual_rate_d(self, log2, levels, states, jobs, rates, states_out=None):
        """the CABAC rate of residual_coding per block (havoc_mi355x_residual_rate); jobs: uint8 tensor holding RESIDUAL_RATE_JOB_DT records; rates: int64 tensor;
        states_out: None, or a uint8 tensor of 128 bytes per job.  No sync."""
        self._ck(self.L.havoc_mi355x_residual_rate(self.h, log2, _ptr(levels), _ptr(states), _ptr(jobs), jobs.numel() // RESIDUAL_RATE_JOB_DT.itemsize, _ptr(rates),
                                                   _ptr(states_out)))

    def residual_rate(self, log2, levels, states, jobs):
        """numpy level: levels int16 (all blocks), states uint8 [k, 128], jobs RESIDUAL_RATE_JOB_DT array -> (rates int64 [max rate_index + count], the entries no
        job writes 0; states_after uint8 [njobs, 128])"""
        jobs = np.ascontiguousarray(jobs, RESIDUAL_RATE_JOB_DT)
        nr = int((jobs["rate_index"].astype(np.int64) + np.clip(jobs["count"], 1, 4)).max()) if len(jobs) else 0
        with self.torch.cuda.stream(self.tstream):
            st = self.torch.from_numpy(np.ascontiguousarray(states, np.uint8).reshape(-1)).to(self.device)
            j = self.torch.from_numpy(jobs.view(np.uint8).reshape(-1).copy()).to(self.device)
            rates = self.torch.zeros(max(nr, 1), dtype=self.torch.int64, device=self.device)
            after = self.torch.zeros(max(len(jobs), 1) * 128, dtype=self.torch.uint8, device=self.device)
        self.residual_rate_d(log2, self.up(np.ascontiguousarray(levels, np.int16)), st, j, rates, after)
        return self.down(rates, np.int64)[:nr], self.down(after, np.uint8)[:len(jobs) * 128].reshape(-1, 128)

    def intra_rate_d(self, log2, levels, states, syntax_states, jobs, rates, states_out=None, syntax_states_out=None):
        """the CABAC rate of an intra candidate: mode bits, split_transform_flag, cbf_luma, residual_coding (havoc_mi355x_intra_rate); jobs: uint8 tensor holding
        INTRA_RATE_JOB_DT records; syntax_states: uint8 tensor, 4 bytes per snapshot; rates: int64 tensor; the two outputs: None, or 128 / 4 bytes per job.  No sync."""
        self._ck(self.L.havoc_mi355x_intra_rate(self.h, log2, _ptr(levels), _ptr(states), _ptr(syntax_states), _ptr(jobs), jobs.numel() // INTRA_RATE_JOB_DT.itemsize,
                                                _ptr(rates), _ptr(states_out), _ptr(syntax_states_out)))

    def intra_rate(self, log2, levels, states, syntax_states, jobs):
        """numpy level: levels int16 (all blocks), states uint8 [k, 128], syntax_states uint8 [k, 4], jobs INTRA_RATE_JOB_DT array -> (rates int64 [max rate_index + 1],
        the entries no job writes 0; states_after uint8 [njobs, 128]; syntax_states_after uint8 [njobs, 4])"""
        jobs = np.ascontiguousarray(jobs, INTRA_RATE_JOB_DT)
        nr = int(jobs["rate_index"].max()) + 1 if len(jobs) else 0
        with self.torch.cuda.stream(self.tstream):
            st = self.torch.from_numpy(np.ascontiguousarray(states, np.uint8).reshape(-1)).to(self.device)
            sy = self.torch.from_numpy(np.ascontiguousarray(syntax_states, np.uint8).reshape(-1)).to(self.device)
            j = self.torch.from_numpy(jobs.view(np.uint8).reshape(-1).copy()).to(self.device)
            rates = self.torch.zeros(max(nr, 1), dtype=self.torch.int64, device=self.device)
            after = self.torch.zeros(max(len(jobs), 1) * 128, dtype=self.torch.uint8, device=self.device)
            after_sy = self.torch.zeros(max(len(jobs), 1) * INTRA_SYNTAX_CTX_BYTES, dtype=self.torch.uint8, device=self.device)
        self.intra_rate_d(log2, self.up(np.ascontiguousarray(levels, np.int16)), st, sy, j, rates, after, after_sy)
        return (self.down(rates, np.int64)[:nr], self.down(after, np.uint8)[:len(jobs) * 128].reshape(-1, 128),
                self.down(after_sy, np.uint8)[:len(jobs) * INTRA_SYNTAX_CTX_BYTES].reshape(-1, INTRA_SYNTAX_CTX_BYTES))

    def tree_rate_d(self, log2_cb, depth, luma_levels, chroma_levels, states, syntax_states, jobs, rates, cbf, states_out=None, syntax_states_out=None):
        """the CABAC rate of an inter unit's whole transform tree at one depth: split_transform_flag, cbf_cb, cbf_cr, cbf_luma and the Y, Cb, Cr residual_coding
        (havoc_mi355x_tree_rate); jobs: uint8 tensor holding TREE_RATE_JOB_DT records; rates: int64 tensor; cbf: int32 tensor (the masks); the two outputs: None, or
        128 / 4 bytes per job.  log2_cb 3..5 at depth 0 or 1; 6 at depth 1 only (a 64x64 unit's one tree, its split inferred: no flag bin, and a job that claims
        one is refused with rate -1).  No sync."""
        self._ck(self.L.havoc_mi355x_tree_rate(self.h, log2_cb, depth, _ptr(luma_levels), _ptr(chroma_levels), _ptr(states), _ptr(syntax_states), _ptr(jobs),
                                               jobs.numel() // TREE_RATE_JOB_DT.itemsize, _ptr(rates), _ptr(cbf), _ptr(states_out), _ptr(syntax_states_out)))

    def tree_rate(self, log2_cb, depth, luma_levels, chroma_levels, states, syntax_states, jobs):
        """numpy level: the levels int16, states uint8 [k, 128], syntax_states uint8 [k, 4], jobs TREE_RATE_JOB_DT array -> (rates int64 and masks uint32
        [max out_index + 1], the entries no job writes 0; states_after uint8 [njobs, 128]; syntax_states_after uint8 [njobs, 4])"""
        jobs = np.ascontiguousarray(jobs, TREE_RATE_JOB_DT)
        nr = int(jobs["out_index"].max()) + 1 if len(jobs) else 0
        with self.torch.cuda.stream(self.tstream):
            st = self.torch.from_numpy(np.ascontiguousarray(states, np.uint8).reshape(-1)).to(self.device)
            sy = self.torch.from_numpy(np.ascontiguousarray(syntax_states, np.uint8).reshape(-1)).to(self.device)
            j = self.torch.from_numpy(jobs.view(np.uint8).reshape(-1).copy()).to(self.device)
            rates = self.torch.zeros(max(nr, 1), dtype=self.torch.int64, device=self.device)
            cbf = self.torch.zeros(max(nr, 1), dtype=self.torch.int32, device=self.device)
            after = self.torch.zeros(max(len(jobs), 1) * 128, dtype=self.torch.uint8, device=self.device)
            after_sy = self.torch.zeros(max(len(jobs), 1) * INTRA_SYNTAX_CTX_BYTES, dtype=self.torch.uint8, device=self.device)
        self.tree_rate_d(log2_cb, depth, self.up(np.ascontiguousarray(luma_levels, np.int16)), self.up(np.ascontiguousarray(chroma_levels, np.int16)), st, sy, j, rates, cbf,
                         after, after_sy)
        return (self.down(rates, np.int64)[:nr], self.down(cbf, np.int32)[:nr].view(np.uint32), self.down(after, np.uint8)[:len(jobs) * 128].reshape(-1, 128),
                self.down(after_sy, np.uint8)[:len(jobs) * INTRA_SYNTAX_CTX_BYTES].reshape(-1, INTRA_SYNTAX_CTX_BYTES))

    def pu_rate_d(self, syntax_states, jobs, slice_params, rates, syntax_out=None):
        """the CABAC rate of every candidate of prediction units: Syntax<prediction_unit> under Measure<void> (havoc_mi355x_pu_rate); syntax_states: uint8 tensor, 16
        bytes per snapshot; jobs: uint8 tensor holding PU_RATE_JOB_DT records; slice_params: PuSlice; rates: int64 tensor; syntax_out: None, or 16 bytes per job.  No sync."""
        self._ck(self.L.havoc_mi355x_pu_rate(self.h, _ptr(syntax_states), _ptr(jobs), jobs.numel() // PU_RATE_JOB_DT.itemsize, C.addressof(slice_params), _ptr(rates),
                                             _ptr(syntax_out)))

    def pu_rate(self, syntax_states, jobs, slice_params):
        """numpy level: syntax_states uint8 [k, 16], jobs PU_RATE_JOB_DT array -> (rates int64 [max out_index + 1], the entries no job writes 0; the snapshots after,
        uint8 [njobs, 16])"""
        jobs = np.ascontiguousarray(jobs, PU_RATE_JOB_DT)
        nr = int(jobs["out_index"].max()) + 1 if len(jobs) else 0
        with self.torch.cuda.stream(self.tstream):
            sy = self.torch.from_numpy(np.ascontiguousarray(syntax_states, np.uint8).reshape(-1)).to(self.device)
            j = self.torch.from_numpy(jobs.view(np.uint8).reshape(-1).copy()).to(self.device) if len(jobs) else self.torch.zeros(32, dtype=self.torch.uint8, device=self.device)
            rates = self.torch.zeros(max(nr, 1), dtype=self.torch.int64, device=self.device)
            after = self.torch.zeros(max(len(jobs), 1) * PU_SYNTAX_CTX_BYTES, dtype=self.torch.uint8, device=self.device)
        self._ck(self.L.havoc_mi355x_pu_rate(self.h, _ptr(sy), _ptr(j), len(jobs), C.addressof(slice_params), _ptr(rates), _ptr(after)))
        return self.down(rates, np.int64)[:nr], self.down(after, np.uint8)[:len(jobs) * PU_SYNTAX_CTX_BYTES].reshape(-1, PU_SYNTAX_CTX_BYTES)

    def pu_decide_d(self, first, count, n, rates, satd_y, satd_cb, satd_cr, lam_q16, syntax_after, cost, best, best_cost, best_syntax=None):
        """go2's comparison of n prediction units over their contiguous candidates (havoc_mi355x_pu_decide): first / count / best: int32 tensors [n]; rates / cost:
        int64 tensors per candidate; best_cost: int64 [n]; syntax_after / best_syntax: uint8, 16 bytes per candidate / unit, or None.  No sync."""
        self._ck(self.L.havoc_mi355x_pu_decide(self.h, _ptr(first), _ptr(count), n, _ptr(rates), _ptr(satd_y), _ptr(satd_cb), _ptr(satd_cr), int(lam_q16),
                                               _ptr(syntax_after), _ptr(cost), _ptr(best), _ptr(best_cost), _ptr(best_syntax)))

    def pu_decide(self, first, count, rates, satd_y, satd_cb, satd_cr, lam_q16, syntax_after):
        """numpy level -> (cost int64 per candidate, best int32 [n], best_cost int64 [n], best_syntax uint8 [n, 16])"""
        n, m = len(first), len(rates)
        t = self.torch
        with t.cuda.stream(self.tstream):
            up = lambda a, dt: t.from_numpy(np.ascontiguousarray(a, dt).reshape(-1)).to(self.device) if np.size(a) else t.zeros(16, dtype=getattr(t, np.dtype(dt).name), device=self.device)
            f, c, r = up(first, np.int32), up(count, np.int32), up(rates, np.int64)
            sy, scb, scr, sa = up(satd_y, np.int32), up(satd_cb, np.int32), up(satd_cr, np.int32), up(syntax_after, np.uint8)
            cost = t.zeros(max(m, 1), dtype=t.int64, device=self.device)
            best = t.zeros(max(n, 1), dtype=t.int32, device=self.device)
            best_cost = t.zeros(max(n, 1), dtype=t.int64, device=self.device)
            best_syntax = t.zeros(max(n, 1) * PU_SYNTAX_CTX_BYTES, dtype=t.uint8, device=self.device)
        self.pu_decide_d(f, c, n, r, sy, scb, scr, lam_q16, sa, cost, best, best_cost, best_syntax)
        return (self.down(cost, np.int64)[:m], self.down(best, np.int32)[:n], self.down(best_cost, np.int64)[:n],
                self.down(best_syntax, np.uint8)[:n * PU_SYNTAX_CTX_BYTES].reshape(-1, PU_SYNTAX_CTX_BYTES))

    def cu_close_d(self, cu_syntax, pu_before, pu_after, pu_rate, choice, tree_choice, tree_rate, pred_ssd, jobs, max_num_merge_cand, lam_q16, out, cu_syntax_out,
                   pu_syntax_out):
        """closes candidate inter coding units (havoc_mi355x_cu_close): the CU's own CABAC bits and the reference's residual / no-residual / skip decision over what
        rqt_decide_tree (choice: RQT_RESULT records, tree_choice: RQT_TREE_RESULT_DT, tree_rate int64 [2 units]), pu_rate (pu_rate int64, pu_after) and unit_pred_ssd
        (pred_ssd int32 [3 units]) left on the device; jobs: uint8 tensor of CU_CLOSE_JOB_DT; out: uint8 tensor of CU_CHOICE_DT; the snapshots uint8, 16 bytes each.  No sync."""
        self._ck(self.L.havoc_mi355x_cu_close(self.h, _ptr(cu_syntax), _ptr(pu_before), _ptr(pu_after), _ptr(pu_rate), _ptr(choice), _ptr(tree_choice), _ptr(tree_rate),
                                              _ptr(pred_ssd), _ptr(jobs), jobs.numel() // CU_CLOSE_JOB_DT.itemsize, int(max_num_merge_cand), int(lam_q16), _ptr(out),
                                              _ptr(cu_syntax_out), _ptr(pu_syntax_out)))

    def cu_close(self, cu_syntax, pu_before, pu_after, pu_rate, choice, tree_choice, tree_rate, pred_ssd, jobs, max_num_merge_cand, lam_q16):
        """numpy level: the inputs as arrays (choice: 104-byte records as uint8 [n, 104] or a structured array) -> (CU_CHOICE_DT [njobs], cu snapshots uint8 [njobs, 16],
        pu snapshots uint8 [njobs, 16])"""
        t = self.torch
        jobs = np.ascontiguousarray(jobs, CU_CLOSE_JOB_DT)
        n = len(jobs)
        with t.cuda.stream(self.tstream):
            up = lambda a: t.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(self.device) if np.size(a) else t.zeros(128, dtype=t.uint8, device=self.device)
            ins = [up(a) for a in (cu_syntax, pu_before, pu_after, pu_rate, choice, tree_choice, tree_rate, pred_ssd)]
            j = up(jobs)
            out = t.zeros(max(n, 1) * CU_CHOICE_DT.itemsize, dtype=t.uint8, device=self.device)
            cu_out = t.zeros(max(n, 1) * 16, dtype=t.uint8, device=self.device)
            pu_out = t.zeros(max(n, 1) * 16, dtype=t.uint8, device=self.device)
        self._ck(self.L.havoc_mi355x_cu_close(self.h, *[_ptr(a) for a in ins], _ptr(j), n, int(max_num_merge_cand), int(lam_q16), _ptr(out), _ptr(cu_out), _ptr(pu_out)))
        return (self.down(out, np.uint8)[:n * 48].view(CU_CHOICE_DT).copy(), self.down(cu_out, np.uint8)[:n * 16].reshape(-1, 16), self.down(pu_out, np.uint8)[:n * 16].reshape(-1, 16))

    def cqt_decide_workspace(self, n_ctus):
        """device scratch for one cqt_decide call over `n_ctus` CTUs (an int64 tensor: 8-byte aligned); the call resets it itself"""
        n = int(self.L.havoc_mi355x_cqt_decide_workspace(int(n_ctus)))
        with self.torch.cuda.stream(self.tstream):
            return self.torch.zeros((n + 7) // 8, dtype=self.torch.int64, device=self.device)

    def cqt_decide_d(self, width, height, ctb_log2, min_cb_log2, flags, cu_syntax, node_cu, choice, work, ctu, node, depth, cu_syntax_out):
        """the coding quadtree of every CTU (havoc_mi355x_cqt_decide) over cu_close's records, read in place: cu_syntax uint8 [16] (the slice's initial snapshot),
        node_cu int32 [n_ctus * cqt_nodes] (the index in `choice` of each node's candidate, -1: none), choice: uint8 tensor of CU_CHOICE_DT; outputs: uint8 tensors of
        CQT_CTU_DT [n_ctus] and CQT_NODE_DT [n_ctus * cqt_nodes], the CtDepth map int8 (whole CTUs, a byte per MinCb cell), the snapshots uint8 [n_ctus * 16].  No sync."""
        self._ck(self.L.havoc_mi355x_cqt_decide(self.h, int(width), int(height), int(ctb_log2), int(min_cb_log2), int(flags), _ptr(cu_syntax), _ptr(node_cu), _ptr(choice),
                                                choice.numel() * choice.element_size() // CU_CHOICE_DT.itemsize, _ptr(work), work.numel() * work.element_size(),
                                                _ptr(ctu), _ptr(node), _ptr(depth), _ptr(cu_syntax_out)))

    def cqt_buffers(self, width, height, ctb_log2, min_cb_log2):
        """-> dict(work, ctu, node, depth, cu_syntax_out): the workspace and zeroed outputs of cqt_decide_d for a picture"""
        t = self.torch
        cx, cy, cells = -(-width >> ctb_log2), -(-height >> ctb_log2), 1 << (ctb_log2 - min_cb_log2)
        n, nodes = cx * cy, cqt_nodes(ctb_log2, min_cb_log2)
        with t.cuda.stream(self.tstream):
            z = lambda k: t.zeros(k, dtype=t.uint8, device=self.device)
            return dict(work=self.cqt_decide_workspace(n), ctu=z(n * CQT_CTU_DT.itemsize), node=z(n * nodes * CQT_NODE_DT.itemsize),
                        depth=t.zeros(n * cells * cells, dtype=t.int8, device=self.device), cu_syntax_out=z(n * CU_SYNTAX_CTX_BYTES))

    def cqt_download(self, B, width, height, ctb_log2, min_cb_log2):
        """the outputs in cqt_buffers' dict as numpy: dict(ctus CQT_CTU_DT [n], nodes CQT_NODE_DT [n, cqt_nodes], depth int8 [rows, cells per row], cu_syntax [n, 16])"""
        cx, cy, cells = -(-width >> ctb_log2), -(-height >> ctb_log2), 1 << (ctb_log2 - min_cb_log2)
        return dict(ctus=self.down(B["ctu"], np.uint8).view(CQT_CTU_DT).copy(),
                    nodes=self.down(B["node"], np.uint8).view(CQT_NODE_DT).reshape(cx * cy, cqt_nodes(ctb_log2, min_cb_log2)).copy(),
                    depth=self.down(B["depth"], np.int8).reshape(cy * cells, cx * cells), cu_syntax=self.down(B["cu_syntax_out"], np.uint8).reshape(-1, CU_SYNTAX_CTX_BYTES))

    def cqt_decide(self, width, height, ctb_log2, min_cb_log2, flags, cu_syntax, node_cu, choice):
        """numpy level: cu_syntax uint8 [16], node_cu int32 [n_ctus, cqt_nodes], choice CU_CHOICE_DT [m] -> cqt_download's dict"""
        t = self.torch
        with t.cuda.stream(self.tstream):
            up = lambda a: t.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(self.device) if np.size(a) else t.zeros(64, dtype=t.uint8, device=self.device)
            ins = [up(np.asarray(cu_syntax, np.uint8)), up(np.asarray(node_cu, np.int32)), up(np.ascontiguousarray(choice, CU_CHOICE_DT))]
        B = self.cqt_buffers(width, height, ctb_log2, min_cb_log2)
        self.cqt_decide_d(width, height, ctb_log2, min_cb_log2, flags, ins[0], ins[1], ins[2], B["work"], B["ctu"], B["node"], B["depth"], B["cu_syntax_out"])
        return self.cqt_download(B, width, height, ctb_log2, min_cb_log2)

    def cqt_commit_d(self, bit_depth, width, height, ctb_log2, min_cb_log2, units, node_cu, ctu, node, cu, choice, tree_choice, zero_at, one_at, chroma_at, luma_pieces,
                     chroma_pieces, pred_y, pred_stride, pred_c, pred_stride_c, pred_off, best, unit_cand, cand_mv, rec_y, rec_origin, rec_stride, rec_c, cb_origin,
                     cr_origin, c_stride, cells):
        """the decided quadtree's final coding units into one picture and one CQT_CELL_DT record per MinCb cell (havoc_mi355x_cqt_commit), over what the calls before
        left on the device, read in place: units int32 [n, 4]; node_cu, ctu, node: cqt_decide_d's; cu: cu_close_d's records; choice, tree_choice, zero_at, one_at,
        chroma_at: rqt_decide_units_d's; luma_pieces / chroma_pieces: 4 / 3 tensors or None (transform sizes 2..5 / 2..4); pred_y, pred_c, pred_off int32 [n, 3]: the
        unit prediction planes and each unit's block in them; best, unit_cand int32 [n]; cand_mv int16 [candidates, 2, 2] or None; cells: uint8 tensor of
        (height >> min_cb_log2) * (width >> min_cb_log2) records.  No sync."""
        a = CqtCommitArgs()
        a.bit_depth, a.width, a.height, a.ctb_log2, a.min_cb_log2, a.n = int(bit_depth), int(width), int(height), int(ctb_log2), int(min_cb_log2), units.numel() // 4
        for k, t in (("d_units", units), ("d_node_cu", node_cu), ("d_ctu", ctu), ("d_node", node), ("d_cu", cu), ("d_choice", choice), ("d_tree_choice", tree_choice),
                     ("d_zero_at", zero_at), ("d_one_at", one_at), ("d_chroma_at", chroma_at), ("d_pred_y", pred_y), ("d_pred_c", pred_c), ("d_pred_off", pred_off),
                     ("d_best", best), ("d_unit_cand", unit_cand), ("d_cand_mv", cand_mv), ("d_rec_y", rec_y), ("d_rec_c", rec_c), ("d_cells", cells)):
            setattr(a, k, _ptr(t))
        a.luma_pieces = (_vp * 4)(*[_ptr(t) for t in luma_pieces])
        a.chroma_pieces = (_vp * 3)(*[_ptr(t) for t in chroma_pieces])
        a.pred_stride, a.pred_stride_c, a.rec_stride, a.c_stride = int(pred_stride), int(pred_stride_c), int(rec_stride), int(c_stride)
        a.rec_origin, a.cb_origin, a.cr_origin = int(rec_origin), int(cb_origin), int(cr_origin)
        self._ck(self.L.havoc_mi355x_cqt_commit(self.h, C.addressof(a)))

    def cqt_cells_download(self, cells, width, height, min_cb_log2):
        """cqt_commit_d's cell map as numpy: CQT_CELL_DT [height >> min_cb_log2, width >> min_cb_log2]"""
        hc, wc = height >> min_cb_log2, width >> min_cb_log2
        return self.down(cells, np.uint8)[:hc * wc * CQT_CELL_DT.itemsize].view(CQT_CELL_DT).reshape(hc, wc).copy()

    def cqt_block_cells_d(self, width, height, min_cb_log2, qp, dpb0, dpb1, cqt_cells, cells, cells_stride):
        """cqt_commit_d's cell map as the (height / 4) x (width / 4) map of CELL_DT records derive_bs_d reads, rows cells_stride cells apart, every cell written
        (havoc_mi355x_cqt_block_cells); cqt_cells, cells: uint8 tensors.  No sync."""
        self._ck(self.L.havoc_mi355x_cqt_block_cells(self.h, int(width), int(height), int(min_cb_log2), int(qp), int(dpb0), int(dpb1), _ptr(cqt_cells), _ptr(cells),
                                                     int(cells_stride)))

    def cqt_block_cells(self, cqt_cells, width, height, min_cb_log2, qp, dpb0, dpb1):
        """numpy level: cqt_cells CQT_CELL_DT [height >> min_cb_log2, width >> min_cb_log2] -> CELL_DT [height / 4, width / 4]"""
        import torch
        cqt_cells = np.ascontiguousarray(cqt_cells, CQT_CELL_DT)
        with torch.cuda.stream(self.tstream):
            d_cqt = torch.from_numpy(cqt_cells.view(np.uint8).reshape(-1).copy()).to(self.device)
            d_cells = torch.zeros((height // 4) * (width // 4) * CELL_DT.itemsize, dtype=torch.uint8, device=self.device)
        self.cqt_block_cells_d(width, height, min_cb_log2, qp, dpb0, dpb1, d_cqt, d_cells, width // 4)
        return self.down(d_cells, np.uint8).view(CELL_DT).reshape(height // 4, width // 4).copy()

    def cqt_motion_store_d(self, width, height, min_cb_log2, poc, ref_poc0, ref_poc1, cqt_cells, store):
        """cqt_commit_d's cell map as the collocated motion store: (height + 15) // 16 dense rows of (width + 15) // 16 COL_CELL_DT records, every one written
        (havoc_mi355x_cqt_motion_store); cqt_cells, store: uint8 tensors.  No sync."""
        self._ck(self.L.havoc_mi355x_cqt_motion_store(self.h, int(width), int(height), int(min_cb_log2), int(poc), int(ref_poc0), int(ref_poc1), _ptr(cqt_cells),
                                                      _ptr(store)))

    def temporal_candidates_d(self, params, store, store_stride, pus, n, out):
        """the temporal candidate of n prediction units per list (havoc_mi355x_temporal_candidates): params: one TEMPORAL_PARAMS_DT record (read during the call);
        store: uint8 tensor of COL_CELL_DT rows store_stride records apart; pus: uint8 tensor of workload.PICTURE_PU_DT [n]; out: uint8 tensor of TEMPORAL_CAND_DT
        [2 n], index 2 * pu + list.  No sync."""
        params = np.ascontiguousarray(params, TEMPORAL_PARAMS_DT).reshape(1)
        self._ck(self.L.havoc_mi355x_temporal_candidates(self.h, params.ctypes.data, _ptr(store), int(store_stride), _ptr(pus), int(n), _ptr(out)))

    def cqt_merge_lists_d(self, params, cqt_cells, pus, n, temporal, out):
        """the merge candidate list of every final coding unit of a committed picture (havoc_mi355x_cqt_merge_lists): params: one MERGE_PARAMS_DT record (read during
        the call); cqt_cells: cqt_commit_d's cell map; pus: uint8 tensor of workload.PICTURE_PU_DT [n]; temporal: uint8 tensor of TEMPORAL_CAND_DT [2 * n] as
        temporal_candidates_d wrote it for the same units, or None (no temporal candidate); out: uint8 tensor of MERGE_LIST_DT [n], every record written.  No sync."""
        params = np.ascontiguousarray(params, MERGE_PARAMS_DT).reshape(1)
        self._ck(self.L.havoc_mi355x_cqt_merge_lists(self.h, params.ctypes.data, _ptr(cqt_cells), _ptr(pus), int(n), None if temporal is None else _ptr(temporal),
                                                     _ptr(out)))

    def cqt_merge_lists_download(self, out, n):
        """cqt_merge_lists_d's records as numpy: MERGE_LIST_DT [n]"""
        return self.down(out, np.uint8)[:n * MERGE_LIST_DT.itemsize].view(MERGE_LIST_DT).copy()

    def unit_pred_ssd_d(self, bit_depth, src_y, src_stride, src_c, src_stride_c, pred_y, pred_stride, pred_c, pred_stride_c, jobs, out):
        """SSD(source, prediction) of units' luma, Cb and Cr blocks in one launch (havoc_mi355x_unit_pred_ssd); jobs: uint8 tensor of PRED_SSD_JOB_DT; out: int32 [3 n].
        No sync."""
        self._ck(self.L.havoc_mi355x_unit_pred_ssd(self.h, bit_depth, _ptr(src_y), src_stride, _ptr(src_c), src_stride_c, _ptr(pred_y), pred_stride, _ptr(pred_c),
                                                   pred_stride_c, _ptr(jobs), jobs.numel() // PRED_SSD_JOB_DT.itemsize, _ptr(out)))

    def unit_pred_ssd(self, bit_depth, src_y, src_stride, src_c, src_stride_c, pred_y, pred_stride, pred_c, pred_stride_c, jobs):
        """numpy level: the four sample arrays (uint8, or uint16 above 8 bits) and PRED_SSD_JOB_DT jobs -> int32 [n, 3]"""
        t, dt = self.torch, np.uint8 if bit_depth == 8 else np.uint16
        jobs = np.ascontiguousarray(jobs, PRED_SSD_JOB_DT)
        n = len(jobs)
        with t.cuda.stream(self.tstream):
            up = lambda a: t.from_numpy(np.ascontiguousarray(a, dt).reshape(-1).view(np.uint8).copy()).to(self.device)
            planes = [up(a) for a in (src_y, src_c, pred_y, pred_c)]
            j = t.from_numpy(jobs.view(np.uint8).reshape(-1).copy()).to(self.device) if n else t.zeros(32, dtype=t.uint8, device=self.device)
            out = t.zeros(3 * max(n, 1), dtype=t.int32, device=self.device)
        self._ck(self.L.havoc_mi355x_unit_pred_ssd(self.h, bit_depth, _ptr(planes[0]), src_stride, _ptr(planes[1]), src_stride_c, _ptr(planes[2]), pred_stride,
                                                   _ptr(planes[3]), pred_stride_c, _ptr(j), n, _ptr(out)))
        return self.down(out, np.int32)[:3 * n].reshape(-1, 3)

    def unit_pred_select_d(self, bit_depth, cand_y, cand_c, dst_y, dst_stride, dst_c, dst_stride_c, first, best, rate, jobs, unit_rate, unit_cand):
        """the winning candidate's Y, Cb and Cr block of every unit out of the candidate buffers into prediction planes, and the winner's rate and candidate index
        (havoc_mi355x_unit_pred_select); first / best: int32 tensors and rate: int64 tensor as pu_decide_d / pu_rate_d leave them; jobs: uint8 tensor of
        PRED_SELECT_JOB_DT; unit_rate: int64, unit_cand: int32, per unit.  No sync."""
        self._ck(self.L.havoc_mi355x_unit_pred_select(self.h, bit_depth, _ptr(cand_y), _ptr(cand_c), _ptr(dst_y), dst_stride, _ptr(dst_c), dst_stride_c, _ptr(first),
                                                      _ptr(best), _ptr(rate), _ptr(jobs), jobs.numel() // PRED_SELECT_JOB_DT.itemsize, _ptr(unit_rate), _ptr(unit_cand)))

    def unit_pred_select(self, bit_depth, cand_y, cand_c, dst_y, dst_stride, dst_c, dst_stride_c, first, best, rate, jobs):
        """numpy level: the candidate buffers and the destination planes as they are before (uint8, or uint16 above 8 bits), first / best int32 and rate int64 per
        unit / candidate, PRED_SELECT_JOB_DT jobs -> (the luma planes after, the chroma planes after, unit_rate int64, unit_cand int32 [len(best)], the entries no
        job names 0)"""
        t, dt = self.torch, np.uint8 if bit_depth == 8 else np.uint16
        jobs = np.ascontiguousarray(jobs, PRED_SELECT_JOB_DT)
        n, nu = len(jobs), len(best)
        with t.cuda.stream(self.tstream):
            up = lambda a, d: t.from_numpy(np.ascontiguousarray(a, d).reshape(-1).view(np.uint8).copy()).to(self.device)
            planes = [up(a, dt) for a in (cand_y, cand_c, dst_y, dst_c)]
            d_first, d_best, d_rate = up(first, np.int32), up(best, np.int32), up(rate, np.int64)
            j = up(jobs.view(np.uint8), np.uint8) if n else t.zeros(32, dtype=t.uint8, device=self.device)
            unit_rate, unit_cand = t.zeros(max(nu, 1), dtype=t.int64, device=self.device), t.zeros(max(nu, 1), dtype=t.int32, device=self.device)
        self._ck(self.L.havoc_mi355x_unit_pred_select(self.h, bit_depth, _ptr(planes[0]), _ptr(planes[1]), _ptr(planes[2]), dst_stride, _ptr(planes[3]), dst_stride_c,
                                                      _ptr(d_first), _ptr(d_best), _ptr(d_rate), _ptr(j), n, _ptr(unit_rate), _ptr(unit_cand)))
        return (self.down(planes[2], np.uint8).view(dt).copy(), self.down(planes[3], np.uint8).view(dt).copy(), self.down(unit_rate, np.int64)[:nu],
                self.down(unit_cand, np.int32)[:nu])

    def intra_rate_jobs_d(self, mpm, order, count, slot, rdoq_jobs, n, flags, jobs):
        """INTRA_RATE_JOB_DT records of the candidates intra_expand laid out (havoc_mi355x_intra_rate_jobs): job c = candidate slot c; jobs: uint8 tensor.  No sync."""
        self._ck(self.L.havoc_mi355x_intra_rate_jobs(self.h, _ptr(mpm), _ptr(order), _ptr(count), _ptr(slot), _ptr(rdoq_jobs), n, flags, _ptr(jobs)))

    def intra_decide_rated_d(self, mpm, order, count, slot, cbf, ssd, stats, rates, tu_jobs, n, log2, rl_q16, out, final):
        """havoc_mi355x_intra_decide_rated: the champion of every partition by rates[s] + rl_q16 * ssd[s]; stats may be None.  No sync."""
        self._ck(self.L.havoc_mi355x_intra_decide_rated(self.h, _ptr(mpm), _ptr(order), _ptr(count), _ptr(slot), _ptr(cbf), _ptr(ssd), _ptr(stats), _ptr(rates),
                                                        _ptr(tu_jobs), n, log2, rl_q16, _ptr(out), _ptr(final)))

    def ssd_linear_d(self, a, b, n, out):
        self._ck(self.L.havoc_mi355x_ssd_linear(self.h, _ptr(a), _ptr(b), n, _ptr(out)))

    # ---------------------------------------------------------------- numpy-level batch interface (tests/suite.py)
    def _jobs(self, j, ncols):
        j = np.ascontiguousarray(np.asarray(j, np.int32)[:, :ncols])
        return self.up(j)

    def sad(self, a, sa, b, sb, jobs):
        out = self.zeros(len(jobs), np.int32)
        self.sad_d(self.up(a), sa, self.up(b), sb, self._jobs(jobs, 4), out)
        return self.down(out, np.int32)

    def sad4(self, a, sa, b, sb, jobs):
        out = self.zeros(4 * len(jobs), np.int32)
        self.sad4_d(self.up(a), sa, self.up(b), sb, self._jobs(jobs, 8), out)
        return self.down(out, np.int32).reshape(-1, 4)

    def sad4_runs(self, a, sa, b, sb, jobs, runs=None, max_run=0):
        """havoc_sad_multiref calls by runs (one search's consecutive calls share a staged window); runs None = cut by sad4_make_runs"""
        jobs = np.ascontiguousarray(jobs, np.int32)
        if runs is None:
            runs = self.sad4_make_runs(jobs, max_run, sb, np.asarray(b).itemsize)
        runs = np.ascontiguousarray(runs, np.int32)
        if runs.ndim == 2 and runs.shape[1] == 2:
            runs = self.as_runs(runs)
        out = self.zeros(4 * len(jobs), np.int32)
        if len(jobs) and len(runs):
            self.sad4_runs_d(self.up(a), sa, self.up(b), sb, self._jobs(jobs, 8), self.up(runs), out)
        return self.down(out, np.int32).reshape(-1, 4)

    def sad_surface(self, a, sa, b, sb, rng, jobs):
        """jobs rows: src_off, ref_off, w, h; returns [njobs, 2R+1, 2R+1] (dy, dx)"""
        jobs = np.asarray(jobs, np.int32)
        side = 2 * rng + 1
        j = np.zeros((len(jobs), 8), np.int32)
        j[:, :4] = jobs[:, :4]
        j[:, 4] = np.arange(len(jobs)) * side * side
        out = self.zeros(len(jobs) * side * side, np.int32)
        if len(jobs):
            mw = (int(j[:, 2].max()) + 3) & ~3
            self.sad_surface_d(self.up(a), sa, self.up(b), sb, rng, mw, int(j[:, 3].max()), self.up(j), out)
        return self.down(out, np.int32).reshape(-1, side, side)

    def ssd(self, a, sa, b, sb, jobs):
        out = self.zeros(len(jobs), np.uint32)
        self.ssd_d(self.up(a), sa, self.up(b), sb, self._jobs(jobs, 4), out)
        return self.down(out, np.uint32)

    def satd_multi(self, a, sa, b, sb, jobs):
        """jobs rows: a_off, w, h, count, b_off[16]; returns [njobs, 16] (entries k >= count are 0); one launch per
        lane-group class like satd"""
        jobs = np.asarray(jobs, np.int32)
        out = np.zeros((len(jobs), 16), np.int32)
        ad, bdv = self.up(a), self.up(b)
        rows = ((jobs[:, 1] + 7) // 8) * jobs[:, 2]
        for lo, hi, mw, mh in ((0, 8, 8, 8), (8, 16, 16, 8), (16, 32, 16, 16), (32, 128, 32, 32), (128, 1 << 30, 64, 64)):
            idx = np.flatnonzero((rows > lo) & (rows <= hi))
            if len(idx):
                o = self.zeros(16 * len(idx), np.int32)
                self.satd_multi_d(ad, sa, bdv, sb, self._jobs(jobs[idx], 20), o, mw, mh)
                out[idx] = self.down(o, np.int32).reshape(-1, 16)
        return out

    def satd(self, a, sa, b, sb, jobs):
        """one launch per lane-group class so that every group size (8 / 16 / 32 / 64 lanes per job) is exercised"""
        jobs = np.asarray(jobs, np.int32)
        out = np.zeros(len(jobs), np.int32)
        ad, bdv = self.up(a), self.up(b)
        rows = ((jobs[:, 2] + 7) // 8) * jobs[:, 3]
        for lo, hi, mw, mh in ((0, 8, 8, 8), (8, 16, 16, 8), (16, 32, 16, 16), (32, 1 << 30, 64, 64)):
            idx = np.flatnonzero((rows > lo) & (rows <= hi))
            if len(idx):
                o = self.zeros(len(idx), np.int32)
                self.satd_d(ad, sa, bdv, sb, self._jobs(jobs[idx], 4), o, mw, mh)
                out[idx] = self.down(o, np.int32)
        return out

    def ssd_linear(self, a, b, n):
        out = self.zeros(1, np.int32)
        self.ssd_linear_d(self.up(a), self.up(b), n, out)
        return int(self.down(out, np.int32)[0])

    def pred_uni(self, taps, bd, dst_len, sd, ref, sr, jobs):
        jobs = np.asarray(jobs, np.int32)
        dst = self.zeros(dst_len, ref.dtype)
        r = self.up(ref)
        for idx, mw, mh in self.size_classes(jobs[:, 2], jobs[:, 3]):
            self.pred_uni_d(taps, bd, dst, sd, r, sr, self._jobs(jobs[idx], 8), mw, mh)
        return self.down(dst, ref.dtype)

    def pred_bi(self, taps, bd, dst_len, sd, ref, sr, jobs):
        jobs = np.asarray(jobs, np.int32)
        dst = self.zeros(dst_len, ref.dtype)
        r = self.up(ref)
        for idx, mw, mh in self.size_classes(jobs[:, 3], jobs[:, 4]):
            self.pred_bi_d(taps, bd, dst, sd, r, sr, self._jobs(jobs[idx], 12), mw, mh)
        return self.down(dst, ref.dtype)

    def subtract_bi(self, bd, dst_len, sd, pred, sp, src, ss, jobs):
        dst = self.zeros(dst_len, src.dtype)
        self.subtract_bi_d(bd, dst, sd, self.up(pred), sp, self.up(src), ss, self._jobs(jobs, 8))
        return self.down(dst, src.dtype)

    def intra(self, bd, dst_len, sd, nb, jobs):
        jobs = np.asarray(jobs, np.int32)
        dst = self.zeros(dst_len, nb.dtype)
        nbd = self.up(nb)
        for log2 in (2, 3, 4, 5):   # one launch per block size (the reference's table index)
            sel = jobs[jobs[:, 2] == log2]
            if len(sel):
                self.intra_d(bd, log2, dst, sd, nbd, self._jobs(sel, 8))
        return self.down(dst, nb.dtype)

    def intra_satd35(self, bd, src, ss, nb, jobs):
        """jobs: int32 [n, 8] = (src_off, nb_off, nbf_off, filt_lo, filt_hi, edge, log2, 0); returns int32 [n, 35]"""
        jobs = np.asarray(jobs, np.int32)
        out = np.zeros((len(jobs), 35), np.int32)
        s, nbd = self.up(src), self.up(nb)
        for log2 in (2, 3, 4, 5):
            idx = np.flatnonzero(jobs[:, 6] == log2)
            if len(idx):
                cost = self.zeros(35 * len(idx), np.int32)
                self.intra_satd35_d(bd, log2, s, ss, nbd, self._jobs(jobs[idx], 8), cost)
                out[idx] = self.down(cost, np.int32).reshape(-1, 35)
        return out

    def residual(self, res_len, sres, res_off, src, ss, pred, sp, jobs):
        res = self.zeros(res_len, np.int16)
        self.residual_d(res, sres, self.up(np.asarray(res_off, np.int32)), self.up(src), ss, self.up(pred), sp, self._jobs(jobs, 4))
        return self.down(res, np.int16)

    @staticmethod
    def _tu_groups(jobs):
        jobs = np.asarray(jobs, np.int32)
        for log2, tr in ((2, 1), (2, 0), (3, 0), (4, 0), (5, 0)):
            sel = jobs[(jobs[:, 4] == log2) & (jobs[:, 5] == tr)]
            if len(sel):
                yield log2, tr, sel

    def transform(self, bd, ncoef, res, stride, jobs):
        co = self.zeros(ncoef, np.int16)
        r = self.up(res)
        for log2, tr, sel in self._tu_groups(jobs):
            self.transform_d(bd, tr, log2, co, r, stride, self._jobs(sel, 4))
        return self.down(co, np.int16)

    def inverse_transform(self, bd, nres, coeffs, jobs):
        res = self.zeros(nres, np.int16)
        c = self.up(coeffs)
        for log2, tr, sel in self._tu_groups(jobs):
            self.inverse_transform_d(bd, tr, log2, res, c, self._jobs(sel, 4))
        return self.down(res, np.int16)

    def inverse_transform_add(self, bd, dst_len, sd, pred, sp, coeffs, jobs):
        dst = self.zeros(dst_len, pred.dtype)
        c = self.up(coeffs)
        p = self.up(pred)
        for log2, tr, sel in self._tu_groups(jobs):
            self.inverse_transform_add_d(bd, tr, log2, dst, sd, p, sp, c, self._jobs(sel, 4))
        return self.down(dst, pred.dtype)

    def quantize(self, nout, src, jobs):
        dst = self.zeros(nout, np.int16)
        cbf = self.zeros(len(jobs), np.int32)
        self.quantize_d(dst, self.up(src), self._jobs(jobs, 8), cbf)
        return self.down(dst, np.int16), self.down(cbf, np.int32)

    def quantize_inverse(self, nout, src, jobs):
        dst = self.zeros(nout, np.int16)
        self.quantize_inverse_d(dst, self.up(src), self._jobs(jobs, 8))
        return self.down(dst, np.int16)

    def quantize_reconstruct(self, dst_len, sr, pred, sp, res, jobs):
        jobs = np.asarray(jobs, np.int32)
        rec = self.zeros(dst_len, np.uint8)
        p = self.up(pred)
        r = self.up(res)
        for log2 in (2, 3, 4, 5):
            sel = jobs[jobs[:, 4] == log2]
            if len(sel):
                self.quantize_reconstruct_d(log2, rec, sr, p, sp, r, self._jobs(sel, 4))
        return self.down(rec, np.uint8)
