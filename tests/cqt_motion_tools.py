"""havoc_mi355x_cqt_motion_store and havoc_mi355x_temporal_candidates restated in numpy (include/havoc_mi355x.h).  Test infrastructure.

`motion_store` is the first call restated -- the committed record per MinCb cell (havoc_mi355x_cqt_cell) as the collocated motion store, one havoc_mi355x_col_cell
per 16x16 luma samples -- with the branch every entry takes counted by name in `tags`; `unit_rows` makes, from the SAME committed cells but unit by unit, what the
reference's own store takes (`Shim`: tests/cqt_motion_shim.cpp, a real StateCollocatedMotion filled through its own fillRectangle once per unit), and `shim_view` puts
the restated store into the shim's terms: an independent second opinion on which unit owns which entry.  `temporal_candidates` is the second call restated -- python
integers, no line shared with search/amvp.hpp -- with the branch every (unit, list) takes counted by name.  `Client` compiles tests/cqt_motion_client.cpp
(cqtMotionStore and deriveTemporalCandidate, the host forms).  Random committed cells come from cqt_finish_tools.make_cells.
"""
import collections
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import sao_decision_tools as T
from cqt_commit_tools import CELL_DT as CQT_CELL_DT
from cqt_finish_tools import make_cells, units_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# include/havoc_mi355x.h: havoc_mi355x_col_cell, havoc_mi355x_temporal_params, havoc_mi355x_temporal_cand; search/search_abi.h: havoc_picture_pu
COL_CELL_DT = np.dtype([("mv", "<i2", (2, 2)), ("ref_poc", "<i4", (2,)), ("pred_flag", "u1", (2,)), ("long_term", "u1", (2,)), ("reserved", "<u4")])
PARAMS_DT = np.dtype([("pic_width", "<i4"), ("pic_height", "<i4"), ("ctb_log2", "<i4"), ("col_poc", "<i4"), ("cur_poc", "<i4"), ("target_poc", "<i4", (2,)),
                      ("all_backwards", "<i4"), ("collocated_from_l0", "<i4"), ("reserved", "<i4", (3,))])
CAND_DT = np.dtype([("mv", "<i2", (2,)), ("available", "<i2"), ("source", "<i2")])
PU_DT = np.dtype([("x0", "i4"), ("y0", "i4"), ("w", "i4"), ("h", "i4"), ("cu_log2_size", "i4"), ("cqt_depth", "i4"), ("part_2Nx2N", "i4"), ("reserved", "i4")])
assert COL_CELL_DT.itemsize == 24 and PARAMS_DT.itemsize == 48 and CAND_DT.itemsize == 8 and PU_DT.itemsize == 32 and CQT_CELL_DT.itemsize == 24
NONE, BOTTOM_RIGHT, CENTRE = 0, 1, 2
SENTINEL = 0xA5         # every byte of a destination before the call


# ================================================================================================================== the store
STORE_TAGS = ("undecided", "pred0", "pred1", "pred2", "unit8_without_entry", "unit8_with_entry", "unit64_sixteen_entries", "right_partial_column", "bottom_partial_row")


def store_shape(W, H):
    return (H + 15) // 16, (W + 15) // 16


def motion_store(cqt_cells, W, H, min_cb_log2, ref_poc0, ref_poc1, tags=None):
    """havoc_mi355x_cqt_motion_store restated -> COL_CELL_DT [(H + 15) // 16, (W + 15) // 16].  Tags per ENTRY: undecided, pred0 / pred1 / pred2,
    right_partial_column / bottom_partial_row (the entry's 16x16 area reaches beyond the picture); per decided UNIT: unit8_without_entry / unit8_with_entry (an 8x8
    unit that contains no / one sample of the 16-grid), unit64_sixteen_entries"""
    tags = collections.Counter() if tags is None else tags
    sh, sw = store_shape(W, H)
    out = np.zeros((sh, sw), COL_CELL_DT)
    owner = {}
    for Y in range(sh):
        for X in range(sw):
            q, c = cqt_cells[16 * Y >> min_cb_log2, 16 * X >> min_cb_log2], out[Y, X]
            tags["right_partial_column"] += 16 * X + 16 > W
            tags["bottom_partial_row"] += 16 * Y + 16 > H
            if q["unit"] < 0:       # the CTU was not decided: "not available", every byte zero; nothing else of q is read
                tags["undecided"] += 1
                continue
            pred = int(q["pred"])
            for l, ref in ((0, ref_poc0), (1, ref_poc1)):
                if pred != 1 - l:
                    c["pred_flag"][l], c["mv"][l], c["ref_poc"][l] = 1, q["mv"][l], ref
            tags["pred%d" % pred] += 1
            owner[int(q["unit"])] = owner.get(int(q["unit"]), 0) + 1
    for x0, y0, q in units_of(cqt_cells, min_cb_log2):
        L, got = int(q["log2_size"]), owner.get(int(q["unit"]), 0)
        if L == 3:
            assert got == (0 if (x0 | y0) & 15 else 1)
            tags["unit8_with_entry" if got else "unit8_without_entry"] += 1
        if L == 6 and got == 16:
            tags["unit64_sixteen_entries"] += 1
    return out


def unit_rows(cqt_cells, min_cb_log2, rng=None):
    """the decided coding units, each once, as the shim takes them: int32 [n, 10] = x0, y0, size, predFlag0, predFlag1, mv0 x, y, mv1 x, y, 0 -- in a random order when
    rng is given (every entry has one writer: the order cannot matter)"""
    rows = []
    for x0, y0, q in units_of(cqt_cells, min_cb_log2):
        pred, mv = int(q["pred"]), q["mv"]
        rows.append((x0, y0, 1 << int(q["log2_size"]), pred != 1, pred != 0, mv[0, 0], mv[0, 1], mv[1, 0], mv[1, 1], 0))
    rows = np.array(rows, np.int32).reshape(-1, 10)
    return rows if rng is None else rows[rng.permutation(len(rows))]


def shim_view(store, ref_poc0, ref_poc1, dpb0, dpb1):
    """the restated store in the shim's terms -> int32 [rows, cols, 8] = predFlag0, predFlag1, mv0 x, y, mv1 x, y, dpb index 0, 1 (-1: none): ref_poc l translated to
    the dpb index of the picture behind list l.  A list without motion must have ref_poc 0 and mv 0"""
    out = np.zeros(store.shape + (8,), np.int32)
    out[..., 0:2] = store["pred_flag"]
    out[..., 2:6] = store["mv"].reshape(store.shape + (4,))
    for l, (ref, dpb) in enumerate(((ref_poc0, dpb0), (ref_poc1, dpb1))):
        used = store["pred_flag"][..., l] != 0
        assert (store["ref_poc"][..., l][used] == ref).all() and not store["ref_poc"][..., l][~used].any() and not store["mv"][..., l, :][~used].any()
        out[..., 6 + l] = np.where(used, dpb, -1)
    assert not store["long_term"].any() and not store["reserved"].any()
    return out


# the synthetic stores: name -> (make_cells' arguments, ref_poc0, ref_poc1).  136x72 at CTB 64 / MinCb 8: 3x2 CTUs, a partial right column (entry X = 8 at x = 128) and
# a partial bottom row (Y = 4 at y = 64); 64x64 at MinCb 8 and at MinCb 16 (a committed cell IS an entry's area).  The seeds were chosen so that the cases together
# reach every tag of STORE_TAGS (tests/test_cqt_motion.py asserts it)
STORE_CASES = {
    "136x72": (dict(seed=4, W=136, H=72, ctb_log2=6, min_cb_log2=3), 0, 16),
    "136x72_ctu_undecided": (dict(seed=14, W=136, H=72, ctb_log2=6, min_cb_log2=3, undecided=(1,)), -3, 7232),
    "64x64_mincb8": (dict(seed=1, W=64, H=64, ctb_log2=6, min_cb_log2=3), 7, 9),
    "64x64_mincb16": (dict(seed=16, W=64, H=64, ctb_log2=6, min_cb_log2=4), 32776, -32759),      # (the two ends of DiffPicOrderCnt's range)
    "64x64_one_unit": (dict(seed=3, W=64, H=64, ctb_log2=6, min_cb_log2=3), 9, 7),      # (one bi-predicted 64x64 unit: sixteen entries)
}
POC = 8                 # the committed picture's own, in every case


def make_store_case(name):
    """-> dict(cqt, W, H, min_cb_log2, poc, ref_poc0, ref_poc1)"""
    a, r0, r1 = STORE_CASES[name]
    return dict(cqt=make_cells(**a), W=a["W"], H=a["H"], min_cb_log2=a["min_cb_log2"], poc=POC, ref_poc0=r0, ref_poc1=r1)


def restate_store(case, tags=None):
    return motion_store(case["cqt"], case["W"], case["H"], case["min_cb_log2"], case["ref_poc0"], case["ref_poc1"], tags)


def golden_path():
    return os.path.join(ROOT, "tests", "golden", "cqt_motion_golden.npz")


GOLDEN_DPB = (3, 5)     # the dpb indices the golden entries were made with (lists 0 and 1)


# ================================================================================================================== the candidates
PU_SIZES = ((8, 8), (16, 16), (32, 32), (64, 64), (16, 8), (8, 16), (32, 16))
CAND_TAGS = ("bottom_right_used", "bottom_right_next_ctu_row", "bottom_right_beyond_right_edge", "bottom_right_beyond_bottom_edge", "bottom_right_empty_centre_used",
             "none", "only_l0", "only_l1", "both_all_backwards", "both_from_l0", "both_from_l1", "same_distance", "scaled", "scaled_negative_td", "td_clipped",
             "tb_clipped", "factor_clipped", "vector_clipped", "long_term", "col_poc_equals_ref_poc", "pu_outside_picture") + tuple("pu_%dx%d" % s for s in PU_SIZES)


def _clip3(lo, hi, v):
    return lo if v < lo else hi if v > hi else v


def _scale(mv, t_d, t_b, tags):
    """8.5.3.2.7 in python integers"""
    td, tb = _clip3(-128, 127, t_d), _clip3(-128, 127, t_b)
    tags["td_clipped"] += td != t_d
    tags["tb_clipped"] += tb != t_b
    tags["scaled_negative_td"] += td < 0
    tx = (16384 + abs(td) // 2) // abs(td) * (1 if td > 0 else -1)      # C's division truncates towards zero
    f = (tb * tx + 32) >> 6
    tags["factor_clipped"] += not -4096 <= f <= 4095
    f = _clip3(-4096, 4095, f)
    out = []
    for c in mv:
        p = f * int(c)
        v = ((abs(p) + 127) >> 8) * (-1 if p < 0 else 1)
        tags["vector_clipped"] += not -32768 <= v <= 32767
        out.append(_clip3(-32768, 32767, v))
    return out


def _cell_vector(c, X, P, tags):
    """one cell's contribution for list X -> (x, y) or None"""
    f0, f1 = bool(c["pred_flag"][0]), bool(c["pred_flag"][1])
    if not f0 and not f1:
        return None
    if f0 and f1:
        if P["all_backwards"]:
            l = X
            tags["both_all_backwards"] += 1
        else:
            l = 1 if P["collocated_from_l0"] else 0
            tags["both_from_l0" if P["collocated_from_l0"] else "both_from_l1"] += 1
    else:
        l = 0 if f0 else 1
        tags["only_l%d" % l] += 1
    if c["long_term"][l]:
        tags["long_term"] += 1
        return None
    t_d, t_b = int(P["col_poc"]) - int(c["ref_poc"][l]), int(P["cur_poc"]) - int(P["target_poc"][X])
    if t_d == 0:            # this project's own rule: the reference would divide by zero
        tags["col_poc_equals_ref_poc"] += 1
        return None
    if t_d == t_b:
        tags["same_distance"] += 1
        return [int(v) for v in c["mv"][l]]
    tags["scaled"] += 1
    return _scale(c["mv"][l], t_d, t_b, tags)


def temporal_candidates(params, store, pus, tags=None):
    """havoc_mi355x_temporal_candidates restated; params: one PARAMS_DT record, store: COL_CELL_DT [rows, cols], pus: PU_DT [n] -> CAND_DT [n, 2]"""
    tags = collections.Counter() if tags is None else tags
    P = np.asarray(params).reshape(1)[0]
    W, H, ctb = int(P["pic_width"]), int(P["pic_height"]), int(P["ctb_log2"])
    out = np.zeros((len(pus), 2), CAND_DT)
    for p, q in enumerate(pus):
        x0, y0, w, h = int(q["x0"]), int(q["y0"]), int(q["w"]), int(q["h"])
        if x0 < 0 or y0 < 0 or w <= 0 or h <= 0 or x0 + w > W or y0 + h > H:
            tags["pu_outside_picture"] += 1
            continue
        tags["pu_%dx%d" % (w, h)] += 1
        xb, yb = x0 + w, y0 + h
        for X in (0, 1):
            v, source = None, NONE
            if xb >= W:
                tags["bottom_right_beyond_right_edge"] += 1
            if yb >= H:
                tags["bottom_right_beyond_bottom_edge"] += 1
            elif (y0 >> ctb) != (yb >> ctb):
                tags["bottom_right_next_ctu_row"] += 1
            consulted = (y0 >> ctb) == (yb >> ctb) and yb < H and xb < W
            if consulted:
                assert (yb >> 4) < store.shape[0] and (xb >> 4) < store.shape[1]
                v = _cell_vector(store[yb >> 4, xb >> 4], X, P, tags)
                source = BOTTOM_RIGHT
            if v is None:
                v = _cell_vector(store[(y0 + h // 2) >> 4, (x0 + w // 2) >> 4], X, P, tags)
                source = CENTRE
                tags["bottom_right_empty_centre_used"] += consulted and v is not None
            if v is None:
                tags["none"] += 1
                continue
            tags["bottom_right_used"] += source == BOTTOM_RIGHT
            out[p, X]["mv"], out[p, X]["available"], out[p, X]["source"] = v, 1, source
    return out


def make_params(W, H, ctb_log2, col_poc, cur_poc, target_poc, all_backwards, collocated_from_l0):
    p = np.zeros(1, PARAMS_DT)
    p["pic_width"], p["pic_height"], p["ctb_log2"], p["col_poc"], p["cur_poc"] = W, H, ctb_log2, col_poc, cur_poc
    p["target_poc"], p["all_backwards"], p["collocated_from_l0"] = target_poc, all_backwards, collocated_from_l0
    return p


def make_col_store(seed, W, H, col_poc):
    """a synthetic store: cells without motion, with one list, with both; vectors small and -- a tenth -- near the ends of the 16-bit range; reference pictures one
    picture away on either side of the collocated one, a few and very many pictures before it, and the collocated picture itself; a few long-term"""
    rng = np.random.default_rng(seed + 3000)
    sh, sw = store_shape(W, H)
    s = np.zeros((sh, sw), COL_CELL_DT)
    kinds = rng.choice(4, (sh, sw), p=(0.2, 0.25, 0.25, 0.3))      # none, L0, L1, both
    refs = np.array([col_poc - 1, col_poc + 1, col_poc - 4, col_poc - 8, col_poc - 200, col_poc + 300, col_poc])
    for l in (0, 1):
        used = (kinds == l + 1) | (kinds == 3)
        mv = rng.integers(-64, 65, (sh, sw, 2))
        big = rng.random((sh, sw)) < 0.1
        mv[big] = rng.choice([-32768, -32760, -30000, 30000, 32767], (int(big.sum()), 2))
        s["pred_flag"][..., l] = used
        s["mv"][..., l, :] = np.where(used[..., None], mv, 0)
        s["ref_poc"][..., l] = np.where(used, rng.choice(refs, (sh, sw), p=(0.2, 0.15, 0.25, 0.15, 0.1, 0.05, 0.1)), 0)
        s["long_term"][..., l] = used & (rng.random((sh, sw)) < 0.08)
    return s


def make_pus(seed, W, H, count):
    """random units of every size of PU_SIZES, each aligned to 8 and inside the picture; then a few that are not inside it"""
    rng = np.random.default_rng(seed + 4000)
    pus = np.zeros(count + 6, PU_DT)
    for i in range(count):
        w, h = PU_SIZES[int(rng.integers(0, len(PU_SIZES)))]
        pus[i]["w"], pus[i]["h"] = w, h
        pus[i]["x0"], pus[i]["y0"] = 8 * int(rng.integers(0, (W - w) // 8 + 1)), 8 * int(rng.integers(0, (H - h) // 8 + 1))
    for i, (x0, y0, w, h) in enumerate(((-8, 0, 8, 8), (0, -8, 16, 16), (W - 8, 0, 16, 8), (0, H - 8, 8, 16), (8, 8, 0, 8), (W, H, 8, 8))):
        pus[count + i]["x0"], pus[count + i]["y0"], pus[count + i]["w"], pus[count + i]["h"] = x0, y0, w, h
    pus["cu_log2_size"], pus["reserved"] = 0x5a5a5a5a, -1      # (not read)
    return pus


# the synthetic calls: name -> (seed, W, H, ctb_log2, col_poc, cur_poc, target_poc, all_backwards, collocated_from_l0, units).  Between them: every choice of list, both
# picture edges, CTU rows of 64, 32 and 16, distances equal, scaled, negative, beyond +-128 on either side (cur_poc 300), and a factor beyond 4095 (tb 127 over td 1)
CAND_CASES = {
    "136x72_from_l0": (1, 136, 72, 6, 8, 4, (0, 8), 0, 1, 160),
    "136x72_all_backwards_ctb32": (2, 136, 72, 5, 8, 16, (12, 8), 1, 0, 160),
    "136x72_from_l1_far_ctb16": (3, 136, 72, 4, 8, 300, (100, 299), 0, 0, 160),
    "72x136_factor": (4, 72, 136, 6, 8, 135, (8, 134), 0, 1, 160),
}


def make_cand_case(name):
    """-> dict(params, store, pus)"""
    seed, W, H, ctb, col_poc, cur_poc, target, back, from_l0, count = CAND_CASES[name]
    return dict(params=make_params(W, H, ctb, col_poc, cur_poc, target, back, from_l0), store=make_col_store(seed, W, H, col_poc), pus=make_pus(seed, W, H, count))


# ================================================================================================================== the host forms and the reference
class Client:
    """tests/cqt_motion_client.cpp: search/cqt_decision.hpp's cqtMotionStore and search/amvp.hpp's deriveTemporalCandidate, compiled at test time"""

    def __init__(self):
        self._tmp = tempfile.TemporaryDirectory()
        so = os.path.join(self._tmp.name, "libcqt_motion_client.so")
        subprocess.check_call(["g++", "-O1", "-std=c++14", "-fPIC", "-shared", "-Wall", "-o", so, os.path.join(ROOT, "tests", "cqt_motion_client.cpp")])
        self.L = C.CDLL(so)
        self.L.cqt_motion_store_picture.restype = None
        self.L.cqt_motion_store_picture.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self.L.temporal_candidates_picture.restype = None
        self.L.temporal_candidates_picture.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p]

    def motion_store(self, case, extra=48):
        """-> uint8: the store's bytes and `extra` more behind them, the sentinel where nothing was written"""
        sh, sw = store_shape(case["W"], case["H"])
        out = np.full(sh * sw * COL_CELL_DT.itemsize + extra, SENTINEL, np.uint8)
        g = np.array([case["W"], case["H"], case["min_cb_log2"], case["ref_poc0"], case["ref_poc1"]], np.int32)
        cqt = np.ascontiguousarray(case["cqt"])
        self.L.cqt_motion_store_picture(g.ctypes.data, cqt.ctypes.data, out.ctypes.data)
        return out

    def temporal_candidates(self, params, store, pus):
        """-> CAND_DT [n, 2]"""
        params, store, pus = np.ascontiguousarray(params, PARAMS_DT), np.ascontiguousarray(store, COL_CELL_DT), np.ascontiguousarray(pus, PU_DT)
        out = np.zeros((len(pus), 2), CAND_DT)
        self.L.temporal_candidates_picture(params.ctypes.data, store.ctypes.data, store.shape[1], pus.ctypes.data, len(pus), out.ctypes.data)
        return out


def flat(store, extra=48):
    """the restated store laid out as a destination with `extra` sentinel bytes behind it"""
    return np.concatenate([np.ascontiguousarray(store).view(np.uint8).reshape(-1), np.full(extra, SENTINEL, np.uint8)])


def reference_dir():
    return T.reference_dir()


class Shim:
    """tests/cqt_motion_shim.cpp over the reference's turing/StateCollocatedMotion.h, built with oracle/Makefile's TURFLAGS"""

    def __init__(self):
        ref = T.reference_dir()
        assert ref, "reference sources not present"
        self._tmp = tempfile.TemporaryDirectory()
        so = os.path.join(self._tmp.name, "libcqt_motion.so")
        flags = T._make_var("TURFLAGS").split()
        subprocess.check_call(["g++"] + flags + ["-shared", "-o", so, os.path.join(ROOT, "tests", "cqt_motion_shim.cpp")])
        self.L = C.CDLL(so)
        self.L.cqt_motion_entries.restype = C.c_int
        self.L.cqt_motion_entries.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]

    def entries(self, case, dpb0, dpb1, rng=None):
        """the reference's store after one fillRectangle per committed unit -> int32 [rows, cols, 8] (shim_view's layout)"""
        sh, sw = store_shape(case["W"], case["H"])
        rows = np.ascontiguousarray(unit_rows(case["cqt"], case["min_cb_log2"], rng))
        out = np.full((sh, sw, 8), -99, np.int32)
        g = np.array([case["W"], case["H"]], np.int32)
        stride = self.L.cqt_motion_entries(g.ctypes.data, rows.ctypes.data, len(rows), dpb0, dpb1, out.ctypes.data)
        assert stride == sw
        return out
