"""havoc_mi355x_cqt_block_cells restated in numpy: the committed record per MinCb cell (havoc_mi355x_cqt_cell) as the map of 4x4 cells havoc_mi355x_derive_bs reads
(include/havoc_mi355x.h).  Test infrastructure.  `block_cells` is the call restated, with the branch every cell takes counted by name in `tags`; `unit_lists` makes,
from the SAME committed cells but unit by unit, the coding / prediction / transform unit rows the reference's own boundary-strength derivation takes
(reflibs.Reference.derive_bs): an independent second opinion on what the flags mean; `make_cells` writes a random quadtree per CTU directly as committed cells;
`Client` compiles tests/cqt_finish_client.cpp (search/cqt_decision.hpp's cqtBlockCells).
"""
import collections
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from cqt_commit_tools import CELL_DT as CQT_CELL_DT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# include/havoc_mi355x.h: havoc_mi355x_cell and HAVOC_CELL_*; HAVOC_CU_OUTCOME_*
CELL_DT = np.dtype([("mv", "<i2", (2, 2)), ("dpb_index", "i1", (2,)), ("flags", "u1"), ("qp_y", "i1"), ("tu_log2", "u1"), ("reserved", "u1", (3,))])
assert CELL_DT.itemsize == 16 and CQT_CELL_DT.itemsize == 24
CELL_INTRA, CELL_CODED, CELL_NO_FILTER, CELL_PU_LEFT, CELL_PU_TOP = 1, 2, 4, 8, 16
CODED, NO_RESIDUAL, SKIPPED = 0, 1, 2
SENTINEL = 0xA5         # every byte of the destination before the call

# the branch a 4x4 cell takes.  only_child_k: the cell is coded as child k of a depth-1 tree whose luma mask has that bit alone; min8_right / min8_bottom: the one coded
# 4x4 block of an 8x8 unit at depth 1 lies in its right column / bottom row -- the strength it raises belongs to the NEIGHBOURING unit's edge; clamp: tu_log2 clamped to 5
REQUIRED_TAGS = ("undecided", "pred0", "pred1", "pred2", "coded_depth0", "only_child_0", "only_child_1", "only_child_2", "only_child_3", "min8_right", "min8_bottom",
                 "coded_64", "uncoded_64", "coded_luma0_chroma")


def block_cells(cqt_cells, W, H, min_cb_log2, qp, dpb0, dpb1, tags=None):
    """havoc_mi355x_cqt_block_cells restated -> CELL_DT [H / 4, W / 4]"""
    tags = collections.Counter() if tags is None else tags
    out = np.zeros((H // 4, W // 4), CELL_DT)
    for y in range(0, H, 4):
        for x in range(0, W, 4):
            q, c = cqt_cells[y >> min_cb_log2, x >> min_cb_log2], out[y >> 2, x >> 2]
            c["qp_y"] = qp
            if q["unit"] < 0:       # the CTU was not decided: nobody's samples, the filter leaves them alone; nothing else of q is read
                c["dpb_index"], c["flags"], c["tu_log2"] = -1, CELL_NO_FILTER, 2
                tags["undecided"] += 1
                continue
            L, outcome, pred, depth, cbf = int(q["log2_size"]), int(q["outcome"]), int(q["pred"]), int(q["tr_depth"]), int(q["cbf"])
            size = 1 << L
            ox, oy = x & (size - 1), y & (size - 1)
            k = (oy >= size // 2) * 2 + (ox >= size // 2) if depth else 0
            coded = outcome == CODED and bool(cbf >> k & 1)
            c["mv"] = q["mv"]
            c["dpb_index"] = (dpb0 if pred != 1 else -1, dpb1 if pred != 0 else -1)
            c["flags"] = (CELL_CODED if coded else 0) | (CELL_PU_LEFT if ox == 0 else 0) | (CELL_PU_TOP if oy == 0 else 0)
            c["tu_log2"] = min(L - depth, 5)
            tags["pred%d" % pred] += 1
            if coded and not depth:
                tags["coded_depth0"] += 1
            if coded and depth and cbf & 15 == 1 << k:
                tags["only_child_%d" % k] += 1
                if L == 3:
                    tags["min8_right"] += k & 1
                    tags["min8_bottom"] += k >> 1
            if L == 6:
                tags["coded_64" if coded else "uncoded_64" if outcome != CODED else "in_coded_64_uncoded_child"] += 1
            if outcome == CODED and not cbf & 15 and cbf >> 4:
                tags["coded_luma0_chroma"] += 1
    return out


def units_of(cqt_cells, min_cb_log2):
    """the decided coding units, each once: [(x0, y0, the committed cell at its origin)] -- the cell whose own position is a multiple of its unit's size"""
    out = []
    for (j, i), q in np.ndenumerate(cqt_cells):
        x, y = i << min_cb_log2, j << min_cb_log2
        if q["unit"] >= 0 and not (x | y) & ((1 << int(q["log2_size"])) - 1):
            out.append((x, y, q))
    return out


def unit_lists(cqt_cells, W, H, min_cb_log2, qp, dpb0, dpb1):
    """-> cus int32 [n, 6] (x0, y0, log2CbSize, intra, QpY, bypass), pus int32 [n, 10] (x0, y0, nPbW, nPbH, mvL0 x, y, mvL1 x, y, dpb index L0, L1 or -1), tus int32
    [m, 5] (x0, y0, log2TrafoSize, cbf_luma, intra): what reflibs.Reference.derive_bs takes.  Made per UNIT: one cu, one 2Nx2N pu, one tu per standing transform block
    -- a unit at transform depth 1 (and a 64x64 unit always: its split is inferred) has four, each with its own bit of the luma mask."""
    cus, pus, tus = [], [], []
    for x0, y0, q in units_of(cqt_cells, min_cb_log2):
        L, pred, depth = int(q["log2_size"]), int(q["pred"]), int(q["tr_depth"])
        size = 1 << L
        assert x0 + size <= W and y0 + size <= H
        cus.append((x0, y0, L, 0, qp, 0))
        mv = q["mv"]
        pus.append((x0, y0, size, size, mv[0, 0], mv[0, 1], mv[1, 0], mv[1, 1], dpb0 if pred != 1 else -1, dpb1 if pred != 0 else -1))
        mask = int(q["cbf"]) & 15 if q["outcome"] == CODED else 0
        if depth or L == 6:
            for k in range(4):
                tus.append((x0 + (k & 1) * size // 2, y0 + (k >> 1) * size // 2, L - 1, mask >> k & 1 if depth else 0, 0))
        else:
            tus.append((x0, y0, L, mask & 1, 0))
    return np.array(cus, np.int32).reshape(-1, 6), np.array(pus, np.int32).reshape(-1, 10), np.array(tus, np.int32).reshape(-1, 5)


def unit_edge_strengths(cqt_cells, W, H, min_cb_log2, bs):
    """the 2-bit strengths (havoc_mi355x_deblock's d_block_bs layout) of every 4-sample segment of the decided units' left and top edges inside the picture"""
    n64 = (W + 63) // 64 * 8 + 1
    out = []
    for x0, y0, q in units_of(cqt_cells, min_cb_log2):
        size = 1 << int(q["log2_size"])
        if x0 > 0:
            out += [bs[(y // 8) * n64 + x0 // 8] >> ((y // 4) % 2) * 2 & 3 for y in range(y0, y0 + size, 4)]
        if y0 > 0:
            out += [bs[(y0 // 8) * n64 + x // 8] >> (4 + ((x // 4) % 2) * 2) & 3 for x in range(x0, x0 + size, 4)]
    return np.array(out, np.int64)


# vectors around a per-picture base: a small pool, so that neighbouring units are often equal, often 1-3 quarter samples apart, often 4 or more apart
POOL = np.array([(0, 0), (0, 0), (1, 0), (0, -2), (3, 3), (5, 0), (0, 7), (-9, 2)], np.int16)


def make_cells(seed, W, H, ctb_log2, min_cb_log2, undecided=(), none_decided=False):
    """a random quadtree per CTU written directly as committed cells -> CQT_CELL_DT [H >> min_cb_log2, W >> min_cb_log2].  pred over all three modes, outcomes over
    all three, both transform depths with random luma masks (most of them one child alone), a coded unit's mask never empty (luma 0 then has a chroma bit);
    undecided: CTUs (raster index) left all-ones bytes"""
    rng = np.random.default_rng(seed + 2000)
    cells = np.zeros((H >> min_cb_log2, W >> min_cb_log2), CQT_CELL_DT)
    base = rng.integers(-40, 41, 2).astype(np.int16)
    cx = -(-W >> ctb_log2)
    count = [0]

    def unit(x, y, L):
        size = 1 << L
        if x >= W or y >= H:
            return
        if L > min_cb_log2 and (x + size > W or y + size > H or rng.random() < (0.45 if L == ctb_log2 else 0.6)):
            for k in range(4):
                unit(x + (k & 1) * size // 2, y + (k >> 1) * size // 2, L - 1)
            return
        q = np.zeros(1, CQT_CELL_DT)[0]
        q["unit"], q["cand"], q["log2_size"] = count[0], int(rng.integers(0, 1 << 20)), L
        count[0] += 1
        q["pred"], q["outcome"] = rng.choice(3, p=(0.5, 0.25, 0.25)), rng.choice(3, p=(0.5, 0.25, 0.25))
        for l in (0, 1):
            if q["pred"] in (l, 2):
                q["mv"][l] = base + POOL[int(rng.integers(0, len(POOL)))]
        if q["outcome"] == CODED:
            q["tr_depth"] = 1 if L == 6 else int(rng.integers(0, 2))
            if q["tr_depth"]:
                luma = 1 << int(rng.integers(0, 4)) if rng.random() < 0.6 else int(rng.integers(0, 16))
                chroma = int(rng.integers(0, 256)) if L > 3 else int(rng.integers(0, 2)) | int(rng.integers(0, 2)) << 4
            else:
                luma, chroma = int(rng.random() < 0.6), int(rng.integers(0, 2)) | int(rng.integers(0, 2)) << 4
            q["cbf"] = luma | chroma << 4 or 1 << 4
        cells[y >> min_cb_log2:(y + size) >> min_cb_log2, x >> min_cb_log2:(x + size) >> min_cb_log2] = q

    for y in range(0, H, 1 << ctb_log2):
        for x in range(0, W, 1 << ctb_log2):
            unit(x, y, ctb_log2)
    n = 1 << (ctb_log2 - min_cb_log2)
    for c in range(cx * -(-H >> ctb_log2)) if none_decided else undecided:
        cells[(c // cx) * n:(c // cx + 1) * n, (c % cx) * n:(c % cx + 1) * n].view(np.uint8)[...] = 0xff
    return cells


# the synthetic cases: name -> (make_cells' arguments, qp, dpb0, dpb1).  136x72 at CTB 64 / MinCb 8: a last column and row one MinCb cell wide; 40x24 at CTB 16: two
# levels only; 64x64 at MinCb 16: a committed cell covers sixteen 4x4 cells.  The seeds were chosen so that the cases together reach every required tag
CASES = {
    "136x72": (dict(seed=4, W=136, H=72, ctb_log2=6, min_cb_log2=3), 32, 0, 1),
    "40x24_ctb16": (dict(seed=3, W=40, H=24, ctb_log2=4, min_cb_log2=3), 27, 3, 3),
    "64x64_mincb16": (dict(seed=16, W=64, H=64, ctb_log2=6, min_cb_log2=4), 51, 127, 0),
    "136x72_ctu_undecided": (dict(seed=14, W=136, H=72, ctb_log2=6, min_cb_log2=3, undecided=(1,)), 0, 1, 2),
    "136x72_none_decided": (dict(seed=5, W=136, H=72, ctb_log2=6, min_cb_log2=3, none_decided=True), 32, 0, 1),
}
FULLY_DECIDED = ("136x72", "40x24_ctb16", "64x64_mincb16")


def make_case(name):
    """-> dict(cqt, W, H, min_cb_log2, qp, dpb0, dpb1)"""
    a, qp, dpb0, dpb1 = CASES[name]
    return dict(cqt=make_cells(**a), W=a["W"], H=a["H"], min_cb_log2=a["min_cb_log2"], qp=qp, dpb0=dpb0, dpb1=dpb1)


def restate(case, tags=None):
    return block_cells(case["cqt"], case["W"], case["H"], case["min_cb_log2"], case["qp"], case["dpb0"], case["dpb1"], tags)


class Client:
    """tests/cqt_finish_client.cpp: search/cqt_decision.hpp's cqtBlockCells, compiled at test time"""

    def __init__(self):
        self._tmp = tempfile.TemporaryDirectory()
        so = os.path.join(self._tmp.name, "libcqt_finish_client.so")
        subprocess.check_call(["g++", "-O1", "-std=c++14", "-fPIC", "-shared", "-Wall", "-o", so, os.path.join(ROOT, "tests", "cqt_finish_client.cpp")])
        self.L = C.CDLL(so)
        self.L.cqt_block_cells_picture.restype = None
        self.L.cqt_block_cells_picture.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]

    def block_cells(self, case, stride=None):
        """-> uint8 [H / 4, stride * 16]: the destination rows, the sentinel where nothing was written"""
        stride = case["W"] // 4 if stride is None else stride
        out = np.full((case["H"] // 4, stride * CELL_DT.itemsize), SENTINEL, np.uint8)
        g = np.array([case["W"], case["H"], case["min_cb_log2"], case["qp"], case["dpb0"], case["dpb1"], stride], np.int32)
        cqt = np.ascontiguousarray(case["cqt"])
        self.L.cqt_block_cells_picture(g.ctypes.data, cqt.ctypes.data, out.ctypes.data)
        return out


def rows_of(cells, stride):
    """the restatement laid out as a destination of `stride` cells per row whose other bytes hold the sentinel -> uint8 [H / 4, stride * 16]"""
    out = np.full((cells.shape[0], stride * CELL_DT.itemsize), SENTINEL, np.uint8)
    out[:, :cells.shape[1] * CELL_DT.itemsize] = np.ascontiguousarray(cells).view(np.uint8).reshape(cells.shape[0], -1)
    return out
