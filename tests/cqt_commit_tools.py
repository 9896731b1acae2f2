"""havoc_mi355x_cqt_commit restated in numpy: of the searched units, the final coding units of every decided CTU into one picture of three planes and one record per
MinCb cell (include/havoc_mi355x.h).  Test infrastructure.  `commit_picture` is the call restated, with the branch every unit takes counted by name in `tags`;
`make_case` makes the inputs of one call -- the quadtree's own records from tests/cqt_tools.py's restatement of the decision over random closed units, random pieces and
prediction planes that differ everywhere, destinations and cells pre-filled with a sentinel -- and `Client` compiles tests/cqt_commit_client.cpp (search/
cqt_decision.hpp's commitCqt).  No reference shim: every sample was pinned where it was made, this step only selects.
"""
import collections
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import cqt_tools as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# include/havoc_mi355x.h: havoc_mi355x_cqt_cell, havoc_mi355x_rqt_unit, havoc_mi355x_rqt_choice, havoc_mi355x_rqt_tree_choice, havoc_mi355x_rqt_chroma_at
CELL_DT = np.dtype([("unit", "<i4"), ("cand", "<i4"), ("mv", "<i2", (2, 2)), ("log2_size", "u1"), ("outcome", "u1"), ("pred", "u1"), ("tr_depth", "u1"), ("cbf", "<u4")])
UNIT_DT = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("log2_size", "<i4"), ("ctx_index", "<i4")])
TU_DT = np.dtype([("cbf", "<i4"), ("ssd", "<u4"), ("nonzero", "<i4"), ("sum_abs", "<i4")])
RQT_DT = np.dtype([("depth", "<i4"), ("tried_zero", "<i4"), ("zero", TU_DT), ("one", TU_DT, 4), ("cost_zero", "<i8"), ("cost_one", "<i8")])
TREE_DT = np.dtype([("mask_zero", "<u4"), ("mask_one", "<u4"), ("chroma_ssd_zero", "<i4"), ("chroma_ssd_one", "<i4")])
CHROMA_AT_DT = np.dtype([("cb_zero", "<i4"), ("cr_zero", "<i4"), ("cb_one", "<i4"), ("cr_one", "<i4")])
assert (CELL_DT.itemsize, UNIT_DT.itemsize, RQT_DT.itemsize, TREE_DT.itemsize, CHROMA_AT_DT.itemsize) == (24, 16, 104, 16, 16)
SENTINEL = 0xA5         # every byte of the destinations and the cells before the call

# the branch a unit takes: the five ways it is committed, the ways it is not
COMMITTED = ("coded_depth0", "coded_depth1", "coded_64", "coded_8_shared_chroma", "no_residual", "skipped")
REQUIRED_TAGS = COMMITTED + ("not_final", "ctu_undecided")


def node_of(x0, y0, log2, ctb_log2):
    """a unit's node index in its CTU's table: depth d = ctb_log2 - log2, (4^d - 1) / 3 + the z-order index of its place"""
    d = ctb_log2 - log2
    px, py = (x0 & ((1 << ctb_log2) - 1)) >> log2, (y0 & ((1 << ctb_log2) - 1)) >> log2
    z = sum((px >> b & 1) << 2 * b | (py >> b & 1) << (2 * b + 1) for b in range(3))
    return Q.first(d) + z


def make_case(seed, width, height, ctb_log2, min_cb_log2, bit_depth, undecided=(), none_decided=False, p_refused=0.08, with_mv=True, refuse_final=0):
    """the inputs of one call, as a dict.  The closed units are cqt_tools.make_case's (a candidate at every node inside the picture: trees of every shape), some of them
    refused afterwards; record p of `choice` IS unit p.  undecided: CTUs whose `decided` is cleared after the decision, node records left as they were.  refuse_final:
    that many final units get a refused record AFTER the decision -- which no quadtree decides over; the call's fourth condition then leaves a hole."""
    rng = np.random.default_rng(seed + 1000)
    q = Q.make_case(seed, width, height, ctb_log2, min_cb_log2, Q.WPP, p_candidate=1.0)
    levels, cells, cx, cy, count = Q.geometry(q)
    n = len(q["choice"])
    # every record's unit: the node that names it; a record no node names gets the geometry of CTU 0's first MinCb node, which names another
    units = np.zeros(n, UNIT_DT)
    units["log2_size"] = min_cb_log2
    for c in range(cx * cy):
        for d in range(levels):
            L = ctb_log2 - d
            for z in range(4 ** d):
                p = q["node_cu"][c, Q.first(d) + z]
                if 0 <= p < n:
                    px = sum((z >> 2 * b & 1) << b for b in range(d))
                    py = sum((z >> (2 * b + 1) & 1) << b for b in range(d))
                    units[p] = ((c % cx << ctb_log2) + (px << L), (c // cx << ctb_log2) + (py << L), L, c)
    # some units above MinCb refused: their nodes then have no candidate
    for p in np.flatnonzero((units["log2_size"] > min_cb_log2) & (rng.random(n) < p_refused)):
        q["choice"][p] = Q.choice_records([Q.REFUSED], [0], [0])[0]
    res = Q.decide_picture(q)
    ctus = res["ctus"].copy()
    for c in undecided:
        assert ctus[c]["decided"] == 1
        ctus[c]["decided"] = 0
    if none_decided:
        ctus["decided"] = 0
    final = [int(q["node_cu"][c, k]) for c in range(cx * cy) for k in range(count) if res["nodes"][c, k]["flags"] & Q.FINAL and res["nodes"][c, k]["choice"] == Q.CU]
    for p in final[1:1 + 2 * refuse_final:2]:
        q["choice"][p] = Q.choice_records([Q.REFUSED], [0], [0])[0]
    S, dt = (1, np.uint8) if bit_depth == 8 else (2, np.uint16)
    top = 1 << bit_depth
    # the transform-tree records and where each unit's candidate pieces are, laid out as DecisionPicture's unit plan lays them out
    uL = units["log2_size"].astype(np.int64)
    rqt, tree, chroma_at = np.zeros(n, RQT_DT), np.zeros(n, TREE_DT), np.zeros(n, CHROMA_AT_DT)
    zero_at, one_at = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    lists, clists = {s: 0 for s in (2, 3, 4, 5)}, {s: 0 for s in (2, 3, 4)}
    for p in range(n):
        L, a = int(uL[p]), chroma_at[p]
        if L < 6:
            zero_at[p], lists[L] = lists[L], lists[L] + 1
            a["cb_zero"], a["cr_zero"] = clists[L - 1], clists[L - 1] + 1
            clists[L - 1] += 2
        else:
            a["cb_zero"], a["cr_zero"] = -1, -1
        one_at[p], lists[L - 1] = lists[L - 1], lists[L - 1] + 4
        if L > 3:
            a["cb_one"], a["cr_one"] = clists[L - 2], clists[L - 2] + 4
            clists[L - 2] += 8
        else:
            a["cb_one"], a["cr_one"] = a["cb_zero"], a["cr_zero"]
    rqt["depth"], rqt["tried_zero"] = rng.integers(0, 2, n), np.where(uL < 6, rng.integers(0, 2, n), 0)
    tree["mask_zero"], tree["mask_one"] = rng.integers(1, 1 << 12, n), rng.integers(1 << 12, 1 << 24, n)
    luma = [rng.integers(0, top, max(lists[s], 1) << 2 * s).astype(dt) for s in (2, 3, 4, 5)]
    chroma = [rng.integers(0, top, max(clists[s], 1) << 2 * s).astype(dt) for s in (2, 3, 4)]
    # the unit prediction planes: plane ctb_log2 - L holds the units of size 2^L at their picture positions
    ux, uy, plane = units["x0"].astype(np.int64), units["y0"].astype(np.int64), ctb_log2 - uL
    hw, hh = width // 2, height // 2
    pred_y, pred_c = rng.integers(0, top, levels * width * height).astype(dt), rng.integers(0, top, 2 * levels * hw * hh).astype(dt)
    pred_off = np.stack([plane * width * height + uy * width + ux, 2 * plane * hw * hh + (uy // 2) * hw + ux // 2, (2 * plane + 1) * hw * hh + (uy // 2) * hw + ux // 2],
                        1).astype(np.int32)
    best = rng.integers(0, 3, n).astype(np.int32)
    unit_cand = (3 * np.arange(n) + best).astype(np.int32)
    cand_mv = rng.integers(1, 1 << 12, (3 * n, 2, 2)).astype(np.int16) * rng.choice([-1, 1], (3 * n, 2, 2)).astype(np.int16)
    # the destinations: padded planes whose rows start at no multiple of 8 bytes
    pad, cpad = 4, 2
    stride, cstride = width + 2 * pad + 3, hw + 2 * cpad + 1
    cplane = (hh + 2 * cpad) * cstride + 5
    return dict(bit_depth=bit_depth, S=S, dt=dt, width=width, height=height, ctb_log2=ctb_log2, min_cb_log2=min_cb_log2, units=units, node_cu=q["node_cu"], ctus=ctus,
                nodes=res["nodes"], cu=q["choice"], rqt=rqt, tree=tree, zero_at=zero_at, one_at=one_at, chroma_at=chroma_at, luma=luma, chroma=chroma, pred_y=pred_y,
                pred_c=pred_c, pred_stride=width, pred_stride_c=hw, pred_off=pred_off, best=best, unit_cand=unit_cand, cand_mv=cand_mv if with_mv else None,
                rec_y_size=(height + 2 * pad) * stride, rec_origin=pad * stride + pad, rec_stride=stride, rec_c_size=2 * cplane, cb_origin=cpad * cstride + cpad,
                cr_origin=cplane + cpad * cstride + cpad, c_stride=cstride)


def sentinels(case):
    """-> the destinations and the cell map as they are before the call: every byte SENTINEL"""
    s = np.dtype(case["dt"]).type(SENTINEL * (0x0101 if case["S"] == 2 else 1))
    hc, wc = case["height"] >> case["min_cb_log2"], case["width"] >> case["min_cb_log2"]
    return dict(rec_y=np.full(case["rec_y_size"], s, case["dt"]), rec_c=np.full(case["rec_c_size"], s, case["dt"]),
                cells=np.full((hc, wc, CELL_DT.itemsize), SENTINEL, np.uint8).view(CELL_DT).reshape(hc, wc))


def _block(buf, origin, stride, x, y, size):
    """the size x size block at (x, y) of a plane inside the flat buffer, as a writable view"""
    return np.lib.stride_tricks.as_strided(buf[origin + y * stride + x:], (size, size), (stride * buf.itemsize, buf.itemsize))


def _pieces(dst, pieces, log2, quads, at):
    """dst <- one piece of size log2, or four of size log2 - 1 in z-order; candidate j of size s lies at j << 2 s"""
    if not quads:
        dst[:] = pieces[log2 - 2][at << 2 * log2:(at + 1) << 2 * log2].reshape(1 << log2, 1 << log2)
        return
    l = log2 - 1
    for k in range(4):
        piece = pieces[l - 2][(at + k) << 2 * l:(at + k + 1) << 2 * l].reshape(1 << l, 1 << l)
        dst[(k >> 1) << l:((k >> 1) + 1) << l, (k & 1) << l:((k & 1) + 1) << l] = piece


def commit_picture(case, tags=None):
    """havoc_mi355x_cqt_commit restated -> dict(rec_y, rec_c: the flat destination buffers, cells CELL_DT [rows, cells per row]), from sentinels(case)"""
    tags = collections.Counter() if tags is None else tags
    out = sentinels(case)
    out["cells"].view(np.uint8)[:] = 0xff                       # the fill
    ctb, mcb, W, H = case["ctb_log2"], case["min_cb_log2"], case["width"], case["height"]
    cx, count = -(-W >> ctb), Q.n_nodes(ctb - mcb + 1)
    for p, u in enumerate(case["units"]):
        x0, y0, L = int(u["x0"]), int(u["y0"]), int(u["log2_size"])
        size = 1 << L
        if L < mcb or L > ctb or x0 < 0 or y0 < 0 or (x0 | y0) & (size - 1) or x0 + size > W or y0 + size > H:
            tags["no_such_node"] += 1
            continue
        c, k = (y0 >> ctb) * cx + (x0 >> ctb), node_of(x0, y0, L, ctb)
        if case["ctus"][c]["decided"] != 1:
            tags["ctu_undecided"] += 1
            continue
        if case["node_cu"][c, k] != p:
            tags["not_its_node"] += 1
            continue
        node = case["nodes"][c, k]
        if not node["flags"] & Q.FINAL or node["choice"] != Q.CU:
            tags["not_final"] += 1
            continue
        outcome = int(case["cu"][p]["outcome"])
        if outcome not in (Q.CODED, Q.NO_RESIDUAL, Q.SKIPPED):
            tags["refused"] += 1
            continue
        y = _block(out["rec_y"], case["rec_origin"], case["rec_stride"], x0, y0, size)
        cb = _block(out["rec_c"], case["cb_origin"], case["c_stride"], x0 // 2, y0 // 2, size // 2)
        cr = _block(out["rec_c"], case["cr_origin"], case["c_stride"], x0 // 2, y0 // 2, size // 2)
        tr_depth = cbf = 0
        if outcome == Q.CODED:
            r, t, a = case["rqt"][p], case["tree"][p], case["chroma_at"][p]
            tr_depth = 0 if L < 6 and r["depth"] == 0 and r["tried_zero"] else 1
            cbf = int(t["mask_one"] if tr_depth else t["mask_zero"])
            _pieces(y, case["luma"], L, tr_depth == 1, int(case["one_at"][p] if tr_depth else case["zero_at"][p]))
            quads = tr_depth == 1 and L > 3
            _pieces(cb, case["chroma"], L - 1, quads, int(a["cb_one"] if quads else a["cb_zero"]))
            _pieces(cr, case["chroma"], L - 1, quads, int(a["cr_one"] if quads else a["cr_zero"]))
            tags["coded_64" if L == 6 else "coded_depth1" if tr_depth else "coded_depth0"] += 1
            if L == 3:
                tags["coded_8_shared_chroma"] += 1
        else:
            off = case["pred_off"][p]
            y[:] = _block(case["pred_y"], int(off[0]), case["pred_stride"], 0, 0, size)
            cb[:] = _block(case["pred_c"], int(off[1]), case["pred_stride_c"], 0, 0, size // 2)
            cr[:] = _block(case["pred_c"], int(off[2]), case["pred_stride_c"], 0, 0, size // 2)
            tags["no_residual" if outcome == Q.NO_RESIDUAL else "skipped"] += 1
        cell = np.zeros(1, CELL_DT)[0]
        pred, cand = int(case["best"][p]), int(case["unit_cand"][p])
        cell["unit"], cell["cand"], cell["log2_size"], cell["outcome"], cell["pred"], cell["tr_depth"], cell["cbf"] = p, cand, L, outcome, pred, tr_depth, cbf
        if case["cand_mv"] is not None and cand >= 0:
            for l in (0, 1):
                if pred in (l, 2):
                    cell["mv"][l] = case["cand_mv"][cand, l]
        out["cells"][y0 >> mcb:(y0 + size) >> mcb, x0 >> mcb:(x0 + size) >> mcb] = cell
    return out


def same(got, want):
    """every destination byte and every cell; -> the first key that differs, or None"""
    for k in ("rec_y", "rec_c", "cells"):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.tobytes() != b.tobytes():
            return k
    return None


# the synthetic cases: name -> make_case's arguments.  136x72 at CTB 64 / MinCb 8 is 3 x 2 CTUs, the last column and row a cell wide and high: forced splits and deleted
# nodes; 40x24 at CTB 16 / MinCb 8 has two levels only.
CASES = {
    "136x72_8bit": dict(seed=1, width=136, height=72, ctb_log2=6, min_cb_log2=3, bit_depth=8),
    "136x72_10bit": dict(seed=3, width=136, height=72, ctb_log2=6, min_cb_log2=3, bit_depth=10),
    "40x24_8bit": dict(seed=7, width=40, height=24, ctb_log2=4, min_cb_log2=3, bit_depth=8),
    "40x24_10bit": dict(seed=8, width=40, height=24, ctb_log2=4, min_cb_log2=3, bit_depth=10, with_mv=False),
    "136x72_ctu_undecided": dict(seed=5, width=136, height=72, ctb_log2=6, min_cb_log2=3, bit_depth=8, undecided=(1,)),
    "40x24_final_refused": dict(seed=9, width=40, height=24, ctb_log2=4, min_cb_log2=3, bit_depth=8, refuse_final=2),
    "136x72_none_decided": dict(seed=6, width=136, height=72, ctb_log2=6, min_cb_log2=3, bit_depth=10, none_decided=True),
}


class Client:
    """tests/cqt_commit_client.cpp: search/cqt_decision.hpp's commitCqt over every CTU, compiled at test time"""

    def __init__(self):
        self._tmp = tempfile.TemporaryDirectory()
        so = os.path.join(self._tmp.name, "libcqt_commit_client.so")
        subprocess.check_call(["g++", "-O1", "-std=c++14", "-fPIC", "-shared", "-Wall", "-o", so, os.path.join(ROOT, "tests", "cqt_commit_client.cpp")])
        self.L = C.CDLL(so)
        self.L.cqt_commit_picture.restype = C.c_int
        self.L.cqt_commit_picture.argtypes = [C.c_void_p, C.c_void_p]

    def commit_picture(self, case):
        """-> (what commit_picture gives, the units committed)"""
        out = sentinels(case)
        out["cells"].view(np.uint8)[:] = 0xff
        n = len(case["units"])
        tree = np.zeros((n, 10), np.int32)
        tree[:, 0], tree[:, 1] = case["rqt"]["depth"], case["rqt"]["tried_zero"]
        tree[:, 2], tree[:, 3] = case["tree"]["mask_zero"].view(np.int32), case["tree"]["mask_one"].view(np.int32)
        tree[:, 4], tree[:, 5] = case["zero_at"], case["one_at"]
        tree[:, 6:] = np.stack([case["chroma_at"][k] for k in ("cb_zero", "cr_zero", "cb_one", "cr_one")], 1)
        g = np.array([case[k] for k in ("bit_depth", "width", "height", "ctb_log2", "min_cb_log2")] + [n] +
                     [case[k] for k in ("pred_stride", "pred_stride_c", "rec_origin", "rec_stride", "cb_origin", "cr_origin", "c_stride")], np.int64)
        keep = [np.ascontiguousarray(a) for a in (case["units"], case["cu"]["outcome"], tree, *case["luma"], *case["chroma"], case["pred_y"], case["pred_c"],
                                                   case["pred_off"], case["best"], case["unit_cand"])]
        keep.append(None if case["cand_mv"] is None else np.ascontiguousarray(case["cand_mv"]))
        keep += [out["rec_y"], out["rec_c"], out["cells"], np.ascontiguousarray(case["node_cu"], np.int32), np.ascontiguousarray(case["ctus"]["decided"]),
                 np.ascontiguousarray(case["nodes"]["choice"]), np.ascontiguousarray(case["nodes"]["flags"])]
        p = np.array([0 if a is None else a.ctypes.data for a in keep], np.uint64)
        done = self.L.cqt_commit_picture(g.ctypes.data, p.ctypes.data)
        return out, done
