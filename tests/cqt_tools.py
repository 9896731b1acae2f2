"""The coding quadtree of a CTU -- Search<coding_quadtree>::go (turing/Search.hpp:808-886) over Syntax<coding_quadtree>::go (turing/SyntaxCtu.hpp:95-139) and the
writer of split_cu_flag (turing/Binarization.h:102-122) -- restated on the CPU in plain Python, in the reference's order, with the branch it takes counted by name
in `tags` (a collections.Counter) and every priced flag appended to `trace`.  Test infrastructure.

Rates are integers (Cost = FixedPoint<int64_t, 16>): the flag's one context-coded bin costs measureEncodeDecision (sao_merge_tools.bin_cost: the tables of
turingcodec_amd/csrc/cabac_tables.h, which the device uses too) and moves its context.  `Shim` compiles tests/cqt_shim.cpp -- the reference's own
Syntax<coding_quadtree>::go and writer over a stand-in handle with a real snake -- into a temporary directory; `DecisionClient` compiles tests/cqt_client.cpp
(search/cqt_decision.hpp's decideCqt).  `make_case` makes the inputs of one call of havoc_mi355x_cqt_decide as a dict; `decide_picture` is the call restated:
the CTUs in coding order, the contexts from CTU to CTU under the WPP rule (turing/StatePictures.h:1042-1075, 1108-1115), the picture's CtDepth map.
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

# include/havoc_mi355x.h: HAVOC_CQT_*, HAVOC_CQT_NODE_*, the records, HAVOC_CU_OUTCOME_*
WPP, ECU = 1, 2
NOT_VISITED, CU, SPLIT, DELETED = 0, 1, 2, 3
FINAL, FLAG_CODED, MUST_SPLIT, ECU_STOP, NO_CANDIDATE, NO_SPLIT_CANDIDATE = 1, 2, 4, 8, 16, 32
REFUSED, CODED, NO_RESIDUAL, SKIPPED = -1, 0, 1, 2
CTU_DT = np.dtype([("decided", "<i4"), ("n_cus", "<i4"), ("rate", "<i8"), ("flag_rate", "<i8"), ("lambda_distortion", "<i8"), ("cost", "<i8")])
NODE_DT = np.dtype([("choice", "u1"), ("flags", "u1"), ("ctx_inc", "u1"), ("pad", "u1", 5), ("cost_full", "<i8"), ("cost_split", "<i8")])
CHOICE_DT = np.dtype([("outcome", "<i4"), ("have_residual", "<i4"), ("rate", "<i8"), ("lambda_distortion", "<i8"), ("cost", "<i8"), ("cost_coded", "<i8"),
                      ("cost_no_residual", "<i8")])
SYNTAX_BYTES = 16


def first(d):
    """index of node (d, 0)"""
    return (4 ** d - 1) // 3


def n_nodes(levels):
    return first(levels)


def depth_of(k):
    """the depth of node index k"""
    return next(d for d in range(5) if k < first(d + 1))


def geometry(case):
    """-> levels, cells per CTU side, CTUs per row, CTU rows, nodes per CTU"""
    levels = case["ctb_log2"] - case["min_cb_log2"] + 1
    ctb = 1 << case["ctb_log2"]
    return levels, 1 << (levels - 1), -(-case["width"] // ctb), -(-case["height"] // ctb), n_nodes(levels)


class Walk:
    """one CTU: cand[k] = None or (rate, lambdaDistortion, skipped) per node; ctx: three states; cell[y + 1][x + 1]: CtDepth, row 0 / column 0 the neighbours'"""

    def __init__(self, cand, ctx, left, up, levels, cells_x, cells_y, ecu, tags, trace, origin, min_cb_log2):
        self.cand, self.ctx, self.levels, self.cells_x, self.cells_y, self.ecu = cand, list(ctx), levels, cells_x, cells_y, ecu
        self.tags = collections.Counter() if tags is None else tags
        self.trace, self.origin, self.min_cb_log2 = trace, origin, min_cb_log2
        cells = 1 << (levels - 1)
        self.cell = np.zeros((9, 9), np.int64)
        self.cell[1:cells + 1, 0], self.cell[0, 1:cells + 1] = left[:cells], up[:cells]
        self.nodes = np.zeros(n_nodes(levels), NODE_DT)
        self.refused = False
        # some node below this one has a candidate: where none has, there is nothing to compare the node's unit with (testSplit == false, Search.hpp:795-801)
        self.below = [False] * n_nodes(levels)
        for d in range(levels - 2, -1, -1):
            for z in range(4 ** d):
                kids = range(first(d + 1) + 4 * z, first(d + 1) + 4 * z + 4)
                self.below[first(d) + z] = any(cand[k] is not None or self.below[k] for k in kids)

    def flag(self, d, x, y, inc, b):
        """Write<Element<split_cu_flag, ae>>: EncodeDecision<split_cu_flag>(binVal, ctxInc), measured"""
        before = list(self.ctx)
        self.ctx[inc], bits = bin_cost(self.ctx[inc], b)
        if self.trace is not None:
            self.trace.append(dict(x0=self.origin[0] + (x << self.min_cb_log2), y0=self.origin[1] + (y << self.min_cb_log2),
                                   log2=self.min_cb_log2 + self.levels - 1 - d, depth=d, left=int(self.cell[y + 1, x]), up=int(self.cell[y, x + 1]), inc=inc, bin=b,
                                   before=before, bits=bits, after=list(self.ctx)))
        return bits

    def children(self, d, z, x, y):
        """SyntaxCtu.hpp:112-136"""
        h = 1 << (self.levels - 2 - d)
        total = [0, 0, 0]
        for k in range(4):
            if self.refused:
                break
            cx, cy = x + (k & 1) * h, y + (k >> 1) * h
            if cx >= self.cells_x or cy >= self.cells_y:
                self.nodes[first(d + 1) + 4 * z + k]["choice"] = DELETED
                self.tags["deleted", "corner" if cx >= self.cells_x and cy >= self.cells_y else "right" if cx >= self.cells_x else "below", d + 1] += 1
                continue
            c = self.go(d + 1, 4 * z + k, cx, cy)
            total = [a + b for a, b in zip(total, c)]
        return total

    def go(self, d, z, x, y):
        """Search<coding_quadtree>::go -> [rate, the coded flags' part of it, lambdaDistortion] of the winner"""
        s = 1 << (self.levels - 1 - d)
        n, c, tags = self.nodes[first(d) + z], self.cand[first(d) + z], self.tags
        over_x, over_y = x + s > self.cells_x, y + s > self.cells_y
        must_split, min_cb = over_x or over_y, d == self.levels - 1          # Search.hpp:810-812
        coded = not must_split and not min_cb                                 # SyntaxCtu.hpp:97-99
        n["cost_full"] = n["cost_split"] = -1
        inc = 0
        if coded:
            inc = int(self.cell[y + 1, x] > d) + int(self.cell[y, x + 1] > d)   # Binarization.h:114-116
            n["ctx_inc"], n["flags"] = inc, FLAG_CODED
            tags["ctx_inc", inc] += 1
        elif min_cb:
            tags["flag_not_coded_min_cb",] += 1
        if must_split:                                                      # :819-823
            tags["must_split", "corner" if over_x and over_y else "right" if over_x else "bottom", d] += 1
            n["flags"] |= MUST_SPLIT
            n["choice"] = SPLIT
            r = self.children(d, z, x, y)
            n["cost_split"] = r[0] + r[2]
            return r
        before = list(self.ctx)
        full = [0, 0, 0]
        if c is not None:                                                   # :839-851
            if coded:
                full[1] = self.flag(d, x, y, inc, 0)
            full[0], full[2] = full[1] + c[0], c[1]
            self.cell[y + 1:y + 1 + s, x + 1:x + 1 + s] = d
            n["cost_full"] = full[0] + full[2]
            n["choice"] = CU
        else:
            n["flags"] |= NO_CANDIDATE
        ecu_stop = c is not None and not min_cb and self.ecu and c[2]       # :854
        if ecu_stop:
            n["flags"] |= ECU_STOP
            tags["ecu_stop", d] += 1
        bare = c is not None and not min_cb and not self.below[first(d) + z]
        if bare:
            n["flags"] |= NO_SPLIT_CANDIDATE
            tags["no_split_candidate", d] += 1
        if c is not None and (min_cb or ecu_stop or bare):
            return full
        if min_cb:
            self.refused = True
            return full
        after = list(self.ctx)                                              # :857-871
        self.ctx = before
        flag = self.flag(d, x, y, inc, 1) if coded else 0
        split = self.children(d, z, x, y)
        if self.refused:
            return split
        split[0] += flag
        split[1] += flag
        n["cost_split"] = split[0] + split[2]
        if c is None or n["cost_split"] < n["cost_full"]:                  # :875
            tags["no_candidate_split" if c is None else "split_wins", d] += 1
            n["choice"] = SPLIT
            return split
        tags["equal_keeps_cu" if n["cost_split"] == n["cost_full"] else "cu_wins", d] += 1
        self.ctx = after
        self.cell[y + 1:y + 1 + s, x + 1:x + 1 + s] = d
        return full


def decide_ctu(cand, ctx, left, up, levels, cells_x, cells_y, ecu, tags=None, trace=None, origin=(0, 0), min_cb_log2=3):
    """-> (CTU_DT record, NODE_DT [nodes], depth int8 [cells, cells], the three contexts after); a refused CTU: all zero, the contexts as they came"""
    w = Walk(cand, ctx, left, up, levels, cells_x, cells_y, ecu, tags, trace, origin, min_cb_log2)
    cells = 1 << (levels - 1)
    r = w.go(0, 0, 0, 0)
    rec = np.zeros(1, CTU_DT)[0]
    if w.refused:
        return rec, np.zeros(n_nodes(levels), NODE_DT), np.zeros((cells, cells), np.int8), list(ctx)
    nodes = w.nodes
    nodes[0]["flags"] |= FINAL
    for d in range(1, levels):
        for z in range(4 ** d):
            p, n = nodes[first(d - 1) + (z >> 2)], nodes[first(d) + z]
            if p["flags"] & FINAL and p["choice"] == SPLIT and n["choice"] != NOT_VISITED:
                n["flags"] |= FINAL
    rec["decided"], rec["n_cus"] = 1, int(((nodes["flags"] & FINAL != 0) & (nodes["choice"] == CU)).sum())
    rec["rate"], rec["flag_rate"], rec["lambda_distortion"], rec["cost"] = r[0], r[1], r[2], r[0] + r[2]
    return rec, nodes, w.cell[1:cells + 1, 1:cells + 1].astype(np.int8), list(w.ctx)


def candidates(case, i):
    """node k of CTU i -> None or (rate, lambdaDistortion, skipped), as havoc_mi355x_cqt_decide reads them"""
    out = []
    for idx in case["node_cu"][i]:
        rec = case["choice"][idx] if 0 <= idx < len(case["choice"]) else None
        if rec is None or rec["outcome"] == REFUSED:
            out.append(None)
        else:
            out.append((int(rec["rate"]), int(rec["lambda_distortion"]), int(rec["outcome"]) == SKIPPED))
    return out


def decide_picture(case, tags=None, trace=None):
    """havoc_mi355x_cqt_decide restated -> dict(ctus CTU_DT [n], nodes NODE_DT [n, nodes], depth int8 [rows, cells per row], cu_syntax uint8 [n, 16]);
    trace (a list): per priced flag a dict, with `ctu` added"""
    tags = collections.Counter() if tags is None else tags
    levels, cells, cx, cy, count = geometry(case)
    wc, hc = case["width"] >> case["min_cb_log2"], case["height"] >> case["min_cb_log2"]
    wpp, ecu = bool(case["flags"] & WPP), bool(case["flags"] & ECU)
    initial = [int(v) for v in case["cu_syntax"][:3]]
    ctx, saved = list(initial), None
    depth = np.zeros((cy * cells, cx * cells), np.int8)
    ctus, nodes = np.zeros(cx * cy, CTU_DT), np.zeros((cx * cy, count), NODE_DT)
    syntax = np.tile(np.asarray(case["cu_syntax"], np.uint8), (cx * cy, 1))
    for r in range(cy):
        for x in range(cx):
            i = r * cx + x
            if x == 0 and r > 0:
                if wpp and cx >= 2:
                    ctx = list(saved)                   # after CTU (1, r - 1)
                    tags["wpp_start_ctu1",] += 1
                elif wpp:
                    ctx = list(initial)
                    tags["wpp_start_slice",] += 1
                else:
                    tags["raster_carry",] += 1
            left = depth[r * cells:(r + 1) * cells, x * cells - 1] if x > 0 else np.full(cells, -1)
            up = depth[r * cells - 1, x * cells:(x + 1) * cells] if r > 0 else np.full(cells, -1)
            t0 = len(trace) if trace is not None else 0
            rec, nd, dp, after = decide_ctu(candidates(case, i), ctx, left, up, levels, min(cells, wc - x * cells), min(cells, hc - r * cells), ecu, tags, trace,
                                            (x << case["ctb_log2"], r << case["ctb_log2"]), case["min_cb_log2"])
            if trace is not None:
                if not rec["decided"]:
                    del trace[t0:]
                for t in trace[t0:]:
                    t["ctu"] = i
            if not rec["decided"]:
                tags["refused_ctu",] += 1
            ctus[i], nodes[i], ctx = rec, nd, after
            depth[r * cells:(r + 1) * cells, x * cells:(x + 1) * cells] = dp
            syntax[i, :3] = ctx
            if wpp and x == 1:
                saved = list(ctx)
    return dict(ctus=ctus, nodes=nodes, depth=depth, cu_syntax=syntax)


def choice_records(outcome, rate, dist):
    """havoc_mi355x_cu_choice records as cu_close leaves them, from what the quadtree reads of them"""
    rec = np.zeros(len(outcome), CHOICE_DT)
    ok = np.asarray(outcome) != REFUSED
    rec["outcome"], rec["have_residual"] = outcome, np.asarray(outcome) == CODED
    rec["rate"], rec["lambda_distortion"] = np.where(ok, rate, -1), np.where(ok, dist, -1)
    rec["cost"] = rec["cost_no_residual"] = np.where(ok, np.asarray(rate, np.int64) + dist, -1)
    rec["cost_coded"] = -1
    return rec


def make_case(seed, width, height, ctb_log2, min_cb_log2, flags, p_candidate=0.8, p_skipped=0.25, refuse=(), equalise=(), bare=()):
    """the inputs of one call: random candidates whose cost grows with their area, so that single units and splits both win at every depth.  Nodes at MinCb always
    have a candidate, except in the CTUs of `refuse`, whose first MinCb node and all its ancestors have none (through -1, an index past the records, or a refused
    record, in turn).  bare: (ctu, node) pairs: the node has a candidate and no node below it has one.  equalise: (ctu, node) pairs in coding order: the node's candidate gets the rate that makes the two costs equal."""
    rng = np.random.default_rng(seed)
    case = dict(width=width, height=height, ctb_log2=ctb_log2, min_cb_log2=min_cb_log2, flags=flags)
    levels, cells, cx, cy, count = geometry(case)
    case["cu_syntax"] = rng.integers(0, 126, SYNTAX_BYTES).astype(np.uint8)
    outcome, rate, dist, node_cu = [REFUSED, REFUSED], [0, 0], [0, 0], np.full((cx * cy, count), -1, np.int32)
    for i in range(cx * cy):
        for d in range(levels):
            area = 4 ** (levels - 1 - d)
            for z in range(4 ** d):
                if i in refuse and z == 0:
                    node_cu[i, first(d) + z] = (-1, 1 << 20, 1)[(list(refuse).index(i) + d) % 3]
                    continue
                if any(i == bi and d > bd and z >> 2 * (d - bd) == bk - first(bd) for bi, bk in bare for bd in [depth_of(bk)]):
                    continue
                if d < levels - 1 and (i, first(d) + z) not in equalise and (i, first(d) + z) not in bare and rng.random() >= p_candidate:
                    continue
                cost = int(area * 40000 * rng.uniform(0.5, 1.5)) + 30000
                r = int(cost * rng.uniform(0.1, 0.9))
                node_cu[i, first(d) + z] = len(outcome)
                outcome.append(SKIPPED if rng.random() < p_skipped else int(rng.integers(0, 2)))
                rate.append(r)
                dist.append(cost - r)
    # the records in another order than the nodes
    m = len(outcome)
    order = rng.permutation(m)
    where = np.empty(m, np.int64)
    where[order] = np.arange(m)
    node_cu = np.where((node_cu >= 0) & (node_cu < m), where[np.clip(node_cu, 0, m - 1)], node_cu).astype(np.int32)
    case["node_cu"] = node_cu
    case["choice"] = choice_records(np.array(outcome)[order], np.array(rate, np.int64)[order], np.array(dist, np.int64)[order])
    for i, k in equalise:
        idx = int(node_cu[i, k])
        assert idx >= 0 and case["choice"][idx]["outcome"] != REFUSED, "an equalised node needs a candidate"
        case["choice"][idx]["outcome"], case["choice"][idx]["have_residual"] = CODED, 1         # no ecu stop: the split must be tried
        n = decide_picture(case)["nodes"][i, k]
        assert n["cost_split"] >= 0 and n["cost_full"] >= 0, (i, k, n)
        dist = int(case["choice"][idx]["lambda_distortion"])
        total = int(case["choice"][idx]["rate"]) + dist + int(n["cost_split"]) - int(n["cost_full"])        # what the unit must cost
        assert total >= 0
        dist = min(dist, total // 2)
        case["choice"][idx]["rate"], case["choice"][idx]["lambda_distortion"] = total - dist, dist
        case["choice"][idx]["cost"] = case["choice"][idx]["cost_no_residual"] = total
        n = decide_picture(case)["nodes"][i, k]
        assert n["cost_split"] == n["cost_full"] and n["choice"] == CU, (i, k, n)
    return case


# the golden file's cases and the fresh ones of the GPU tests: name -> make_case's arguments.  136x72 at CTB 64 / MinCb 8 is 3 x 2 CTUs with both partial edges, a
# cell wide and high: must-splits and deleted children at every depth; its CTU 0 holds the equalised nodes (depth 2, 1, 0 in coding order), CTU 1 is refused; the
# raster case has a CTU that is one bare 64x64 unit and bare nodes at depth 1 and 2.
# 64x136 is one CTU wide and three high: a WPP row there starts from the slice's contexts.
CASES = {
    "136x72_wpp": dict(seed=1, width=136, height=72, ctb_log2=6, min_cb_log2=3, flags=WPP, refuse=(1,), equalise=((0, 5), (0, 1), (0, 0))),
    "136x72_ecu_raster": dict(seed=2, width=136, height=72, ctb_log2=6, min_cb_log2=3, flags=ECU, refuse=(4,), bare=((0, 0), (1, 2), (1, 7))),
    "72x40_wpp_ecu": dict(seed=3, width=72, height=40, ctb_log2=5, min_cb_log2=3, flags=WPP | ECU, equalise=((0, 1), (0, 0))),
    "40x24_wpp": dict(seed=4, width=40, height=24, ctb_log2=4, min_cb_log2=3, flags=WPP, refuse=(3,), equalise=((0, 0),)),
    "64x64_wpp": dict(seed=5, width=64, height=64, ctb_log2=6, min_cb_log2=3, flags=WPP),
    "64x64_raster": dict(seed=5, width=64, height=64, ctb_log2=6, min_cb_log2=3, flags=0),
    "64x136_wpp": dict(seed=6, width=64, height=136, ctb_log2=6, min_cb_log2=3, flags=WPP),
    "64x136_raster": dict(seed=6, width=64, height=136, ctb_log2=6, min_cb_log2=3, flags=0),
    "48x48_min16": dict(seed=7, width=48, height=48, ctb_log2=5, min_cb_log2=4, flags=WPP),
    "rows_12x6": dict(seed=8, width=384, height=192, ctb_log2=5, min_cb_log2=3, flags=WPP | ECU, refuse=(30,), bare=((5, 0), (6, 3), (40, 2))),
}
RESULT_KEYS = ("ctus", "nodes", "depth", "cu_syntax")


def required_tags():
    """the branches the golden inputs must reach between them, at every depth where each can occur (four levels: a decision at depth 0..2, a child at 1..3)"""
    need = [(kind, d) for kind in ("cu_wins", "split_wins", "equal_keeps_cu", "ecu_stop", "no_candidate_split", "no_split_candidate") for d in range(3)]
    need += [("must_split", where, d) for where in ("right", "bottom", "corner") for d in range(3)]
    need += [("deleted", where, d) for where in ("right", "below", "corner") for d in range(1, 4)]
    need += [("ctx_inc", v) for v in range(3)]
    return need + [("flag_not_coded_min_cb",), ("refused_ctu",), ("wpp_start_ctu1",), ("wpp_start_slice",), ("raster_carry",)]


def golden_path():
    return os.path.join(ROOT, "tests", "golden", "cqt_golden.npz")


def pack(case, res):
    """a case and its recorded results as the flat arrays of the golden file: what the quadtree reads of the records, in the narrowest types that hold it"""
    ch, nd = case["choice"], res["nodes"]
    out = dict(params=np.array([case[k] for k in ("width", "height", "ctb_log2", "min_cb_log2", "flags")], np.int32), cu_syntax=case["cu_syntax"],
               node_cu=case["node_cu"], outcome=ch["outcome"].astype(np.int8), rate=ch["rate"].astype(np.int32), dist=ch["lambda_distortion"].astype(np.int32),
               ctus=res["ctus"].view(np.uint8), node_bytes=np.stack([nd["choice"], nd["flags"], nd["ctx_inc"]], -1), cost_full=nd["cost_full"].astype(np.int32),
               cost_split=nd["cost_split"].astype(np.int32), depth=res["depth"], syntax3=res["cu_syntax"][:, :3])
    assert all(np.array_equal(out[k], ch[f]) for k, f in (("rate", "rate"), ("dist", "lambda_distortion")))
    assert np.array_equal(out["cost_full"], nd["cost_full"]) and np.array_equal(out["cost_split"], nd["cost_split"])
    return out


def unpack(g, name):
    """-> (case, recorded results) of the golden file's case `name`"""
    a = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + ".")}
    p = [int(v) for v in a["params"]]
    case = dict(width=p[0], height=p[1], ctb_log2=p[2], min_cb_log2=p[3], flags=p[4], cu_syntax=a["cu_syntax"], node_cu=a["node_cu"],
                choice=choice_records(a["outcome"].astype(np.int32), a["rate"].astype(np.int64), a["dist"].astype(np.int64)))
    nodes = np.zeros(a["node_bytes"].shape[:2], NODE_DT)
    nodes["choice"], nodes["flags"], nodes["ctx_inc"] = a["node_bytes"][..., 0], a["node_bytes"][..., 1], a["node_bytes"][..., 2]
    nodes["cost_full"], nodes["cost_split"] = a["cost_full"], a["cost_split"]
    syntax = np.tile(case["cu_syntax"], (len(nodes), 1))
    syntax[:, :3] = a["syntax3"]
    return case, dict(ctus=a["ctus"].view(CTU_DT).copy(), nodes=nodes, depth=a["depth"], cu_syntax=syntax)


def same(got, want):
    """every CTU record, node record, depth cell and snapshot byte; -> the first key that differs, or None"""
    for k in RESULT_KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.tobytes() != b.tobytes():
            return k
    return None


class Shim:
    """tests/cqt_shim.cpp over the reference's turing/SyntaxCtu.hpp, Binarization.h, Write.h, StateSpatial.h, Snake.h and Cabac.cpp, built with oracle/Makefile's TURFLAGS"""

    def __init__(self):
        ref = T.reference_dir()
        assert ref, "reference sources not present"
        self._tmp = tempfile.TemporaryDirectory()
        so = os.path.join(self._tmp.name, "libcqt.so")
        flags = T._make_var("TURFLAGS").split()
        subprocess.check_call(["g++"] + flags + ["-shared", "-o", so, os.path.join(ROOT, "tests", "cqt_shim.cpp")]
                              + [os.path.join(ref, "turing", f) for f in ("Cabac.cpp", "ScanOrder.cpp")])
        L = self.L = C.CDLL(so)
        L.cqt_snake_after_reset.restype = None
        L.cqt_snake_after_reset.argtypes = [C.c_int] * 6 + [C.c_void_p]
        L.cqt_flag.restype = C.c_int64
        L.cqt_flag.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.cqt_open.restype = C.c_void_p
        L.cqt_open.argtypes = [C.c_int] * 4
        L.cqt_close.restype = None
        L.cqt_close.argtypes = [C.c_void_p]
        L.cqt_commit.restype = None
        L.cqt_commit.argtypes = [C.c_void_p] + [C.c_int] * 4
        L.cqt_ctu.restype = C.c_int64
        L.cqt_ctu.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]

    def snake_after_reset(self, case, x, y):
        """CtDepth the freshly reset snake answers (left of, above) the luma position (x, y)"""
        out = np.zeros(2, np.int32)
        self.L.cqt_snake_after_reset(case["width"], case["height"], case["ctb_log2"], case["min_cb_log2"], x, y, out.ctypes.data)
        return int(out[0]), int(out[1])

    def flag(self, case, t):
        """one traced flag by the reference's writer -> (bits, states after, ctxInc, CtDepth answered left, above)"""
        p = np.array([case["width"], case["height"], case["ctb_log2"], case["min_cb_log2"], t["x0"], t["y0"], t["log2"], t["depth"], t["left"], t["up"], t["bin"]], np.int32)
        states, out = np.array(t["before"], np.uint8), np.zeros(3, np.int32)
        bits = self.L.cqt_flag(p.ctypes.data, states.ctypes.data, out.ctypes.data)
        return int(bits), [int(v) for v in states], int(out[0]), int(out[1]), int(out[2])

    def picture(self, case, res):
        """the reference's Syntax<coding_quadtree>::go over the decided tree of every CTU in coding order (turing/Write.h:806-812): split_cu_flag from res["depth"],
        the units' rates from the candidates, the contexts handed from CTU to CTU as decide_picture does -> (rate [n], states after [n, 3]); a refused CTU is not
        walked: its cells are committed with CtDepth 0 and it reports rate 0 and the states as they came"""
        levels, cells, cx, cy, count = geometry(case)
        ctb, mcb = case["ctb_log2"], case["min_cb_log2"]
        wpp = bool(case["flags"] & WPP)
        depth = np.ascontiguousarray(res["depth"], np.int8)
        h = self.L.cqt_open(case["width"], case["height"], ctb, mcb)
        initial = np.array(case["cu_syntax"][:3], np.uint8)
        ctx, saved = initial.copy(), None
        rates, states = np.zeros(cx * cy, np.int64), np.zeros((cx * cy, 3), np.uint8)
        for r in range(cy):
            for x in range(cx):
                i = r * cx + x
                if x == 0 and r > 0 and wpp:
                    ctx = (saved if cx >= 2 else initial).copy()
                if res["ctus"][i]["decided"]:
                    node_rate = np.array([c[0] if c else 0 for c in candidates(case, i)], np.int64)
                    rates[i] = self.L.cqt_ctu(h, x << ctb, r << ctb, ctx.ctypes.data, depth.ctypes.data, depth.shape[1], node_rate.ctypes.data)
                else:
                    for cy_ in range(min(cells, (case["height"] >> mcb) - r * cells)):
                        for cx_ in range(min(cells, (case["width"] >> mcb) - x * cells)):
                            self.L.cqt_commit(h, (x << ctb) + (cx_ << mcb), (r << ctb) + (cy_ << mcb), 1 << mcb, 0)
                states[i] = ctx
                if wpp and x == 1:
                    saved = ctx.copy()
        self.L.cqt_close(h)
        return rates, states


def bin_table():
    """[2 state + bin] = new state | Q16 rate << 8: the walk's table (cabac_tables.h: bin_entry)"""
    t = np.zeros(256, np.int32)
    for s in range(128):
        for b in range(2):
            ns, bits = bin_cost(s, b)
            t[2 * s + b] = ns | bits << 8
    return t


class DecisionClient:
    """tests/cqt_client.cpp: search/cqt_decision.hpp's decideCqt, compiled at test time"""

    def __init__(self):
        self._tmp = tempfile.TemporaryDirectory()
        so = os.path.join(self._tmp.name, "libcqt_client.so")
        subprocess.check_call(["g++", "-O1", "-std=c++14", "-fPIC", "-shared", "-Wall", "-o", so, os.path.join(ROOT, "tests", "cqt_client.cpp")])
        self.L = C.CDLL(so)
        self.L.cqt_decide_ctu.restype = C.c_int
        self.L.cqt_decide_ctu.argtypes = [C.c_void_p] * 9
        self.bins = bin_table()

    def decide_ctu(self, cand, ctx, left, up, levels, cells_x, cells_y, ecu):
        """-> what cqt_tools.decide_ctu gives"""
        count, cells = n_nodes(levels), 1 << (levels - 1)
        g = np.array([levels, cells_x, cells_y, ecu], np.int32)
        c = np.array([[1, c[2], c[0], c[1]] if c else [0, 0, 0, 0] for c in cand], np.int64)
        states, out, nodes, depth = np.array(ctx, np.uint8), np.zeros(6, np.int64), np.zeros((count, 5), np.int64), np.zeros((8, 8), np.int8)
        l8, u8 = np.full(8, -1, np.int8), np.full(8, -1, np.int8)
        l8[:cells], u8[:cells] = left[:cells], up[:cells]
        assert self.L.cqt_decide_ctu(g.ctypes.data, c.ctypes.data, self.bins.ctypes.data, states.ctypes.data, l8.ctypes.data, u8.ctypes.data, out.ctypes.data,
                                     nodes.ctypes.data, depth.ctypes.data) == 0
        rec, nd = np.zeros(1, CTU_DT)[0], np.zeros(count, NODE_DT)
        rec["decided"], rec["n_cus"], rec["rate"], rec["flag_rate"], rec["lambda_distortion"], rec["cost"] = out
        nd["choice"], nd["flags"], nd["ctx_inc"], nd["cost_full"], nd["cost_split"] = nodes.T
        return rec, nd, depth[:cells, :cells].copy(), [int(v) for v in states]

    def decide_picture(self, case):
        """decide_picture with every CTU walked by decideCqt"""
        levels, cells, cx, cy, count = geometry(case)
        wc, hc = case["width"] >> case["min_cb_log2"], case["height"] >> case["min_cb_log2"]
        wpp, ecu = bool(case["flags"] & WPP), bool(case["flags"] & ECU)
        initial = [int(v) for v in case["cu_syntax"][:3]]
        ctx, saved = list(initial), None
        depth = np.zeros((cy * cells, cx * cells), np.int8)
        ctus, nodes = np.zeros(cx * cy, CTU_DT), np.zeros((cx * cy, count), NODE_DT)
        syntax = np.tile(np.asarray(case["cu_syntax"], np.uint8), (cx * cy, 1))
        for r in range(cy):
            for x in range(cx):
                i = r * cx + x
                if x == 0 and r > 0 and wpp:
                    ctx = list(saved if cx >= 2 else initial)
                left = depth[r * cells:(r + 1) * cells, x * cells - 1] if x > 0 else np.full(cells, -1)
                up = depth[r * cells - 1, x * cells:(x + 1) * cells] if r > 0 else np.full(cells, -1)
                ctus[i], nodes[i], dp, ctx = self.decide_ctu(candidates(case, i), ctx, left, up, levels, min(cells, wc - x * cells), min(cells, hc - r * cells), ecu)
                depth[r * cells:(r + 1) * cells, x * cells:(x + 1) * cells] = dp
                syntax[i, :3] = ctx
                if wpp and x == 1:
                    saved = list(ctx)
        return dict(ctus=ctus, nodes=nodes, depth=depth, cu_syntax=syntax)
