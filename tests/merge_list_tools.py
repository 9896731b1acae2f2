"""havoc_mi355x_cqt_merge_lists restated in python integers (include/havoc_mi355x.h).  Test infrastructure.

`merge_lists` is the call restated -- which searched units are final, which neighbour positions a unit may read (the availability rule in this file's own words:
picture edges, CTU order, z-order by Morton index of the unit's ORIGIN), what a committed cell and the two temporal records give, and the list (spatial candidates
with their pruning, the temporal candidate, combined and zero candidates) -- sharing no line with search/merge_list.hpp, tests/merge.hpp or search/picture_order.hpp,
with the branch every unit takes counted by name in `tags`.  `make_case` writes seeded committed cell maps directly: random quadtrees per CTU whose EVERY visited node is
a searched unit (as the product's unit table has them: the parents of a split are units that are not final), vectors from a small pool so that neighbours are often
equal, CTUs left undecided.  `Client` compiles tests/merge_list_client.cpp (the host form cqtMergeList, and merge_list.hpp beside tests/merge.hpp on rows);
`random_rows` makes the rows of that comparison.
"""
import collections
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# include/havoc_mi355x.h: havoc_mi355x_cqt_cell, _temporal_cand, _merge_cand, _merge_list, _merge_params; search/search_abi.h: havoc_picture_pu
CQT_CELL_DT = np.dtype([("unit", "<i4"), ("cand", "<i4"), ("mv", "<i2", (2, 2)), ("log2_size", "u1"), ("outcome", "u1"), ("pred", "u1"), ("tr_depth", "u1"), ("cbf", "<u4")])
TEMPORAL_CAND_DT = np.dtype([("mv", "<i2", (2,)), ("available", "<i2"), ("source", "<i2")])
PU_DT = np.dtype([("x0", "i4"), ("y0", "i4"), ("w", "i4"), ("h", "i4"), ("cu_log2_size", "i4"), ("cqt_depth", "i4"), ("part_2Nx2N", "i4"), ("reserved", "i4")])
MERGE_CAND_DT = np.dtype([("mv", "<i2", (2, 2)), ("pred_flag", "u1", (2,)), ("ref_idx", "i1", (2,))])
MERGE_LIST_DT = np.dtype([("cand", MERGE_CAND_DT, (5,)), ("n_cand", "i1"), ("n_real", "i1"), ("match", "i1"), ("reserved", "u1")])
MERGE_PARAMS_DT = np.dtype([("pic_width", "<i4"), ("pic_height", "<i4"), ("ctb_log2", "<i4"), ("min_cb_log2", "<i4"), ("max_cand", "<i4"), ("ref_poc", "<i4", (2,)),
                            ("reserved", "<i4", (5,))])
assert (CQT_CELL_DT.itemsize, TEMPORAL_CAND_DT.itemsize, PU_DT.itemsize, MERGE_CAND_DT.itemsize, MERGE_LIST_DT.itemsize, MERGE_PARAMS_DT.itemsize) == (24, 8, 32, 12, 64, 48)
SENTINEL = 0xA5         # every byte of a destination before the call
NAMES = ("A1", "B1", "B0", "A0", "B2")
COMB = ((0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1), (0, 3), (3, 0), (1, 3), (3, 1), (2, 3), (3, 2))      # combIdx -> (l0CandIdx, l1CandIdx), HEVC table 8-7

REQUIRED_TAGS = (tuple("%s_taken" % n for n in NAMES) + tuple("%s_unavailable" % n for n in NAMES) +
                 ("B1_pruned_A1", "B0_pruned_B1", "A0_pruned_A1", "B2_pruned_A1", "B2_pruned_B1", "B2_skipped_four") +
                 tuple("full_at_%s" % n for n in NAMES + ("col", "combined")) + tuple("full_early_max%d" % m for m in range(1, 6)) +
                 ("col_l0_only", "col_l1_only", "col_both", "col_none", "col_no_table") +
                 tuple("comb%d_accepted" % c for c in range(12)) + tuple("comb%d_rejected" % c for c in range(12)) +
                 tuple("zero_fill_%d" % k for k in range(1, 6)) +
                 ("left_of_picture", "above_picture", "right_of_picture", "ctu_does_not_precede", "next_ctu_row", "later_in_z_order", "neighbour_undecided", "own_undecided") +
                 tuple("match_%d" % k for k in range(5)) + ("match_none", "match_combined", "match_zero") +
                 ("not_final_parent_of_a_split", "not_final_shape", "final_8", "final_16", "final_32", "final_64"))


def _morton(x, y):
    m = 0
    for b in range(8):
        m |= (x >> b & 1) << 2 * b | (y >> b & 1) << 2 * b + 1
    return m


def position_readable(W, H, ctb_log2, x0, y0, xN, yN, tags):
    """may the unit with origin (x0, y0) read the position?  One slice, one tile, wavefront order: inside the picture; in a CTU of an earlier row, or of this row further
    left, or in this CTU at an earlier Morton index than the unit's origin (the unit is an aligned square: what lies outside it is wholly before or wholly after it)"""
    if xN < 0:
        tags["left_of_picture"] += 1
        return False
    if yN < 0:
        tags["above_picture"] += 1
        return False
    if xN >= W:
        tags["right_of_picture"] += 1
        return False
    if yN >= H:
        tags["below_picture"] += 1
        return False
    (cxN, cyN), (cx, cy) = (xN >> ctb_log2, yN >> ctb_log2), (x0 >> ctb_log2, y0 >> ctb_log2)
    if cyN > cy:
        tags["next_ctu_row"] += 1
        return False
    if cyN < cy:
        tags["in_an_earlier_ctu_row"] += 1
        return True
    if cxN > cx:
        tags["ctu_does_not_precede"] += 1
        return False
    if cxN < cx:
        tags["in_the_ctu_to_the_left"] += 1
        return True
    mask = (1 << ctb_log2) - 1
    if _morton(xN & mask, yN & mask) > _morton(x0 & mask, y0 & mask):
        tags["later_in_z_order"] += 1
        return False
    return True


def _motion_of(cell):
    """a committed cell as motion: (predFlag0, predFlag1, (mv0 x, y), (mv1 x, y)); reference index 0 in the lists it uses, an unused list's vector zero"""
    pred = int(cell["pred"])
    f0, f1 = pred != 1, pred != 0
    return (f0, f1, (int(cell["mv"][0, 0]), int(cell["mv"][0, 1])) if f0 else (0, 0), (int(cell["mv"][1, 0]), int(cell["mv"][1, 1])) if f1 else (0, 0))


def _equal(a, b):
    """the reference's comparison of two units' motion: the same lists, and in a used list the same vector (the reference index is 0 everywhere)"""
    return a[0] == b[0] and a[1] == b[1] and (not a[0] or a[2] == b[2]) and (not a[1] or a[3] == b[3])


NOTHING = (False, False, (0, 0), (0, 0))


def derive_list(nb, col, max_cand, same_poc, tags):
    """nb: five motions A1, B1, B0, A0, B2 (NOTHING: no neighbour); col: a motion or None -> (the max_cand candidates, how many are not zero candidates, the kind of every
    place: 's' spatial, 't' temporal, 'c' combined, 'z' zero)"""
    out, kind = [], []
    a1, b1, b0, a0, b2 = nb

    def full(where):
        if len(out) == max_cand:
            tags["full_at_%s" % where] += 1
            tags["full_early_max%d" % max_cand] += 1
            tags["full_at_%s_max%d" % (where, max_cand)] += 1
            return True
        return False

    steps = (("A1", a1, ()), ("B1", b1, (("A1", a1),)), ("B0", b0, (("B1", b1),)), ("A0", a0, (("A1", a1),)), ("B2", b2, (("A1", a1), ("B1", b1))))
    for name, m, against in steps:
        if name == "B2" and len(out) == 4:
            tags["B2_skipped_four"] += 1
            continue
        if not (m[0] or m[1]):
            tags["%s_unavailable" % name] += 1
            continue
        twin = [other for other, o in against if _equal(m, o)]
        if twin:
            tags["%s_pruned_%s" % (name, twin[0])] += 1
            continue
        out.append(m)
        kind.append("s")
        tags["%s_taken" % name] += 1
        if full(name):
            return out, len(out), kind
    if col is not None and (col[0] or col[1]):
        out.append(col)
        kind.append("t")
        if full("col"):
            return out, len(out), kind
    first = len(out)
    for c, (i, j) in enumerate(COMB):
        if c >= first * (first - 1):
            break
        p, q = out[i], out[j]
        if not (p[0] and q[1]):
            tags["comb%d_not_applicable" % c] += 1
            continue
        if same_poc and p[2] == q[3]:
            tags["comb%d_rejected" % c] += 1
            continue
        tags["comb%d_accepted" % c] += 1
        out.append((True, True, p[2], q[3]))
        kind.append("c")
        if full("combined"):
            return out, len(out), kind
    real = len(out)
    tags["zero_fill_%d" % (max_cand - real)] += 1
    while len(out) < max_cand:
        out.append((True, True, (0, 0), (0, 0)))
        kind.append("z")
    return out, real, kind


def merge_lists(params, cells, pus, temporal=None, tags=None):
    """havoc_mi355x_cqt_merge_lists restated; params: one MERGE_PARAMS_DT record, cells: CQT_CELL_DT [H >> min, W >> min], pus: PU_DT [n], temporal: TEMPORAL_CAND_DT
    [n, 2] or None -> MERGE_LIST_DT [n]"""
    tags = collections.Counter() if tags is None else tags
    P = np.asarray(params).reshape(1)[0]
    W, H, ctb, mcb, max_cand = (int(P[k]) for k in ("pic_width", "pic_height", "ctb_log2", "min_cb_log2", "max_cand"))
    same_poc = int(P["ref_poc"][0]) == int(P["ref_poc"][1])
    out = np.zeros(len(pus), MERGE_LIST_DT)
    out["match"] = -1
    for p, u in enumerate(pus):
        x0, y0, w, h = (int(u[k]) for k in ("x0", "y0", "w", "h"))
        sizes = {1 << L: L for L in range(mcb, ctb + 1)}
        if w != h or w not in sizes or x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H or x0 % w or y0 % h:
            tags["not_final_shape"] += 1
            continue
        own = cells[y0 >> mcb, x0 >> mcb]
        if own["unit"] < 0:
            tags["own_undecided"] += 1
            continue
        if own["unit"] != p or own["log2_size"] != sizes[w]:
            tags["not_final_parent_of_a_split" if own["log2_size"] < sizes[w] else "not_final_other"] += 1
            continue
        tags["final_%d" % w] += 1
        nb = []
        for xN, yN in ((x0 - 1, y0 + h - 1), (x0 + w - 1, y0 - 1), (x0 + w, y0 - 1), (x0 - 1, y0 + h), (x0 - 1, y0 - 1)):
            m = NOTHING
            if position_readable(W, H, ctb, x0, y0, xN, yN, tags):
                c = cells[yN >> mcb, xN >> mcb]
                if c["unit"] < 0:
                    tags["neighbour_undecided"] += 1
                else:
                    m = _motion_of(c)
            nb.append(m)
        col = None
        if temporal is None:
            tags["col_no_table"] += 1
        else:
            t0, t1 = temporal[p, 0], temporal[p, 1]
            f0, f1 = bool(t0["available"]), bool(t1["available"])
            col = (f0, f1, (int(t0["mv"][0]), int(t0["mv"][1])) if f0 else (0, 0), (int(t1["mv"][0]), int(t1["mv"][1])) if f1 else (0, 0))
            tags["col_both" if f0 and f1 else "col_l0_only" if f0 else "col_l1_only" if f1 else "col_none"] += 1
        lst, real, kind = derive_list(nb, col, max_cand, same_poc, tags)
        r = out[p]
        r["n_cand"], r["n_real"] = max_cand, real
        for k, m in enumerate(lst):
            r["cand"][k]["pred_flag"], r["cand"][k]["mv"] = (m[0], m[1]), (m[2], m[3])
        mine = _motion_of(own)
        hits = [k for k, m in enumerate(lst) if _equal(m, mine)]
        r["match"] = hits[0] if hits else -1
        tags["match_%d" % hits[0] if hits else "match_none"] += 1
        if hits and kind[hits[0]] == "c":
            tags["match_combined"] += 1
        if hits and kind[hits[0]] == "z":
            tags["match_zero"] += 1
    return out


# ================================================================================================================== the cases
def make_params(W, H, ctb_log2, max_cand, ref_poc, min_cb_log2=3):
    p = np.zeros(1, MERGE_PARAMS_DT)
    p["pic_width"], p["pic_height"], p["ctb_log2"], p["min_cb_log2"], p["max_cand"], p["ref_poc"] = W, H, ctb_log2, min_cb_log2, max_cand, ref_poc
    return p


POOL_SMALL = ((0, 0), (4, 0))                                                       # two vectors: neighbours are equal half the time, combined candidates get rejected
POOL_WIDE = ((0, 0), (4, 0), (0, -8), (3, 3), (-9, 2), (17, -1))
POOL_ENDS = ((32767, -32768), (-32768, 32767), (32767, 32767), (-32768, -32768), (0, 0))      # the ends of the 16-bit range


def make_case(seed, W, H, ctb_log2, max_cand, ref_poc, pool=POOL_WIDE, pred_p=(0.4, 0.3, 0.3), split_p=0.55, undecided=(), col_p=(0.25, 0.25, 0.25, 0.25), extra=2):
    """-> dict(params, cells, pus, temporal, extra).  A random quadtree per CTU; EVERY visited node is a unit of the table (a parent before its four children, CTUs in
    raster order), the leaves are the final units; `undecided`: CTUs (raster index) whose cells stay all-ones bytes -- their units are in the table all the same.  Then
    `extra` units that cannot be final: one outside the picture, one that is not square.  temporal: per (unit, list) available by col_p = P(none, L0, L1, both)"""
    rng = np.random.default_rng(seed + 5000)
    cells = np.zeros((H >> 3, W >> 3), CQT_CELL_DT)
    cells.view(np.uint8)[...] = 0xff
    pus = []
    cx = -(-W >> ctb_log2)

    def node(x, y, L, wiped):
        size = 1 << L
        if x >= W or y >= H:
            return
        inside = x + size <= W and y + size <= H
        p = None
        if inside:
            p = len(pus)
            pus.append((x, y, size, size, L, ctb_log2 - L, 1, 0))
        if L > 3 and (not inside or rng.random() < split_p):
            for k in range(4):
                node(x + (k & 1) * size // 2, y + (k >> 1) * size // 2, L - 1, wiped)
            return
        q = np.zeros(1, CQT_CELL_DT)[0]
        q["unit"], q["cand"], q["log2_size"] = p, int(rng.integers(0, 1 << 20)), L
        q["pred"], q["outcome"] = rng.choice(3, p=pred_p), rng.integers(0, 3)
        for l in (0, 1):
            if q["pred"] in (l, 2):
                q["mv"][l] = pool[int(rng.integers(0, len(pool)))]
        q["cbf"] = int(rng.integers(0, 1 << 12)) if q["outcome"] == 0 else 0
        if not wiped:
            cells[y >> 3:(y + size) >> 3, x >> 3:(x + size) >> 3] = q

    for j, y in enumerate(range(0, H, 1 << ctb_log2)):
        for i, x in enumerate(range(0, W, 1 << ctb_log2)):
            node(x, y, ctb_log2, j * cx + i in undecided)
    for e in ((W, 0, 8, 8, 3, ctb_log2 - 3, 1, 0), (0, 0, 16, 8, 4, ctb_log2 - 4, 0, 0))[:extra]:
        pus.append(e)
    pus = np.array([tuple(u) for u in pus], PU_DT)
    temporal = np.zeros((len(pus), 2), TEMPORAL_CAND_DT)
    kinds = rng.choice(4, len(pus), p=col_p)
    for l in (0, 1):
        have = (kinds == l + 1) | (kinds == 3)
        temporal["available"][:, l] = have
        temporal["source"][:, l] = np.where(have, 2, 0)
        temporal["mv"][:, l] = np.where(have[:, None], np.array(pool)[rng.integers(0, len(pool), len(pus))], 0)
    return dict(params=make_params(W, H, ctb_log2, max_cand, ref_poc), cells=cells, pus=pus, temporal=temporal, extra=extra)


# name -> make_case's arguments.  Pictures 64x64, 72x40 and 136x72 (edges that are no CTU multiples) at CTB 64, 32 and 16; max_cand 1..5; equal and different picture
# order counts; the two-vector pool (pruning, rejected combinations, a unit's own motion among its candidates), the wide pool, the ends of the 16-bit range; undecided
# CTUs; a picture of one unit (n == 1 without the extras).  Together they reach every tag of REQUIRED_TAGS (tests/test_merge_list.py asserts it)
CASES = {
    "136x72_ctb64_max5_same_poc": dict(seed=1, W=136, H=72, ctb_log2=6, max_cand=5, ref_poc=(8, 8), pool=POOL_SMALL),
    "136x72_ctb64_max5_same_poc_b": dict(seed=2, W=136, H=72, ctb_log2=6, max_cand=5, ref_poc=(8, 8), pool=POOL_SMALL, pred_p=(0.2, 0.2, 0.6), split_p=0.8),
    "136x72_ctb32_max5_same_poc": dict(seed=3, W=136, H=72, ctb_log2=5, max_cand=5, ref_poc=(0, 0), pool=POOL_SMALL, pred_p=(0.3, 0.3, 0.4), split_p=0.7),
    "136x72_ctb16_max5": dict(seed=4, W=136, H=72, ctb_log2=4, max_cand=5, ref_poc=(0, 16), pool=POOL_SMALL),
    "136x72_ctb64_max5_wide": dict(seed=5, W=136, H=72, ctb_log2=6, max_cand=5, ref_poc=(0, 16), split_p=0.75),
    "136x72_ctb64_max4_undecided": dict(seed=6, W=136, H=72, ctb_log2=6, max_cand=4, ref_poc=(0, 16), undecided=(1,), split_p=0.8),
    "72x40_ctb32_max3": dict(seed=7, W=72, H=40, ctb_log2=5, max_cand=3, ref_poc=(0, 16), pool=POOL_SMALL, split_p=0.7),
    "72x40_ctb16_max2": dict(seed=8, W=72, H=40, ctb_log2=4, max_cand=2, ref_poc=(4, 4), pool=POOL_SMALL),
    "72x40_ctb64_max1": dict(seed=9, W=72, H=40, ctb_log2=6, max_cand=1, ref_poc=(0, 16)),
    "64x64_ctb64_ends": dict(seed=10, W=64, H=64, ctb_log2=6, max_cand=5, ref_poc=(-2 ** 31, 2 ** 31 - 1), pool=POOL_ENDS, split_p=0.9),
    "64x64_ctb32_max5_few": dict(seed=11, W=64, H=64, ctb_log2=5, max_cand=5, ref_poc=(0, 16), pool=POOL_SMALL, col_p=(0.7, 0.1, 0.1, 0.1), split_p=0.3),
    "136x72_ctb64_max5_one_list": dict(seed=111, W=136, H=72, ctb_log2=6, max_cand=5, ref_poc=(8, 8), pool=POOL_SMALL, pred_p=(0.45, 0.45, 0.1), split_p=0.9,
                                       col_p=(0.1, 0.4, 0.4, 0.1)),      # (few bi-predicted units: combinations that do not apply, so that the late ones are reached)
    "136x72_ctb64_max5_all_8x8": dict(seed=13, W=136, H=72, ctb_log2=6, max_cand=5, ref_poc=(0, 16), split_p=1.0),      # (the longest table: 153 final units of 197)
    "64x64_one_unit": dict(seed=12, W=64, H=64, ctb_log2=6, max_cand=5, ref_poc=(0, 16), split_p=0.0, extra=0),
}


def make_ctu_case(cols, rows, motion, undecided, temporal, ctb_log2=4, max_cand=5, ref_poc=(8, 8)):
    """a picture whose every CTU is ONE unit (unit index = the CTU's raster index), written by hand: motion {ctu: (pred, mv0, mv1)} (any other CTU: list 0, vector
    0, 0), undecided CTUs, temporal {ctu: ((available0, mv0), (available1, mv1))} (any other unit: none)"""
    size, n = 1 << ctb_log2, cols * rows
    cells = np.zeros((rows * size >> 3, cols * size >> 3), CQT_CELL_DT)
    pus = np.zeros(n, PU_DT)
    temp = np.zeros((n, 2), TEMPORAL_CAND_DT)
    for c in range(n):
        x, y = c % cols * size, c // cols * size
        pus[c] = (x, y, size, size, ctb_log2, 0, 1, 0)
        pred, mv0, mv1 = motion.get(c, (0, (0, 0), (0, 0)))
        q = np.zeros(1, CQT_CELL_DT)[0]
        q["unit"], q["cand"], q["log2_size"], q["pred"], q["mv"] = c, 7 * c, ctb_log2, pred, (mv0, mv1)
        block = cells[y >> 3:(y + size) >> 3, x >> 3:(x + size) >> 3]
        block[...] = q
        if c in undecided:
            block.view(np.uint8)[...] = 0xff
        for l, (have, mv) in enumerate(temporal.get(c, ((0, (0, 0)), (0, (0, 0))))):
            temp[c, l] = (mv, have, 2 if have else 0)
    return dict(params=make_params(cols * size, rows * size, ctb_log2, max_cand, ref_poc), cells=cells, pus=pus, temporal=temp, extra=0)


# The last two combined candidates, (2, 3) and (3, 2), are ACCEPTED only when every earlier combination is rejected or does not apply, which takes two IDENTICAL
# candidates at places 0 and 1 (worked out by hand: both list-1-only with the vector the later list-0 candidate has).  The rule compares A1 with B1 and B1 with B0, so
# the pair can only be A1 and B0 with B1 missing and B0 there: the CTU above undecided, the CTU above-right decided, the unit a whole CTU (then B2, in the CTU
# above-left, is the third candidate and the temporal candidate the fourth).  3 x 2 CTUs of 16x16, CTU 1 undecided, the unit is CTU 4: A1 = CTU 3, B0 = CTU 2, B2 = CTU 0
_V, _U = (4, 0), (0, 0)
CTU_CASES = {
    "ctu_comb10_accepted": dict(cols=3, rows=2, motion={3: (1, _U, _V), 2: (1, _U, _V), 0: (0, _V, _U), 4: (2, _V, _U)}, undecided=(1,), temporal={4: ((0, _U), (1, _U))}),
    "ctu_comb11_accepted": dict(cols=3, rows=2, motion={3: (1, _U, _V), 2: (1, _U, _V), 0: (1, _U, _U), 4: (2, _V, _U)}, undecided=(1,), temporal={4: ((1, _V), (0, _U))}),
}
CASES.update(CTU_CASES)


def make(name):
    return make_ctu_case(**CASES[name]) if name in CTU_CASES else make_case(**CASES[name])


def restate(case, with_temporal=True, tags=None):
    return merge_lists(case["params"], case["cells"], case["pus"], case["temporal"] if with_temporal else None, tags)


def guarded(want, guard=2):
    """the restated records laid out as a destination with `guard` sentinel records before and after"""
    g = np.full(guard * MERGE_LIST_DT.itemsize, SENTINEL, np.uint8)
    return np.concatenate([g, np.ascontiguousarray(want).view(np.uint8).reshape(-1), g])


# ================================================================================================================== rows for merge_list.hpp beside tests/merge.hpp
def random_rows(seed, n, restricted):
    """int32 [n, 64] in tests/search_client.cpp: client_merge's layout.  restricted: what havoc_mi355x_cqt_merge_lists can meet -- partIdx 0, a square unit of 8..64, a
    B slice, one reference per list, reference index 0; else everything the text covers: second units of a split, 8x4 / 4x8 units, P slices, up to four references per
    list with reference indices into picture order count tables that often agree.  Vectors from a pool of three and, an eighth, the ends of the 16-bit range"""
    rng = np.random.default_rng(seed)
    r = np.zeros((n, 64), np.int32)
    if restricted:
        size = 8 << rng.integers(0, 4, n)
        r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4], r[:, 5] = 0, size, size, 1, 1, 1
    else:
        r[:, 0] = rng.integers(0, 2, n)
        r[:, 1], r[:, 2] = 4 << rng.integers(0, 3, n), 4 << rng.integers(0, 3, n)
        r[:, 3] = rng.random(n) < 0.75
        r[:, 4], r[:, 5] = rng.integers(1, 5, n), rng.integers(1, 5, n)
    r[:, 6], r[:, 7] = rng.integers(1, 6, n), rng.integers(0, 2, n)
    for k in range(6):
        q = r[:, 8 + 8 * k:16 + 8 * k]
        kind = rng.choice(4, n, p=(0.5, 0.17, 0.17, 0.16))      # (half of the neighbours are not there: lists that end early and lists filled with zero candidates)
        q[:, 0], q[:, 1] = (kind == 1) | (kind == 3), (kind == 2) | (kind == 3)
        if not restricted:
            q[:, 2:4] = rng.integers(0, 4, (n, 2))
        mv = rng.integers(-1, 2, (n, 4))
        ends = rng.random((n, 4)) < 0.125
        mv[ends] = rng.choice([-32768, 32767], int(ends.sum()))
        q[:, 4:8] = mv
    r[:, 56:64] = rng.integers(0, 3, (n, 8))
    return r


# ================================================================================================================== the host forms
class Client:
    """tests/merge_list_client.cpp, compiled at test time with plain g++ into a temporary directory"""

    def __init__(self):
        self._tmp = tempfile.TemporaryDirectory()
        so = os.path.join(self._tmp.name, "libmerge_list_client.so")
        subprocess.check_call(["g++", "-O1", "-std=c++14", "-fPIC", "-shared", "-Wall", "-I", os.path.join(ROOT, "turingcodec_amd", "search"), "-o", so,
                               os.path.join(ROOT, "tests", "merge_list_client.cpp")])
        self.L = C.CDLL(so)
        self.L.merge_list_rows.restype = None
        self.L.merge_list_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self.L.cqt_merge_lists_host.restype = None
        self.L.cqt_merge_lists_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]

    def rows(self, rows):
        """-> (merge_list.hpp's lists int32 [n, 5, 8], tests/merge.hpp's, the two return values int32 [n, 2])"""
        rows = np.ascontiguousarray(rows, np.int32)
        new, old, ret = np.zeros((len(rows), 5, 8), np.int32), np.zeros((len(rows), 5, 8), np.int32), np.zeros((len(rows), 2), np.int32)
        self.L.merge_list_rows(rows.ctypes.data, len(rows), new.ctypes.data, old.ctypes.data, ret.ctypes.data)
        return new, old, ret

    def host(self, case, with_temporal=True, guard=2):
        """cqtMergeList over the case's units -> uint8: `guard` sentinel records, the records, `guard` sentinel records"""
        n = len(case["pus"])
        out = np.full((n + 2 * guard) * MERGE_LIST_DT.itemsize, SENTINEL, np.uint8)
        params, cells, pus = np.ascontiguousarray(case["params"]), np.ascontiguousarray(case["cells"]), np.ascontiguousarray(case["pus"])
        temporal = np.ascontiguousarray(case["temporal"]) if with_temporal else None
        self.L.cqt_merge_lists_host(params.ctypes.data, cells.ctypes.data, pus.ctypes.data, n, temporal.ctypes.data if with_temporal else None,
                                    out.ctypes.data + guard * MERGE_LIST_DT.itemsize)
        return out


def private_havoc():
    """-> a Havoc context on a non-blocking stream made HERE through the HIP runtime, not taken from torch's pool of streams.  torch hands its 32 pooled streams out in
    turn and never returns one, so every `Havoc(stream="new")` of a test module moves the streams that LATER tests of the same process receive -- and
    tests/test_step_banded.py needs its two pictures' streams on different hardware queues.  The stream stays alive for the rest of the process (buffers that torch's
    allocator caches are tied to it)"""
    import torch
    from turingcodec_amd import havoc
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    L, _ = havoc._load()
    L.hipStreamCreateWithFlags.restype = C.c_int
    L.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    s = C.c_void_p()
    rc = L.hipStreamCreateWithFlags(C.byref(s), 1)      # hipStreamNonBlocking
    assert rc == 0 and s.value, rc
    return havoc.Havoc(0, stream=s.value)


def golden_path():
    return os.path.join(ROOT, "tests", "golden", "merge_list_golden.npz")
