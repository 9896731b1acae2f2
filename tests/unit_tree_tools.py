"""What the trees of the searched units add to tests/tree_rate_tools.py: the one tree of a 64x64 inter unit (log2CbSize 6 above MaxTbLog2SizeY 5: the transform depth
and the split are inferred, turing/Reconstruct.cpp:1300-1310, so the tree is depth 1's without a split_transform_flag bin -- four 32x32 Y and four 16x16 Cb and Cr
blocks).  Test infrastructure.

tree_rate_tools.tree_rate, geometry and walk_jobs take L = 6 as they are (rate_flags(6) is 0: nothing is coded above MaxTbLog2SizeY); what stops at 5 there is the
list of units and the made cases, which are restated here: `make_cases64` makes the trees, `case_names` names what a tree is, `REQUIRED_CASES` what a set must reach.
"""
import collections

import numpy as np

import tree_rate_tools as TR

L64, DEPTH64 = 6, 1
ENCODER = (1, 2, 5)      # MaxTrafoDepth for inter, MinTbLog2SizeY, MaxTbLog2SizeY: what the shim is given for every 64x64 tree
REQUIRED_CASES = ("zero_tree", "luma_only", "chroma_only", "cb_with_zero_child", "cr_without_cb", "all_twelve", "sdh_on", "sdh_off")


def case_names(mask, sdh):
    """the made cases a tree of cbf mask `mask` (bit k Y block k, 4 + k Cb, 8 + k Cr) belongs to"""
    y, cb, cr = mask & 0xf, mask >> 4 & 0xf, mask >> 8 & 0xf
    names = []
    if mask == 0:
        names.append("zero_tree")
    else:
        names.append("sdh_on" if sdh else "sdh_off")      # (an uncoded tree reads no SDH)
    if y and not (cb or cr):
        names.append("luma_only")
    if (cb or cr) and not y:
        names.append("chroma_only")
    if cb and cb != 0xf:
        names.append("cb_with_zero_child")
    if cr and not cb:
        names.append("cr_without_cb")
    if mask == 0xfff:
        names.append("all_twelve")
    return names


def reached(masks, jobs):
    """-> Counter of case_names over the jobs' trees (masks indexed by out_index)"""
    tags = collections.Counter()
    for job in jobs:
        tags.update(case_names(int(masks[int(job["out_index"])]), int(job["sdh"])))
    return tags


def make_cases64(oracle, seed, count, n_states=7):
    """`count` trees of a 64x64 unit, as tree_rate_tools.make_cases makes them (one in eight without a level, one coded in chroma only, one in luma only, one in Cb
    only), plus, per eight, one with all twelve blocks coded and one coded in Cr without Cb; every tree under the encoder's own set-up (ENCODER), flags 0
    -> (luma, chroma, states, syntax states, jobs, aux)"""
    luma, chroma, states, syntax, jobs, aux = TR.make_cases(oracle, seed, L64, DEPTH64, count, n_states)
    aux["max_trafo_depth"], aux["min_tb"], aux["max_tb"] = ENCODER
    assert (jobs["flags"] == 0).all() and TR.rate_flags(L64, *ENCODER) == 0
    ly, ny, lc, nc = TR.geometry(L64, DEPTH64)
    assert (ly, ny, lc, nc) == (5, 4, 4, 4)
    sy, sc = TR.sizes(L64, DEPTH64)
    rng = np.random.default_rng(seed + 5)
    coded_y = [luma[o:o + (1 << 2 * ly)].copy() for o in range(0, len(luma), 1 << 2 * ly) if luma[o:o + (1 << 2 * ly)].any()]
    coded_c = [chroma[o:o + (1 << 2 * lc)].copy() for o in range(0, len(chroma), 1 << 2 * lc) if chroma[o:o + (1 << 2 * lc)].any()]
    for k in range(count):
        y, cb, cr = luma[k * sy:(k + 1) * sy], chroma[2 * k * sc:(2 * k + 1) * sc], chroma[(2 * k + 1) * sc:(2 * k + 2) * sc]
        if k % 8 == 5:      # every block coded
            for b in range(4):
                if not y[b << 2 * ly:(b + 1) << 2 * ly].any():
                    y[b << 2 * ly:(b + 1) << 2 * ly] = coded_y[int(rng.integers(0, len(coded_y)))]
                for c in (cb, cr):
                    if not c[b << 2 * lc:(b + 1) << 2 * lc].any():
                        c[b << 2 * lc:(b + 1) << 2 * lc] = coded_c[int(rng.integers(0, len(coded_c)))]
        elif k % 8 == 6:    # Cr without Cb
            cb[:] = 0
            if not cr.any():
                b = int(rng.integers(0, 4))
                cr[b << 2 * lc:(b + 1) << 2 * lc] = coded_c[int(rng.integers(0, len(coded_c)))]
    return luma, chroma, states, syntax, jobs, aux


def expected_calls64(mask):
    """the residual_coding calls of a coded 64x64 tree in the syntax's order, from the header's description alone: (x0, y0, log2, cIdx, cbf)"""
    out = []
    for k in range(4):
        x0, y0 = (k & 1) * 32, (k >> 1) * 32
        out += [(x0, y0, 5, 0, mask >> k & 1), (x0, y0, 4, 1, mask >> (4 + k) & 1), (x0, y0, 4, 2, mask >> (8 + k) & 1)]
    return out


# ---- havoc_mi355x_rqt_decide_units: search/tu_decision.hpp's decideRqt over three planes for units of 8x8 .. 64x64, in numpy ---------------------------------
def decide_units(units, zero_at, one_at, sizes, csizes, chroma_at, tree_rate, tree_cbf, rl_q16):
    """tree_rate_tools.decide_tree's records for units of every searched size: a unit of 8 .. 32 is decided there, as it is; a 64x64 unit has depth 1 only (sizes[5]:
    four 32x32 luma candidates at one_at, csizes[4]: four Cb and four Cr at cb_one / cr_one; rate and mask at 2 i + 1) -- one[], cost_one, mask_one, chroma_ssd_one
    as for any unit, depth 0 untried, depth = 1 exactly when the mask is not 0 -> (RQT_RESULT_DT, RQT_TREE_RESULT_DT)"""
    from turingcodec_amd.decisions import RQT_RESULT_DT
    from turingcodec_amd.havoc import RQT_TREE_RESULT_DT
    rec, tree = np.zeros(len(units), RQT_RESULT_DT), np.zeros(len(units), RQT_TREE_RESULT_DT)

    def i32(v):
        return int(np.array(v & 0xFFFFFFFF, np.uint32).view(np.int32))

    for i, u in enumerate(units):
        if int(u["log2_size"]) != L64:
            r, t = TR.decide_tree(units[i:i + 1], zero_at[i:i + 1], one_at[i:i + 1], sizes, csizes, chroma_at[i:i + 1], tree_rate[2 * i:2 * i + 2],
                                  tree_cbf[2 * i:2 * i + 2], rl_q16)
            rec[i], tree[i] = r[0], t[0]
            continue
        s1, c1, j1, a = sizes[5], csizes[4], int(one_at[i]), chroma_at[i]
        ssd = 0
        for k in range(4):
            rec[i]["one"][k]["cbf"], rec[i]["one"][k]["ssd"] = int(s1["cbf"][j1 + k]), int(s1["ssd"][j1 + k])
            ssd += int(s1["ssd"][j1 + k])
        chroma = sum(int(c1["ssd"][a["cb_one"] + k]) + int(c1["ssd"][a["cr_one"] + k]) for k in range(4))
        tree[i]["mask_one"], tree[i]["chroma_ssd_one"] = tree_cbf[2 * i + 1], i32(chroma)
        rec[i]["cost_one"] = int(tree_rate[2 * i + 1]) + rl_q16 * i32(ssd + 4 * chroma)
        rec[i]["depth"] = int(tree_cbf[2 * i + 1] != 0)
    return rec, tree


MADE_UNITS = 4      # random_units: 0 an uncoded 64x64 unit, 1 a 64x64 unit coded in chroma only, 2 one coded in every block, 3 a 32x32 tie (depth 1 stands)


def random_units(seed, n):
    """n units of 8x8 .. 64x64 with arbitrary outcomes, masks and rates, laid out as tree_rate_tools.random_trees lays them out (luma candidates per transform size,
    chroma candidates per chroma size, a candidate's luma cbf its mask bit); a 64x64 unit has depth-1 candidates only and -1 where a depth-0 candidate would be named.
    The first MADE_UNITS are made cases.  -> (units, zero_at, one_at, sizes, csizes, chroma_at, tree_rate, tree_cbf)"""
    from turingcodec_amd.decisions import RQT_CU_DT
    from turingcodec_amd.havoc import RQT_CHROMA_AT_DT
    rng = np.random.default_rng(seed)
    units = np.zeros(n, RQT_CU_DT)
    units["log2_size"] = rng.integers(3, 7, n)
    units["log2_size"][:MADE_UNITS] = [6, 6, 6, 5][:n]
    units["x0"], units["y0"] = 64 * (np.arange(n) % 8), 64 * (np.arange(n) // 8)
    count, ccount = {s: 0 for s in (2, 3, 4, 5)}, {s: 0 for s in (2, 3, 4)}
    zero_at, one_at, chroma_at = np.full(n, -1, np.int32), np.zeros(n, np.int32), np.zeros(n, RQT_CHROMA_AT_DT)
    for i, L in enumerate(int(v) for v in units["log2_size"]):
        one_at[i] = count[L - 1]
        count[L - 1] += 4
        a = chroma_at[i]
        if L < 6:
            zero_at[i] = count[L]
            count[L] += 1
            c = max(L - 1, 2)
            a["cb_zero"], a["cr_zero"] = ccount[c], ccount[c] + 1
            ccount[c] += 2
        else:
            a["cb_zero"], a["cr_zero"] = -1, -1
        if L > 3:
            a["cb_one"], a["cr_one"] = ccount[L - 2], ccount[L - 2] + 4
            ccount[L - 2] += 8
        else:
            a["cb_one"], a["cr_one"] = a["cb_zero"], a["cr_zero"]
    sizes = {s: dict(cbf=np.zeros(m, np.int32), ssd=rng.integers(0, 60000, m).astype(np.uint32)) for s, m in count.items()}
    csizes = {s: dict(cbf=np.zeros(m, np.int32), ssd=rng.integers(0, 20000, m).astype(np.uint32)) for s, m in ccount.items()}
    tree_rate = rng.integers(0, 1 << 27, 2 * n).astype(np.int64)
    tree_cbf = np.zeros(2 * n, np.uint32)
    for i, L in enumerate(int(v) for v in units["log2_size"]):
        nc = 4 if L > 3 else 1
        kind = rng.integers(0, 6)
        one = int(rng.integers(1, 16)) | int(rng.integers(0, 1 << nc)) << 4 | int(rng.integers(0, 1 << nc)) << 8
        if kind == 0:
            one = 0                                                      # uncoded
        elif kind == 1:
            one &= 0xff0                                                 # chroma only
            one |= 0 if one else 0x100
        tree_cbf[2 * i + 1] = one
        if L < 6:
            tree_cbf[2 * i] = int(rng.integers(0, 2)) | int(rng.integers(0, 2)) << 4 | int(rng.integers(0, 2)) << 8
        else:
            tree_cbf[2 * i], tree_rate[2 * i] = 0xdead, -12345          # entry 2 i of a 64x64 unit is nobody's: never read
    if n >= MADE_UNITS:
        tree_cbf[1], tree_rate[1] = 0, 0
        tree_cbf[3], tree_cbf[5] = 0x240, 0xfff
        j0, j1, a = int(zero_at[3]), int(one_at[3]), chroma_at[3]
        sizes[4]["ssd"][j1:j1 + 4], sizes[5]["ssd"][j0] = [10, 20, 30, 40], 100 - 4 * 7 + 4 * 36
        csizes[3]["ssd"][a["cb_one"]:a["cb_one"] + 4], csizes[3]["ssd"][a["cr_one"]:a["cr_one"] + 4] = [1, 2, 3, 4], [5, 6, 7, 8]
        csizes[4]["ssd"][[a["cb_zero"], a["cr_zero"]]] = [3, 4]
        tree_rate[6], tree_rate[7], tree_cbf[6], tree_cbf[7] = 5000, 5000, 0x111, 0x3
    for i, L in enumerate(int(v) for v in units["log2_size"]):      # a candidate's cbf = its mask bit
        a, nc = chroma_at[i], 4 if L > 3 else 1
        for k in range(4):
            sizes[L - 1]["cbf"][one_at[i] + k] = int(tree_cbf[2 * i + 1]) >> k & 1
        if L < 6:
            sizes[L]["cbf"][zero_at[i]] = int(tree_cbf[2 * i]) & 1
            c0 = csizes[max(L - 1, 2)]
            c0["cbf"][a["cb_zero"]], c0["cbf"][a["cr_zero"]] = int(tree_cbf[2 * i]) >> 4 & 1, int(tree_cbf[2 * i]) >> 8 & 1
        if L > 3:
            for k in range(4):
                csizes[L - 2]["cbf"][a["cb_one"] + k] = int(tree_cbf[2 * i + 1]) >> (4 + k) & 1
                csizes[L - 2]["cbf"][a["cr_one"] + k] = int(tree_cbf[2 * i + 1]) >> (8 + k) & 1
    return units, zero_at, one_at, sizes, csizes, chroma_at, tree_rate, tree_cbf


def made_units_hold(rec, tree):
    """units 0-3 of random_units"""
    assert rec["depth"][0] == 0 and rec["tried_zero"][0] == 0 and tree["mask_one"][0] == 0                                     # the uncoded 64x64 unit
    assert rec["depth"][1] == 1 and rec["tried_zero"][1] == 0 and tree["mask_one"][1] == 0x240 and not rec["one"]["cbf"][1].any()      # coded in chroma only
    assert rec["depth"][2] == 1 and rec["tried_zero"][2] == 0 and tree["mask_one"][2] == 0xfff
    for i in range(3):      # depth 0 of a 64x64 unit stays as an untried depth 0 is recorded
        assert rec["cost_zero"][i] == 0 and tree["mask_zero"][i] == 0 and tree["chroma_ssd_zero"][i] == 0 and rec["zero"]["ssd"][i] == 0 and rec["zero"]["cbf"][i] == 0
    assert rec["depth"][3] == 1 and rec["tried_zero"][3] == 1 and rec["cost_zero"][3] == rec["cost_one"][3]                    # a tie: depth 1 stands


def unit_client_rows(units, zero_at, one_at, sizes, csizes, chroma_at, tree_rate, tree_cbf):
    """the int64 [n, 14] rows tests/unit_decide_client.cpp takes: tree_rate_tools.client_rows' thirteen and the unit's log2 size; a 64x64 unit's depth-0 columns hold
    a value that would show if it were read"""
    rows = np.zeros((len(units), 14), np.int64)
    for i, u in enumerate(units):
        L = int(u["log2_size"])
        rows[i, 13] = L
        if L != L64:
            rows[i, :13] = TR.client_rows(units[i:i + 1], zero_at[i:i + 1], one_at[i:i + 1], sizes, csizes, chroma_at[i:i + 1], tree_rate[2 * i:2 * i + 2],
                                          tree_cbf[2 * i:2 * i + 2])[0]
            continue
        j1, a, c1 = int(one_at[i]), chroma_at[i], csizes[4]["ssd"]
        cb1, cr1 = int(c1[a["cb_one"]:a["cb_one"] + 4].astype(np.int64).sum()), int(c1[a["cr_one"]:a["cr_one"] + 4].astype(np.int64).sum())
        rows[i, :13] = [int(tree_cbf[2 * i + 1])] + [int(v) for v in sizes[5]["ssd"][j1:j1 + 4]] + [cb1, cr1, int(tree_rate[2 * i + 1]), 0xfff, 77777, 7777, 777, 1]
    return rows


class UnitDecisionClient:
    """tests/unit_decide_client.cpp: search/tu_decision.hpp's decideRqt with a tree rate, the chroma functor and the unit's own size, compiled at test time"""

    def __init__(self):
        import ctypes as C
        import os
        import subprocess
        import tempfile
        self._tmp = tempfile.TemporaryDirectory()
        so = os.path.join(self._tmp.name, "libunit_decide_client.so")
        subprocess.check_call(["g++", "-O1", "-std=c++14", "-fPIC", "-shared", "-Wall", "-o", so, os.path.join(TR.ROOT, "tests", "unit_decide_client.cpp")])
        self.L = C.CDLL(so)
        self.L.unit_decide.restype = C.c_int
        self.L.unit_decide.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_void_p]

    def decide(self, rows, rl_q16):
        """rows: int64 [n, 14] -> int64 [n, 6]: depth, tried_zero, cost_zero, cost_one, depth-0 luma blocks evaluated, depth-0 chroma asked for"""
        rows = np.ascontiguousarray(rows, np.int64)
        out = np.zeros((len(rows), 6), np.int64)
        assert self.L.unit_decide(rows.ctypes.data, len(rows), rl_q16, out.ctypes.data) == 0
        return out


# ---- havoc_mi355x_unit_pred_select in numpy ----------------------------------------------------------------------------------------------------------------
def select_case(seed, bit_depth, W=128, H=128):
    """units of all four sizes in four W x H luma planes (plane 6 - L for size 2^L) and four (Cb, Cr) plane pairs: blocks of different sizes overlap in picture
    position, never within a plane; best runs through 0, 1, 2, -1 at every size; the candidates' predictions are random samples, candidate 3 i + k of a size group at
    block (3 i + k) of that group, the groups one after the other in one luma and one chroma buffer (Cb blocks of a group, then its Cr blocks); the planes hold a
    sentinel -> dict(cand_y, cand_c, dst_y, dst_c, stride, cstride, first, best, rate, jobs, the planes wanted, unit_rate and unit_cand wanted)"""
    from turingcodec_amd.havoc import PRED_SELECT_JOB_DT
    rng = np.random.default_rng(seed)
    dt, top = (np.uint8, 256) if bit_depth == 8 else (np.uint16, 1 << bit_depth)
    sentinel = 0xA5 if bit_depth == 8 else 0x3A5
    place = []      # (L, x, y): every size covers the upper left 64x64 and more, so the planes overlap in picture position
    for L, step in ((6, 64), (5, 32), (4, 16), (3, 8)):
        n = 1 << L
        cells = [(x, y) for y in range(0, H, n) for x in range(0, W, n)]
        keep = cells[:4] if L == 6 else [c for k, c in enumerate(cells) if k % 3 != 2][:12]      # gaps: some places of a plane have no unit
        place += [(L, x, y) for x, y in keep]
    order = rng.permutation(len(place))
    place = [place[k] for k in order]
    n_units = len(place)
    group = {L: [k for k in range(n_units) if place[k][0] == L] for L in (6, 5, 4, 3)}
    best = np.zeros(n_units, np.int32)
    for L in (3, 4, 5, 6):      # -1, 0, 1, 2 at every size
        for i, k in enumerate(group[L]):
            best[k] = (i + L) % 4 - 1
        assert {int(best[k]) for k in group[L]} == {-1, 0, 1, 2}
    first = (3 * np.arange(n_units) + 5).astype(np.int32)
    rate = rng.integers(0, 1 << 40, 3 * n_units + 5).astype(np.int64)
    base_y, base_c, at_y, at_c = {}, {}, 0, 0
    for L in (6, 5, 4, 3):
        base_y[L], base_c[L] = at_y, at_c
        at_y += 3 * len(group[L]) << 2 * L
        at_c += 2 * (3 * len(group[L]) << 2 * (L - 1))
    cand_y, cand_c = rng.integers(0, top, at_y).astype(dt), rng.integers(0, top, at_c).astype(dt)
    stride, cstride = W, W // 2
    dst_y, dst_c = np.full(4 * W * H, sentinel, dt), np.full(4 * 2 * (W // 2) * (H // 2), sentinel, dt)
    want_y, want_c = dst_y.copy(), dst_c.copy()
    jobs = np.zeros(n_units, PRED_SELECT_JOB_DT)
    unit_rate, unit_cand = np.zeros(n_units, np.int64), np.zeros(n_units, np.int32)
    cpe = (W // 2) * (H // 2)
    for L in (6, 5, 4, 3):
        n, m = 1 << L, 1 << (L - 1)
        for i, k in enumerate(group[L]):
            _, x, y = place[k]
            j = jobs[k]
            j["log2_size"], j["unit"] = L, k
            j["cand_off"] = [base_y[L] + 3 * i * n * n, base_c[L] + 3 * i * m * m, base_c[L] + 3 * len(group[L]) * m * m + 3 * i * m * m]
            plane = 6 - L
            j["dst_off"] = [plane * W * H + y * W + x, 2 * plane * cpe + (y // 2) * cstride + x // 2, (2 * plane + 1) * cpe + (y // 2) * cstride + x // 2]
            b = int(best[k])
            unit_cand[k], unit_rate[k] = (first[k] + b, rate[first[k] + b]) if b >= 0 else (-1, -1)
            if b < 0:
                continue
            for c, (src, dst, s, size) in enumerate(((cand_y, want_y, stride, n), (cand_c, want_c, cstride, m), (cand_c, want_c, cstride, m))):
                block = src[int(j["cand_off"][c]) + b * size * size:int(j["cand_off"][c]) + (b + 1) * size * size].reshape(size, size)
                rows = int(j["dst_off"][c]) + np.arange(size)[:, None] * s + np.arange(size)
                assert (dst[rows] == sentinel).all()      # no two blocks of a plane overlap
                dst[rows] = block
    return dict(cand_y=cand_y, cand_c=cand_c, dst_y=dst_y, dst_c=dst_c, stride=stride, cstride=cstride, first=first, best=best, rate=rate, jobs=jobs,
                want_y=want_y, want_c=want_c, unit_rate=unit_rate, unit_cand=unit_cand, sentinel=sentinel, place=place)
