"""The temporal candidate in the picture search's predictors (havoc_mi355x_search_temporal; picture_order.hpp: derivePredictors / walkPictureSequential with a table).
Test infrastructure: builds tests/search_temporal_client.cpp for the `oracle` and `ref` back ends, makes the pictures and the synthetic candidate tables, runs the
walk with a table through ctypes and the device search through the C ABI.

    tests/_build/libsearch_temporal_oracle.so   the walk over the CPU oracle
    tests/_build/libsearch_temporal_ref.so      the walk over the reference's tables (where oracle/_ref is built)
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import search_tools as st

ROOT = st.ROOT
SRC = os.path.join(ROOT, "tests", "search_temporal_client.cpp")
CAND_DT = np.dtype([("mv", "<i2", (2,)), ("available", "<i2"), ("source", "<i2")])      # havoc_mi355x_temporal_cand
assert CAND_DT.itemsize == 8
SENTINEL = 0xA5
PICTURES = {"136x72": (136, 72), "416x240": (416, 240)}      # 3 x 2 and 7 x 4 CTUs: the last CTU row and column are partial
PAD = 96


def build(kind):
    """the library path, or None where the back end's own library is not there"""
    os.makedirs(st.BUILD, exist_ok=True)
    out = os.path.join(st.BUILD, f"libsearch_temporal_{kind}.so")
    deps = [SRC, st.SRC] + [os.path.join(ROOT, "turingcodec_amd", "search", f) for f in ("decision.hpp", "table_view.hpp", "search_abi.h", "picture_order.hpp", "amvp.hpp",
                                                                                         "cand_mode_list.hpp", "tu_decision.hpp")] + [os.path.join(ROOT, "tests", "merge.hpp")]
    base = ["g++", "-O2", "-std=c++14", "-fPIC", "-shared", "-Wall"] + st.INC + [SRC, "-o", out]
    if kind == "ref":
        lib = os.path.join(ROOT, "oracle", "_ref", "libhavoc_ref.so")
        if not os.path.exists(lib):
            return out if os.path.exists(out) else None
        if not st._newer(out, lib, *deps):
            subprocess.check_call(base + ["-L" + os.path.dirname(lib), "-lhavoc_ref", "-Wl,-rpath,$ORIGIN/../../oracle/_ref"])
    elif kind == "oracle":
        lib = os.path.join(ROOT, "oracle", "liboracle.so")
        if not st._newer(out, lib, *deps):
            subprocess.check_call(base + ["-DSEARCH_ORACLE", "-L" + os.path.dirname(lib), "-loracle", "-Wl,-rpath,$ORIGIN/../../oracle"])
    else:
        raise ValueError(kind)
    return out


def have_ref():
    return build("ref") is not None


class Client:
    """walkPictureSequential with a table of temporal candidates, one table call at a time"""

    def __init__(self, kind="oracle", mask=3):
        path = build(kind)
        if path is None:
            raise FileNotFoundError(kind)
        L = self.L = C.CDLL(path)
        vp, ip, i = C.c_void_p, C.c_ssize_t, C.c_int
        L.client_open.argtypes = [i]
        L.client_picture_uni_temporal.argtypes = [i, vp, ip, vp, vp, ip, C.POINTER(st.Params), vp, vp, i, i, vp, vp, vp, vp, vp, vp]
        assert L.client_open(mask) == 0

    def walk(self, case, cands, report=False):
        """(results [2 n], field, refinements [2 n]) and, with report, int32 [n, 2, 10] (search_temporal_client.cpp); cands: CAND_DT [n, 2] or None"""
        n = len(case["pus"])
        par = case["params"]
        out, out_bi = np.zeros(2 * n, st.RESULT_DT), np.zeros(2 * n, st.RESULT_DT)
        field = np.zeros((2, (par.pic_height + 3) // 4, (par.pic_width + 3) // 4, 2), np.int16)
        rep = np.zeros((n, 2, 10), np.int32) if report else None
        rate = np.asarray(case["mvp_rate"], np.int64)
        if cands is not None:
            cands = np.ascontiguousarray(cands, CAND_DT)
            assert cands.shape == (n, 2)
        origin = lambda p: p.ctypes.data + (PAD * case["stride"] + PAD) * p.itemsize
        src, r0, r1 = case["planes"]
        rc = self.L.client_picture_uni_temporal(src.itemsize, origin(src), case["stride"], origin(r0), origin(r1), case["stride"], C.byref(par), case["pus"].ctypes.data,
                                                case["ctu_first"].ctypes.data, case["cx"], case["cy"], rate.ctypes.data, out.ctypes.data, field.ctypes.data,
                                                out_bi.ctypes.data, cands.ctypes.data if cands is not None else None, rep.ctypes.data if report else None)
        assert rc == 0
        return (out, field, out_bi, rep) if report else (out, field, out_bi)


@functools.lru_cache(maxsize=None)
def make_case(name, bit_depth):
    """the picture of DecisionPicture(seed=5): planes, units in decision order, parameters"""
    from turingcodec_amd.decisions import decision_inputs
    W, H = PICTURES[name]
    d = decision_inputs(W, H, bit_depth, 32, 5)
    return dict(W=W, H=H, bd=bit_depth, planes=d["planes"], stride=d["stride"], pus=np.ascontiguousarray(d["pus"]), ctu_first=np.ascontiguousarray(d["ctu_first"], np.int32),
                cx=d["cx"], cy=d["cy"], params=d["params"], mvp_rate=d["mvp_rate"])


SEED = 3


def make_table(case, seed=SEED):
    """a synthetic table: about three quarters of the records available, vectors within +-40 quarter samples; and on a few units at each of the four picture edges
    records whose components are the int16 extremes or lie one full sample beyond what LimitFullPelMv allows the unit (decision.hpp:143-166)"""
    rng = np.random.default_rng(seed)
    pus, W, H = case["pus"], case["W"], case["H"]
    n = len(pus)
    t = np.zeros((n, 2), CAND_DT)
    t["available"] = rng.random((n, 2)) < 0.75
    t["mv"] = rng.integers(-40, 41, (n, 2, 2))
    t["mv"][t["available"] == 0] = 0
    t["source"] = np.where(t["available"] != 0, rng.integers(1, 3, (n, 2)), 0)
    edges = {"left": np.flatnonzero(pus["x0"] == 0), "top": np.flatnonzero(pus["y0"] == 0), "right": np.flatnonzero(pus["x0"] + pus["w"] == W),
             "bottom": np.flatnonzero(pus["y0"] + pus["h"] == H)}
    extreme = []
    for k, (edge, idx) in enumerate(sorted(edges.items())):
        assert len(idx) >= 1, edge
        for j, p in enumerate(idx[[0, len(idx) // 2, -1]]):      # (a small picture may name a unit twice: the later record stands)
            q = pus[p]
            lo = (-64 - q["x0"], -64 - q["y0"])
            hi = (W + 64 - q["x0"] - q["w"], H + 64 - q["y0"] - q["h"])
            choices = [(32767, -32768), (-32768, 32767), (-32767, 32767), (4 * (hi[0] + 1), 4 * (lo[1] - 1)), (4 * (lo[0] - 1), 4 * (hi[1] + 1)), (32767, 32767)]
            for l in (0, 1):
                t[p, l] = (choices[(2 * k + j + 3 * l) % len(choices)], 1, 2)
            extreme.append(int(p))
    return t, sorted(set(extreme))


def unavailable_table(case):
    return np.zeros((len(case["pus"]), 2), CAND_DT)


# ---- the device search through the C ABI (no DecisionPicture: the planes, the units and every destination are this module's) -------------------------------------
class DevicePicture:
    def __init__(self, hv, case):
        self.hv, self.case = hv, case
        S = self.S = 1 if case["bd"] == 8 else 2
        dt = np.uint8 if S == 1 else np.uint16
        n = case["planes"][0].size
        pe = self.pe = (n + 63) & ~63
        pic = np.zeros(3 * pe, dt)
        for k, p in enumerate(case["planes"]):
            pic[k * pe:k * pe + n] = p
        self.d_pic, self.d_phase = hv.up(pic), hv.zeros(32 * pe, dt)
        W, H, stride = case["W"], case["H"], case["stride"]
        for r in (0, 1):
            ph, ref = self.d_phase[r * 16 * pe:(r + 1) * 16 * pe], self.d_pic[(1 + r) * pe:(2 + r) * pe]
            with hv.torch.cuda.stream(hv.tstream):
                ph[:pe] = ref
            hv.interp_planes_d(case["bd"], ph, pe, ref, stride, 12, 4, W + 2 * PAD - 24, H + 2 * PAD - 8)
        self.d_pus = hv.up(case["pus"].view(np.uint8).reshape(-1))
        self.d_first = hv.up(case["ctu_first"])
        self.n = len(case["pus"])
        self.cells = ((W + 3) // 4) * ((H + 3) // 4)
        self.work_bytes = int(hv.L.havoc_mi355x_search_workspace(W, H))

    def search(self, step_launches, bi, n_pus=None):
        """one havoc_mi355x_search_picture_uni over sentinel-filled destinations: (rc, results, field, refinements or None, the last word of the workspace)"""
        hv, c, pe = self.hv, self.case, self.pe
        fill = lambda nbytes: hv.up(np.full(nbytes, SENTINEL, np.uint8))
        d_out, d_bi = fill(2 * self.n * 56), fill(2 * self.n * 56) if bi else None
        d_field, d_work = fill(2 * self.cells * 4), fill((self.work_bytes + 15) & ~15)
        o = PAD * c["stride"] + PAD
        i64 = lambda a, b: (C.c_int64 * 2)(int(a), int(b))
        base, ph = self.d_pic.data_ptr(), self.d_phase.data_ptr()
        rc = hv.L.havoc_mi355x_search_picture_uni(hv.h, self.S, C.byref(c["params"]), i64(*c["mvp_rate"]), base, o, c["stride"], base, i64(pe + o, 2 * pe + o), c["stride"], ph,
                                                  pe, i64(o, 16 * pe + o), self.d_pus.data_ptr(), self.d_first.data_ptr(), c["cx"], c["cy"],
                                                  self.n if n_pus is None else n_pus, d_out.data_ptr(), d_bi.data_ptr() if bi else None, d_field.data_ptr(),
                                                  d_work.data_ptr(), step_launches)
        hv.sync()
        if rc != 0:
            return rc, None, None, None, None
        res = hv.down(d_out, np.uint8).view(st.RESULT_DT)
        field = hv.down(d_field, np.uint8).view(np.int16).reshape(2, (c["H"] + 3) // 4, (c["W"] + 3) // 4, 2)
        gave_up = int(hv.down(d_work, np.uint8)[:self.work_bytes].view(np.int32)[-1])
        return rc, res, field, hv.down(d_bi, np.uint8).view(st.RESULT_DT) if bi else None, gave_up


def same_records(a, b, skip=("replays",)):
    return all(np.array_equal(a[k], b[k]) for k in a.dtype.names if k not in skip)
