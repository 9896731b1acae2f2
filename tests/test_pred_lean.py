"""The inter prediction kernels (k_pred, k_pred_classes, k_subtract_bi of kernels_inter.hip) on every route they have, against the C restatement (the `oracle`
fixture), for equality.  The kernels have two forms in one binary: the lean one (a quad of columns per lane in the horizontal pass, no output tile, no filter at
a zero phase in the 32 / 64 classes, four samples per lane in SubtractBi) for widths that are multiples of four, and the earlier one for every other width and
under HAVOC_PRED_LEAN=0.  What a rewrite of exactly these kernels can break is pinned here:

  1. every route: uni / bi x 8 / 4 taps x bit depths 8, 9, 10, every block of {4, 8, 16, 32, 64}^2 (all four size classes, non-square blocks, heights that are
     no multiple of 8) plus widths 2, 6, 10, 12 (the earlier form beside the lean one in one launch) x every phase pair (uni) / every zero / non-zero kind (bi);
  2. ragged tables: job counts around the workgroup boundaries of every class (32 / 8 / 2 / 1 jobs per workgroup), through the one-launch and the per-class entry points;
  3. exactly the block: a sentinel-filled destination with slots wider and taller than the block;
  4. unaligned destinations (dst_off = 1, 2, 3 mod 4) and reference windows at the first / last rows and columns the plane allows;
  5. extremes: reference planes of 0, of the maximum, and a checkerboard of both; SubtractBi pairs that clip at both ends;
  6. both arms: the same cases under HAVOC_PRED_LEAN=0 in an interpreter of its own (the switch is read once per process).

Shapes are the smallest that take each path; every case runs in a few seconds."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = cases.PLANE_W
SIDES = (4, 8, 16, 32, 64)
BLOCKS = [(w, h) for w in SIDES for h in SIDES] + [(2, 8), (6, 8), (10, 16), (12, 16), (2, 4), (6, 4), (10, 8), (12, 12), (24, 32), (48, 64), (16, 12), (32, 24)]
ROUTES = [(bi, taps, bd) for bi in (False, True) for taps in (8, 4) for bd in (8, 9, 10)]
COUNTS = [1, 2, 7, 8, 9, 31, 33]


def dtype_of(bd):
    return np.uint8 if bd == 8 else np.uint16


def sentinel(bd):
    return 0xA5 if bd == 8 else 0xA5A5


def plane(rng, bd, kind="uniform"):
    mx = (1 << bd) - 1
    if kind == "uniform":
        a = rng.integers(0, mx + 1, size=(H, W))
    elif kind == "zero":
        a = np.zeros((H, W), np.int64)
    elif kind == "max":
        a = np.full((H, W), mx)
    elif kind == "checker":
        a = ((np.add.outer(np.arange(H), np.arange(W)) & 1) * mx)
    elif kind == "checker_inv":
        a = (((np.add.outer(np.arange(H), np.arange(W)) + 1) & 1) * mx)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a.astype(dtype_of(bd))).ravel()


def phases(taps):
    n = 4 if taps == 8 else 8
    return [(xf, yf) for yf in range(n) for xf in range(n)]


def bi_kinds(taps, k0=0):
    """the 16 kinds of (xFrac0, yFrac0, xFrac1, yFrac1): zero or not, per phase and reference; the non-zero values rotate through all of them"""
    n = 4 if taps == 8 else 8
    out = []
    k = k0
    for kind in range(16):
        fr = []
        for b in range(4):
            if kind >> b & 1:
                fr.append(1 + k % (n - 1))
                k += 1
            else:
                fr.append(0)
        out.append(tuple(fr))
    return out


def uni_job(dst, ref, w, h, xf, yf):
    return (dst, ref, w, h, xf, yf, 0, 0)


def bi_job(dst, r0, r1, w, h, fr):
    return (dst, r0, r1, w, h, fr[0], fr[1], fr[2], fr[3], 0, 0, 0)


def table(rng, bi, taps, blocks, all_phases, slot, dst0=0, k0=0):
    """one job per block and phase pair (uni) / kind (bi), at random reference positions, job i writing to dst0 + i * slot"""
    jobs = []
    for (w, h) in blocks:
        for k, ph in enumerate(bi_kinds(taps, k0 + len(jobs)) if bi else (phases(taps) if all_phases else [phases(taps)[i] for i in (0, 1, 4 if taps == 8 else 8, 6 if taps == 8 else 27)])):
            o = dst0 + len(jobs) * slot
            if bi:
                jobs.append(bi_job(o, cases.off(*cases.rand_pos(rng, w, h)), cases.off(*cases.rand_pos(rng, w, h)), w, h, ph))
            else:
                jobs.append(uni_job(o, cases.off(*cases.rand_pos(rng, w, h)), w, h, *ph))
    return np.array(jobs, np.int32)


def expected_pred(oracle, bi, taps, bd, ref, sr, jobs, dst_len, sd, fill):
    exp = np.full(dst_len, fill, ref.dtype)
    for j in jobs.tolist():
        if bi:
            oracle.pred_bi(exp, j[0], sd, ref, j[1], j[2], sr, j[3], j[4], j[5], j[6], j[7], j[8], bd, taps)
        else:
            oracle.pred_uni(exp, j[0], sd, ref, j[1], sr, j[2], j[3], j[4], j[5], bd, taps)
    return exp


def run_pred(hv, bi, taps, bd, ref, sr, jobs, dst_len, sd, fill, how):
    """how = "classes": the class-sorted table in one launch (what the step does); "per_class": one launch per size class"""
    dst = hv.up(np.full(dst_len, fill, ref.dtype))
    d_ref = hv.up(ref)
    w, h = (jobs[:, 3], jobs[:, 4]) if bi else (jobs[:, 2], jobs[:, 3])
    if how == "classes":
        js, counts, _ = hv.sort_by_class(jobs, w, h)
        hv.pred_classes_d(bi, taps, bd, dst, sd, d_ref, sr, hv.up(js), counts)
    else:
        for idx, mw, mh in hv.size_classes(w, h):
            (hv.pred_bi_d if bi else hv.pred_uni_d)(taps, bd, dst, sd, d_ref, sr, hv.up(np.ascontiguousarray(jobs[idx])), mw, mh)
    return hv.down(dst, ref.dtype)


def compare(got, exp, jobs, what):
    if not np.array_equal(got, exp):
        bad = np.flatnonzero(got != exp)
        starts = jobs[:, 0]
        i = int(np.searchsorted(np.sort(starts), bad[0], side="right")) - 1
        raise AssertionError(f"{what}: {len(bad)} samples differ, first at {int(bad[0])} (got {int(got[bad[0]])}, want {int(exp[bad[0]])}), near job {jobs[np.argsort(starts)[max(i, 0)]].tolist()}")


# ---- 1. every route --------------------------------------------------------------------------------------------------------------------------------------

def check_every_route(hv, oracle, bi, taps, bd):
    rng = np.random.default_rng(1000 + 100 * bi + 10 * taps + bd)
    ref = plane(rng, bd)
    slot = 64 * 64
    jobs = table(rng, bi, taps, BLOCKS, True, slot)
    n = len(jobs) * slot
    exp = expected_pred(oracle, bi, taps, bd, ref, W, jobs, n, 64, 0)
    for how in ("classes", "per_class"):
        compare(run_pred(hv, bi, taps, bd, ref, W, jobs, n, 64, 0, how), exp, jobs, f"{how} bi={bi} taps={taps} bd={bd}")


@pytest.mark.parametrize("bi,taps,bd", ROUTES)
def test_every_route(hv, oracle, bi, taps, bd):
    check_every_route(hv, oracle, bi, taps, bd)


# ---- 2. ragged tables ------------------------------------------------------------------------------------------------------------------------------------

def check_ragged(hv, oracle, count):
    """`count` jobs of ONE class per launch (the last workgroup is partly empty: 32 / 8 / 2 / 1 jobs per workgroup), then `count` jobs of every class in one table"""
    rng = np.random.default_rng(2000 + count)
    slot = 64 * 64
    for bi in (False, True):
        for taps, bd in ((8, 8), (4, 8), (8, 10), (4, 9)):
            ref = plane(rng, bd)
            tables = []
            for cs in (8, 16, 32, 64):
                shapes = [(cs, cs), (cs, cs // 2), (cs // 2, cs), (cs, cs // 2 + 4 if cs > 8 else 4)]
                per = 16 if bi else 4       # jobs that table() makes per block: take one of them, another kind / phase pair for every block
                tables.append(table(rng, bi, taps, [shapes[i % 4] for i in range(count)], False, slot)[[i * per + (3 * i + count) % per for i in range(count)]])
            for t in tables + [np.concatenate(tables)]:
                t = t.copy()
                t[:, 0] = np.arange(len(t)) * slot
                n = len(t) * slot
                exp = expected_pred(oracle, bi, taps, bd, ref, W, t, n, 64, 0)
                for how in ("classes", "per_class"):
                    compare(run_pred(hv, bi, taps, bd, ref, W, t, n, 64, 0, how), exp, t, f"ragged {count} {how} bi={bi} taps={taps} bd={bd}")


@pytest.mark.parametrize("count", COUNTS)
def test_ragged_tables(hv, oracle, count):
    check_ragged(hv, oracle, count)


# ---- 3. exactly the block --------------------------------------------------------------------------------------------------------------------------------

SD, SROWS = 80, 72      # slots wider and taller than any block


def touched_mask(n, jobs, wcol, sd):
    m = np.zeros(n, bool)
    for j in jobs.tolist():
        for r in range(j[wcol + 1]):
            m[j[0] + r * sd:j[0] + r * sd + j[wcol]] = True
    return m


def check_exact_block(hv, oracle, bi, taps, bd):
    rng = np.random.default_rng(3000 + 100 * bi + 10 * taps + bd)
    ref = plane(rng, bd)
    slot = SD * SROWS
    jobs = table(rng, bi, taps, BLOCKS, False, slot, dst0=3 * SD + 5)
    n = len(jobs) * slot
    fill = sentinel(bd)
    exp = expected_pred(oracle, bi, taps, bd, ref, W, jobs, n, SD, fill)
    m = touched_mask(n, jobs, 3 if bi else 2, SD)
    assert (exp[~m] == fill).all()
    for how in ("classes", "per_class"):
        got = run_pred(hv, bi, taps, bd, ref, W, jobs, n, SD, fill, how)
        assert (got[~m] == fill).all(), f"{how}: {int((got[~m] != fill).sum())} samples outside the blocks were written"
        compare(got, exp, jobs, f"exact {how} bi={bi} taps={taps} bd={bd}")


@pytest.mark.parametrize("bi,taps,bd", [(bi, taps, bd) for bi in (False, True) for taps in (8, 4) for bd in (8, 10)])
def test_prediction_writes_exactly_the_block(hv, oracle, bi, taps, bd):
    check_exact_block(hv, oracle, bi, taps, bd)


def subtract_jobs(rng, blocks, slot, sd, dst0=0, align=None):
    jobs = []
    for i, (w, h) in enumerate(blocks):
        p, s = cases.off(*cases.rand_pos(rng, w, h)), cases.off(*cases.rand_pos(rng, w, h))
        if align is not None:
            p, s = p - p % 4 + align[1], s - s % 4 + align[2]
        jobs.append((dst0 + i * slot + (align[0] if align is not None else 0), p, s, w, h, 0, 0, 0))
    return np.array(jobs, np.int32)


def check_subtract(hv, oracle, bd, jobs, pred, src, n, sd, what):
    fill = sentinel(bd)
    exp = np.full(n, fill, src.dtype)
    for j in jobs.tolist():
        oracle.subtract_bi(exp, j[0], sd, pred, j[1], W, src, j[2], W, j[3], j[4], bd)
    m = touched_mask(n, jobs, 3, sd)
    dst = hv.up(np.full(n, fill, src.dtype))
    hv.subtract_bi_d(bd, dst, sd, hv.up(pred), W, hv.up(src), W, hv.up(jobs))
    got = hv.down(dst, src.dtype)
    assert (got[~m] == fill).all(), f"{what}: {int((got[~m] != fill).sum())} samples outside the blocks were written"
    compare(got, exp, jobs, what)


def check_subtract_bi(hv, oracle, bd):
    """every block, every alignment of destination, prediction and source against the 4-sample accesses, ragged tables (4 jobs per workgroup), sentinel-filled slots"""
    rng = np.random.default_rng(3500 + bd)
    pred, src = plane(rng, bd), plane(rng, bd)
    slot = SD * SROWS
    jobs = subtract_jobs(rng, BLOCKS, slot, SD, dst0=3 * SD + 5)
    check_subtract(hv, oracle, bd, jobs, pred, src, len(jobs) * slot, SD, f"subtract_bi bd={bd}")
    for a in range(1, 64):
        align = (a & 3, a >> 2 & 3, a >> 4 & 3)
        blocks = [BLOCKS[(a + 7 * i) % len(BLOCKS)] for i in range(3)]
        jobs = subtract_jobs(rng, blocks, slot, SD + (a % 3), dst0=3 * SD + 8, align=align)
        check_subtract(hv, oracle, bd, jobs, pred, src, len(jobs) * slot + 8 * SD, SD + (a % 3), f"subtract_bi bd={bd} align={align}")
    for count in (1, 2, 3, 4, 5, 7, 9):
        jobs = subtract_jobs(rng, [BLOCKS[(3 * i + count) % len(BLOCKS)] for i in range(count)], slot, SD, dst0=SD + 1)
        check_subtract(hv, oracle, bd, jobs, pred, src, len(jobs) * slot, SD, f"subtract_bi bd={bd} count={count}")


@pytest.mark.parametrize("bd", [8, 9, 10])
def test_subtract_bi_writes_exactly_the_block(hv, oracle, bd):
    check_subtract_bi(hv, oracle, bd)


# ---- 4. unaligned destinations, reference windows at the plane's edges -----------------------------------------------------------------------------------

def corner_offsets(taps, w, h):
    """reference block origins whose filter window (rows -AB .. h + TAPS - 2 - AB, the dwords of the horizontal filter's quads) touches the first / last row and column"""
    ab = taps // 2 - 1
    wq = (w + 3) & ~3
    x1, y1 = W - wq - (5 if taps == 8 else 3), H - h - (taps - 1 - ab)
    return [cases.off(ab, ab), cases.off(x1, ab), cases.off(ab, y1), cases.off(x1, y1)]


def check_unaligned(hv, oracle, bi, taps, bd):
    rng = np.random.default_rng(4000 + 100 * bi + 10 * taps + bd)
    ref = plane(rng, bd)
    sd = 67                                         # odd: the alignment of a row's first sample changes from row to row too
    slot = sd * SROWS
    blocks = [(4, 4), (8, 8), (8, 4), (16, 16), (12, 16), (16, 4), (32, 32), (32, 8), (64, 64), (64, 16), (24, 32), (6, 8)]
    jobs = []
    for a in (1, 2, 3):
        for c in range(4):
            for bidx, (w, h) in enumerate(blocks):
                o = len(jobs) * slot + 4 * sd + 4 + a          # = a mod 4
                co = corner_offsets(taps, w, h)
                if bi:
                    jobs.append(bi_job(o, co[c], co[(c + 1 + bidx) % 4], w, h, bi_kinds(taps, len(jobs))[(5 * c + 3 * bidx + a) % 16]))
                else:
                    jobs.append(uni_job(o, co[c], w, h, *phases(taps)[(5 * len(jobs) + c) % len(phases(taps))]))
    jobs = np.array(jobs, np.int32)
    n = len(jobs) * slot
    fill = sentinel(bd)
    exp = expected_pred(oracle, bi, taps, bd, ref, W, jobs, n, sd, fill)
    for how in ("classes", "per_class"):
        compare(run_pred(hv, bi, taps, bd, ref, W, jobs, n, sd, fill, how), exp, jobs, f"unaligned {how} bi={bi} taps={taps} bd={bd}")


@pytest.mark.parametrize("bi,taps,bd", [(bi, taps, bd) for bi in (False, True) for taps in (8, 4) for bd in (8, 10)])
def test_unaligned_destinations_and_edge_windows(hv, oracle, bi, taps, bd):
    check_unaligned(hv, oracle, bi, taps, bd)


# ---- 5. extremes -----------------------------------------------------------------------------------------------------------------------------------------

def check_extremes(hv, oracle, bd):
    rng = np.random.default_rng(5000 + bd)
    slot = 64 * 64
    blocks = [(8, 8), (16, 16), (32, 32), (64, 64), (32, 16), (4, 8), (16, 64), (6, 8)]
    for kind in ("zero", "max", "checker"):
        ref = plane(rng, bd, kind)
        for bi in (False, True):
            for taps in (8, 4):
                jobs = table(rng, bi, taps, blocks, True, slot)
                n = len(jobs) * slot
                exp = expected_pred(oracle, bi, taps, bd, ref, W, jobs, n, 64, 0)
                compare(run_pred(hv, bi, taps, bd, ref, W, jobs, n, 64, 0, "classes"), exp, jobs, f"extremes {kind} bi={bi} taps={taps} bd={bd}")
    # SubtractBi: 2 * src - pred below 0 (src 0, pred max), above the maximum (src max, pred 0), and both in one block (opposite checkerboards)
    planes = {k: plane(rng, bd, k) for k in ("zero", "max", "checker", "checker_inv")}
    for ks, kp in (("zero", "max"), ("max", "zero"), ("checker", "checker_inv"), ("max", "max"), ("zero", "zero")):
        jobs = subtract_jobs(rng, BLOCKS, SD * SROWS, SD, dst0=SD + 2)
        check_subtract(hv, oracle, bd, jobs, planes[kp], planes[ks], len(jobs) * SD * SROWS, SD, f"subtract_bi extremes src={ks} pred={kp} bd={bd}")


@pytest.mark.parametrize("bd", [8, 9, 10])
def test_extremes(hv, oracle, bd):
    check_extremes(hv, oracle, bd)


# ---- 6. both arms ----------------------------------------------------------------------------------------------------------------------------------------

def run_everything(hv, oracle):
    for bi, taps, bd in ROUTES:
        check_every_route(hv, oracle, bi, taps, bd)
    for count in COUNTS:
        check_ragged(hv, oracle, count)
    for bi in (False, True):
        for taps in (8, 4):
            for bd in (8, 10):
                check_exact_block(hv, oracle, bi, taps, bd)
                check_unaligned(hv, oracle, bi, taps, bd)
    for bd in (8, 9, 10):
        check_subtract_bi(hv, oracle, bd)
        check_extremes(hv, oracle, bd)


_ARM_SCRIPT = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import reflibs, test_pred_lean
from turingcodec_amd import Havoc
test_pred_lean.run_everything(Havoc(0), reflibs.Oracle())
print("ok")
"""


def test_the_earlier_arm_matches_the_oracle_too():
    """HAVOC_PRED_LEAN=0 keeps every job on the earlier form of the kernels; unset (the tests above) takes the lean one where the width allows.  The switch is read
    once per process, so the other arm runs every case above in an interpreter of its own"""
    out = subprocess.run([sys.executable, "-c", _ARM_SCRIPT, ROOT], capture_output=True, text=True, timeout=900, env=dict(os.environ, HAVOC_PRED_LEAN="0"))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-3000:]


@pytest.fixture(scope="module")
def hv():
    from turingcodec_amd import Havoc
    return Havoc(0)
