"""The fused transform-unit chain (csrc/kernels_tu_fused.hip: k_tu_forward and its SCAN form, k_tu_forward_mfma32, k_tu_reconstruct) pinned at every edge, QP
and scan threshold.  Every expected value is the oracle's -- `transform`, `quantize_inverse`, `inverse_transform_add`, `ssd`, `rdoq`, composed as
suite.LoopImpl.tu_forward / tu_reconstruct compose them -- and everything is bit exact.  Generators and numpy restatements: tests/tu_chain_tools.py.

  part 1  forward       every (size, transform type) x bit depth 8 / 9 / 10: impulses, basis-matched blocks, constant and extreme residuals, ragged job counts,
                        block offsets, strides, the coefficient buffer's footprint; the 32x32 8-bit cases again with the matrix-core kernel switched off
  part 2  reconstruct   every de-quantiser, every clip (the CPU test says which each route reaches), impulse levels, sparse blocks, SSD extremes, in place,
                        footprint, ragged job counts
  part 3  scan          tu_forward_scan + rdoq_prescanned: coefficients, the zeroed level blocks, the RdoqInfo records (inputs that land ON the three
                        thresholds of rdoqThresholds: the CPU test counts them), levels and flags against havoc_mi355x_rdoq and the oracle; argument errors

The device buffers are sentinel-filled and compared WHOLE with what the oracle leaves in the same buffers, so every comparison is also a footprint check.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cases
import tu_chain_tools as tc

W, H = cases.PLANE_W, cases.PLANE_H
ROUTE_IDS = [tc.route_id(r) for r in tc.ROUTES]
SCAN_CASES = [(8, 4), (8, 5), (10, 4), (10, 5)]
SCAN_IDS = [f"n{1 << log2}dct-{bd}bit" for bd, log2 in SCAN_CASES]
gpu = pytest.mark.gpu
routes = pytest.mark.parametrize("route", tc.ROUTES, ids=ROUTE_IDS)
scans = pytest.mark.parametrize("bd,log2", SCAN_CASES, ids=SCAN_IDS)


@pytest.fixture(scope="module")
def hv():
    from turingcodec_amd import Havoc
    return Havoc(0)


def same(got, want, what):
    bad = np.flatnonzero(np.asarray(got).ravel() != np.asarray(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {np.asarray(want).size} differ, first at {bad[:8].tolist()}: got {np.asarray(got).ravel()[bad[:8]].tolist()}, " \
                          f"want {np.asarray(want).ravel()[bad[:8]].tolist()}"


# ================================================================================================================== CPU: the restatements and the coverage
@routes
def test_numpy_restatement_equals_the_oracle(oracle, route):
    """the numpy transforms of tu_chain_tools (which say what a case reaches) give the oracle's coefficients and reconstructions, on random and on clipping blocks"""
    log2, tr, bd = route
    n, mx = 1 << log2, (1 << bd) - 1
    rng = np.random.default_rng(1)
    res = np.concatenate([rng.integers(-mx, mx + 1, (6, n, n)), tc.extreme_residuals(n, mx, 2)])
    got, _ = tc.np_forward(res, log2, tr, bd)
    for i in range(len(res)):
        co = np.zeros(n * n, np.int16)
        oracle.transform(co, 0, np.ascontiguousarray(res[i], np.int16).ravel(), 0, n, log2, tr, bd)
        same(got[i], co, f"forward block {i}")
    levels, pred, launches = tc.clip_cases(log2, tr, bd)
    dt = cases.sample_dtype(tc.S_of(bd))
    for qp, lo, hi in launches:
        scale, shift = cases.dequant_params(qp, log2, bd)
        for i in range(lo, hi, 3):
            dq, rec = np.zeros(n * n, np.int16), np.zeros(n * n, dt)
            oracle.quantize_inverse(dq, 0, np.ascontiguousarray(levels[i]).ravel(), 0, scale, shift, n * n)
            oracle.inverse_transform_add(rec, 0, n, np.ascontiguousarray(pred[i].astype(dt)).ravel(), 0, n, dq, 0, log2, tr, bd)
            same(tc.np_reconstruct(levels[i], qp, log2, tr, bd, pred[i])[0], rec, f"reconstruction of clip case {i} at qp {qp}")


# routes on which NO level block reaches the clip of the second inverse pass (the residual clip): its input is a clipped int16 and its shift 20 - bitDepth, so
# |residual| <= (32768 A + half) >> (20 - bitDepth) with A the largest column sum of |M| -- below 32768 everywhere but at 32x32, 10-bit (tc.clip_is_reachable)
RESIDUAL_CLIP_OUT_OF_REACH = [r for r in ROUTE_IDS if r != "n32dct-10bit"]


def test_every_clip_is_reached_from_both_sides():
    """the clip cases of part 2 reach the de-quantiser clip, the first-pass clip (o >> 7), the residual clip and the sample clip at 0 and at max, each from both
    sides, on every route where the arithmetic allows it; where it does not, the route is listed above and the bound that forbids it is checked here"""
    out_of_reach = []
    for route in tc.ROUTES:
        log2, tr, bd = route
        seen = tc.clip_coverage(log2, tr, bd)
        for clip in tc.CLIPS:
            if tc.clip_is_reachable(clip, log2, tr, bd):
                for side in (-1, 1):
                    assert (clip, side) in seen, (tc.route_id(route), clip, side)
            else:
                assert clip == "residual" and (clip, -1) not in seen and (clip, 1) not in seen, (tc.route_id(route), clip)
                out_of_reach.append(tc.route_id(route))
    assert out_of_reach == RESIDUAL_CLIP_OUT_OF_REACH


def test_basis_matched_blocks_reach_the_largest_coefficients(oracle):
    """8-bit 16x16 and 32x32: 32640 at DC, 26462 at the checkerboard, and a first pass that peaks below 2^15 (neither pass overflows)"""
    for log2 in (4, 5):
        n = 1 << log2
        res, kl = tc.basis_matched_residuals(log2, 0, 255)
        for (k, l), want in (((0, 0), 32640), ((n - 1, n - 1), 26462)):
            co = np.zeros(n * n, np.int16)
            oracle.transform(co, 0, np.ascontiguousarray(res[kl.index((k, l))], np.int16).ravel(), 0, n, log2, 0, 8)
            assert int(co[k * n + l]) == want == int(np.abs(co.astype(np.int64)).max()), (log2, k, l, int(co[k * n + l]))
        assert 29000 < tc.np_forward(res, log2, 0, 8)[1] < 32768


@scans
def test_scan_inputs_land_on_every_threshold(oracle, bd, log2):
    """at least SCAN_TARGET 4x4 groups of the scan tests' blocks have a largest |coefficient| of exactly thr[m] - 1, and as many of exactly thr[m], for each of the
    three thresholds -- counted here from the oracle's coefficients alone"""
    case = tc.scan_case(oracle, bd, log2)
    n = 1 << log2
    cells = np.zeros((3, 2), np.int64)
    for i, b in enumerate(case["blocks"]):
        co = np.zeros(n * n, np.int16)
        oracle.transform(co, 0, np.ascontiguousarray(case["res"][i], np.int16).ravel(), 0, n, log2, 0, bd)
        same(co, case["coef"][i], f"block {i}")
        cells += tc.threshold_cells(co, n, b["quant_scale"], b["quant_shift"])
    assert cells.min() >= tc.SCAN_TARGET, cells.tolist()
    assert len(case["blocks"]) < 1500
    info = case["info"]
    assert info["mask"][0] & 1 and info["mask3"][0] & 1 and int(case["coef"][0][0]) >= 32640         # the basis-matched DC block: above every threshold
    assert not info["mask"][1] and not info["mask2"][1] and not info["mask3"][1] and info["sumSq"][1] == 0 and case["cbf"][1] == 0      # the all-zero residual
    assert {b["scan_idx"] for b in case["blocks"]} == {0, 1, 2} and {b["qp"] for b in case["blocks"]} == set(tc.SCAN_QPS)
    assert {(b["is_intra"], b["sdh"]) for b in case["blocks"]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert (case["cbf"] != 0).any() and ((info["mask"] != 0) & (info["mask2"] == 0)).any() and (info["mask3"] != 0).any()


def test_workspace_layout_arithmetic():
    """csrc/rdoq_work.h restated: two uint32[66] arrays and four uint32 rounded up to 16 bytes, 32-byte RdoqInfo records, a uint32 of order per job, 64 spare bytes"""
    assert tc.INFO_OFFSET == 544 and tc.INFO_DT.itemsize == tc.INFO_BYTES == 32
    assert [tc.workspace_bytes(n) for n in (0, 1, 9)] == [608, 644, 544 + 36 * 9 + 64]
    assert tc.rdoq_thresholds(26214, 19) == [11, 31, 51] and tc.rdoq_thresholds(16384, 15) == [1, 3, 5]      # ceil((2 k - 1) 2^(shift - 1) / scale)
    m, m2, m3, sq = tc.np_rdoq_info(np.array([0] * 15 + [-32768] + [0] * 240), 16, 26214, 19)
    assert (m, m2, m3, sq) == (8, 8, 8, 1 << 30)                                                            # (row 0, column 15): group gy = 0, gx = 3
    assert tc.np_rdoq_info(np.arange(256) == 4 * 16 + 15, 16, 16384, 15) == (1 << 7, 0, 0, 1)


# ================================================================================================================== part 1: forward
def check_forward(hv, oracle, route, res, seed, counts=None):
    log2, tr, bd = route
    lay = tc.forward_layout(res, bd, seed)
    for count in counts or [len(res)]:
        jobs = lay["jobs"][:count]
        want = tc.oracle_forward(oracle, bd, log2, tr, lay["src"], lay["ss"], lay["pred"], lay["sp"], jobs, lay["ncoef"])
        got = tc.device_forward(hv, bd, log2, tr, lay["src"], lay["ss"], lay["pred"], lay["sp"], jobs, lay["ncoef"])
        same(got, want, f"{tc.route_id(route)}, {count} jobs: coefficient buffer")
        assert (want != tc.COEF_SENTINEL).any()


@gpu
@routes
def test_forward_impulses(hv, oracle, route):
    """one job per (y, x) and sign: the residual is 0 everywhere but +-max there (a source of all max / all 0 against a prediction that differs at one sample):
    every basis entry and every lane-to-row mapping, N^2 jobs a sign"""
    log2, tr, bd = route
    n, mx = 1 << log2, (1 << bd) - 1
    res = tc.impulse_residuals(n, mx)
    s = np.where(res.sum(axis=(1, 2), keepdims=True) > 0, mx, 0) + np.zeros_like(res)
    dt = cases.sample_dtype(tc.S_of(bd))
    src, ss, so = tc.strip(s.astype(dt), dt, 4)
    pred, sp, po = tc.strip((s - res).astype(dt), dt, 12, tc.slot_order(len(res), 3))
    jobs = np.stack([(tc.slot_order(len(res), 4) + 1) * n * n, so, po, 0 * so], axis=1).astype(np.int32)
    ncoef = (len(res) + 2) * n * n
    want = tc.oracle_forward(oracle, bd, log2, tr, src, ss, pred, sp, jobs, ncoef)
    same(tc.device_forward(hv, bd, log2, tr, src, ss, pred, sp, jobs, ncoef), want, tc.route_id(route))
    assert len(np.unique(want)) > n


@gpu
@routes
def test_forward_basis_matched_blocks(hv, oracle, route):
    """residual (y, x) = sign(M[k][y]) sign(M[l][x]) max: the largest magnitude each coefficient can take (all (k, l) to 8x8, the corner and middle rows above)"""
    log2, tr, bd = route
    res, _ = tc.basis_matched_residuals(log2, tr, (1 << bd) - 1)
    check_forward(hv, oracle, route, res, 11)


@gpu
@routes
def test_forward_extreme_residuals_and_ragged_job_counts(hv, oracle, route):
    """constants +-max and 0, checkerboards, the residuals that put 0x00 / 0x7f / 0x80 / 0xff in the low and 0 / -1 in the high byte plane of the matrix-core
    kernel's operand; all of them, then the first 1, TPW - 1, TPW, TPW + 1, 2 TPW + 1 (and 2, 9 at 32x32) of them in launches of their own"""
    log2, tr, bd = route
    res = tc.extreme_residuals(1 << log2, (1 << bd) - 1, 5)
    counts = tc.ragged_counts(log2, mfma=log2 == 5)
    assert max(counts) <= len(res)
    check_forward(hv, oracle, route, res, 21, [len(res)] + counts)


@gpu
@routes
def test_forward_block_offsets_in_the_plane(hv, oracle, route):
    """random 160x160 planes at the plane's own stride: source and prediction blocks at every residue mod 4 in x and at the first and last rows and columns"""
    log2, tr, bd = route
    n = 1 << log2
    rng = np.random.default_rng(31 + log2)
    S = tc.S_of(bd)
    src, pred = cases.rand_plane(rng, S, bd).ravel(), cases.rand_plane(rng, S, bd, kind="extremes" if tr else "uniform").ravel()
    xs, ys = [0, 1, 2, 3, W - n - 3, W - n - 2, W - n - 1, W - n], [0, 1, H - n - 1, H - n]
    pos = [(x, y) for y in ys for x in xs]
    jobs = np.array([((i + 1) * n * n, cases.off(*pos[i]), cases.off(*pos[(5 * i + 3) % len(pos)]), 0) for i in range(len(pos))], np.int32)
    ncoef = (len(pos) + 2) * n * n
    want = tc.oracle_forward(oracle, bd, log2, tr, src, W, pred, W, jobs, ncoef)
    same(tc.device_forward(hv, bd, log2, tr, src, W, pred, W, jobs, ncoef), want, tc.route_id(route))


def rerun_without_mfma(select):
    """the switch HAVOC_TU_MFMA is read once per process: the selected tests again in an interpreter of their own with the 32x32 forward transform of 8-bit
    content on the vector units (k_tu_forward<1, 5>)"""
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-p", "no:cacheprovider", "-k", select], capture_output=True, text=True,
                         timeout=900, env=dict(os.environ, HAVOC_TU_MFMA="0"), cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0 and "failed" not in out.stdout and "skipped" not in out.stdout, out.stdout[-1500:] + out.stderr[-500:]
    return int(re.search(r"(\d+) passed", out.stdout).group(1))


@gpu
def test_forward_32x32_8bit_on_the_vector_units():
    assert rerun_without_mfma("test_forward and n32dct-8bit and not vector_units") >= 4      # impulses, basis-matched, extremes and ragged counts, offsets


# ================================================================================================================== part 2: reconstruct
def check_reconstruct(hv, oracle, route, levels, pred, src, launches, seed):
    log2, tr, bd = route
    lay = tc.reconstruct_layout(levels, pred, src, bd, seed)
    args = (bd, log2, tr, launches, lay["rec"], lay["sr"], lay["pred"], lay["sp"], lay["src"], lay["ss"], lay["levels"], lay["jobs"], lay["nssd"])
    want_rec, want_ssd = tc.oracle_reconstruct(oracle, *args)
    got_rec, got_ssd = tc.device_reconstruct(hv, *args)
    same(got_rec, want_rec, f"{tc.route_id(route)}: reconstruction buffer")
    same(got_ssd, want_ssd, f"{tc.route_id(route)}: ssd buffer")
    live = sorted(i for _, lo, hi in launches for i in range(lo, hi))
    assert (want_ssd[[i for i in range(lay["nssd"]) if i not in live]] == tc.SSD_SENTINEL).all()
    return want_rec, want_ssd, lay


def rand_samples(rng, count, n, bd):
    return rng.integers(0, 1 << bd, (count, n, n))


@gpu
@routes
def test_reconstruct_every_dequantiser(hv, oracle, route):
    """qp 0 .. 51 at 8-bit, .. 57 at 9-bit, .. 63 at 10-bit (scale and shift of cases.dequant_params: all six scales, every shift), a dense random block of levels
    in [-48, 48] each"""
    log2, tr, bd = route
    n, nqp = 1 << log2, 52 + 6 * (bd - 8)
    rng = np.random.default_rng(50 + log2)
    check_reconstruct(hv, oracle, route, rng.integers(-48, 49, (nqp, n, n)), rand_samples(rng, nqp, n, bd), rand_samples(rng, nqp, n, bd),
                      [(qp, qp, qp + 1) for qp in range(nqp)], 51)


@gpu
@routes
def test_reconstruct_clips(hv, oracle, route):
    """the level blocks that reach the de-quantiser clip, the first-pass clip, the residual clip and the sample clip (test_every_clip_is_reached_from_both_sides says
    which, from numpy): dense +-32767 / -32768, lone +-32767 at DC and at (N - 1, N - 1), at qp 0 / 30 / 51, against predictions of all 0 and all max"""
    log2, tr, bd = route
    levels, pred, launches = tc.clip_cases(log2, tr, bd)
    src = rand_samples(np.random.default_rng(60), len(levels), 1 << log2, bd)
    check_reconstruct(hv, oracle, route, levels, pred, src, launches, 61)


@gpu
@routes
def test_reconstruct_impulse_levels(hv, oracle, route):
    """one job per (y, x) with level +1 and one with -1, at a mid QP (30) and at the largest scale (51): the inverse basis"""
    log2, tr, bd = route
    n = 1 << log2
    lv = tc.impulse_residuals(n, 1)
    rng = np.random.default_rng(70)
    mid = np.full((2 * len(lv), n, n), 1 << (bd - 1))
    check_reconstruct(hv, oracle, route, np.concatenate([lv, lv]), mid, rand_samples(rng, 2 * len(lv), n, bd), [(30, 0, len(lv)), (51, len(lv), 2 * len(lv))], 71)


@gpu
@routes
def test_reconstruct_sparse_blocks(hv, oracle, route):
    """only the top-left k x k non-zero for k in {1, 3, 4, 5, 7, 8, 9, 15, 16, 17, N}, the same with a single level just outside the square, only row 0, only
    column 0, the all-zero block: the boundaries at which a kernel that skips the zero part of a block goes wrong"""
    log2, tr, bd = route
    n = 1 << log2
    lv = tc.sparse_level_blocks(n, 80 + log2)
    rng = np.random.default_rng(81)
    check_reconstruct(hv, oracle, route, lv, rand_samples(rng, len(lv), n, bd), rand_samples(rng, len(lv), n, bd), [(27, 0, len(lv))], 82)


@gpu
@routes
def test_reconstruct_ssd_extremes(hv, oracle, route):
    """source 0 against a reconstruction of all max and the reverse (about 1.07e9 at 10-bit 32x32, the oracle's `>> 4` included), and source == reconstruction: 0"""
    log2, tr, bd = route
    n, mx = 1 << log2, (1 << bd) - 1
    full, zero = np.full((n, n), mx), np.zeros((n, n), np.int64)
    same_blk = np.random.default_rng(90).integers(0, mx + 1, (n, n))
    _, ssd, _ = check_reconstruct(hv, oracle, route, np.zeros((3, n, n), np.int16), [full, zero, same_blk], [zero, full, same_blk], [(32, 0, 3)], 91)
    big = n * n * mx * mx
    assert ssd[:3].tolist() == [big >> 4 if bd > 8 else big] * 2 + [0]


@gpu
@routes
def test_reconstruct_in_place(hv, oracle, route):
    """pred and rec the same buffer and offset at the plane's stride, the TUs of a wavefront adjacent in the plane (and one in the plane's last corner); expected:
    the oracle, in place, in job order"""
    log2, tr, bd = route
    n = 1 << log2
    rng = np.random.default_rng(100 + log2)
    S = tc.S_of(bd)
    plane, src = cases.rand_plane(rng, S, bd).ravel(), cases.rand_plane(rng, S, bd).ravel()
    per_row = W // n
    count = min(3 * (64 // n) + 1, per_row * per_row - 1)
    offs = [cases.off((i % per_row) * n, (i // per_row) * n) for i in range(count)] + [cases.off(W - n, H - n)]
    order = tc.slot_order(len(offs), 101)
    jobs = np.array([(order[i] * n * n, offs[(7 * i + 2) % len(offs)], offs[i], offs[i]) for i in range(len(offs))], np.int32)
    levels = rng.integers(-48, 49, len(offs) * n * n).astype(np.int16)
    args = (bd, log2, tr, [(27, 0, len(offs))], plane, W, None, W, src, W, levels, jobs, len(offs) + 3)
    want_rec, want_ssd = tc.oracle_reconstruct(oracle, *args)
    got_rec, got_ssd = tc.device_reconstruct(hv, *args)
    same(got_rec, want_rec, f"{tc.route_id(route)}: plane")
    same(got_ssd, want_ssd, f"{tc.route_id(route)}: ssd")
    assert not np.array_equal(want_rec, plane)


@gpu
@routes
def test_reconstruct_ragged_job_counts(hv, oracle, route):
    """1, TPW - 1, TPW, TPW + 1, 2 TPW + 1 jobs: the reconstruction strip (stride > N) and the longer ssd buffer keep their sentinel outside the live jobs"""
    log2, tr, bd = route
    n = 1 << log2
    total = 2 * (64 // n) + 1
    rng = np.random.default_rng(110 + log2)
    lv, pred, src = rng.integers(-48, 49, (total, n, n)), rand_samples(rng, total, n, bd), rand_samples(rng, total, n, bd)
    for count in tc.ragged_counts(log2):
        _, ssd, lay = check_reconstruct(hv, oracle, route, lv, pred, src, [(24, 0, count)], 111)
        assert (ssd[count:] == tc.SSD_SENTINEL).all() and lay["sr"] > n


# ================================================================================================================== part 3: the scan folded into the forward transform
def run_scan(hv, case, lay, bd, log2, count):
    """tu_forward_scan on the first `count` jobs -> (coefficients, level buffer after the scan, RdoqInfo records, then rdoq_prescanned: levels, cbf; havoc_mi355x_rdoq on
    the same coefficients: levels, cbf)"""
    import torch
    from turingcodec_amd.havoc import RDOQ_JOB_DT
    assert int(hv.L.havoc_mi355x_rdoq_workspace(count)) == tc.workspace_bytes(count) == 544 + 36 * count + 64, "the workspace layout of csrc/rdoq_work.h moved"
    d_src, d_pred = hv.up(lay["src"]), hv.up(lay["pred"])
    jobs = hv.up(np.ascontiguousarray(lay["jobs"][:count]))
    with torch.cuda.stream(hv.tstream):
        rjobs = torch.from_numpy(np.ascontiguousarray(lay["rjobs"][:count], RDOQ_JOB_DT).view(np.uint8).reshape(-1).copy()).to(hv.device)
        states = torch.from_numpy(np.ascontiguousarray(case["states"]).reshape(-1)).to(hv.device)
    coef = hv.up(np.full(lay["ncoef"], tc.COEF_SENTINEL, np.int16))
    levels = hv.up(np.full(lay["nlevel"], tc.LEVEL_SENTINEL, np.int16))
    work = hv.rdoq_workspace(count)
    hv.tu_forward_scan_d(bd, log2, coef, d_src, lay["ss"], d_pred, lay["sp"], jobs, rjobs, levels, work)
    zeroed = hv.down(levels, np.int16).copy()
    raw = hv.down(work, np.int64).view(np.uint8)
    info = raw[tc.INFO_OFFSET:tc.INFO_OFFSET + tc.INFO_BYTES * count].copy().view(tc.INFO_DT)
    cbf = hv.up(np.full(count + 4, -7, np.int32))
    hv.rdoq_prescanned_d(bd, log2, levels, coef, states, rjobs, cbf, work)
    levels2, cbf2 = hv.up(np.full(lay["nlevel"], tc.LEVEL_SENTINEL, np.int16)), hv.up(np.full(count + 4, -7, np.int32))
    hv.rdoq_d(bd, log2, levels2, coef, states, rjobs, cbf2, hv.rdoq_workspace(count))
    return hv.down(coef, np.int16), zeroed, info, hv.down(levels, np.int16), hv.down(cbf, np.int32), hv.down(levels2, np.int16), hv.down(cbf2, np.int32)


def check_scan(hv, oracle, bd, log2, count=None):
    case = tc.scan_case(oracle, bd, log2)
    lay = tc.scan_layout(case, bd, log2)
    count = count or len(case["blocks"])
    what = f"{1 << log2}x{1 << log2} {bd}-bit, {count} jobs"
    coef, zeroed, info, levels, cbf, levels2, cbf2 = run_scan(hv, case, lay, bd, log2, count)
    want_coef, want_zeroed, want_levels = tc.expected_buffers(case, lay, log2, count)
    # 1. coefficients: the oracle's, and tu_forward's
    same(coef, want_coef, f"{what}: coefficients of tu_forward_scan")
    same(tc.device_forward(hv, bd, log2, 0, lay["src"], lay["ss"], lay["pred"], lay["sp"], lay["jobs"][:count], lay["ncoef"]), want_coef, f"{what}: coefficients of tu_forward")
    # 2. the level buffer: zero on exactly the N^2 levels at each dst_off
    same(zeroed, want_zeroed, f"{what}: level buffer after the scan")
    # 3. the RdoqInfo records
    for name in tc.INFO_DT.names:
        same(info[name], case["info"][name][:count], f"{what}: RdoqInfo.{name}")
    # 4. levels and coded-block flags: rdoq_prescanned == rdoq == the oracle
    want_cbf = np.concatenate([case["cbf"][:count], np.full(4, -7, np.int32)])
    same(levels, want_levels, f"{what}: levels of rdoq_prescanned")
    same(levels2, want_levels, f"{what}: levels of rdoq")
    same(cbf, want_cbf, f"{what}: cbf of rdoq_prescanned")
    same(cbf2, want_cbf, f"{what}: cbf of rdoq")
    assert lay["jobs"][0, 0] != 0 and lay["jobs"][0, 1] != 0 and (lay["rjobs"]["dst_off"] != lay["rjobs"]["src_off"]).all()      # job 0 is not block 0 of the buffers


@gpu
@scans
def test_scan_in_forward_on_the_thresholds(hv, oracle, bd, log2):
    """all blocks of tu_chain_tools.scan_case in one launch: coefficients, zeroed level blocks, RdoqInfo (mask / mask2 / mask3 with groups ON thr - 1 and thr, sumSq),
    then levels and flags"""
    check_scan(hv, oracle, bd, log2)


@gpu
@scans
def test_scan_in_forward_ragged_job_counts(hv, oracle, bd, log2):
    for count in tc.ragged_counts(log2, mfma=log2 == 5):
        check_scan(hv, oracle, bd, log2, count)


@gpu
def test_scan_in_forward_32x32_8bit_on_the_vector_units():
    assert rerun_without_mfma("test_scan_in_forward and n32dct-8bit and not vector_units") >= 2      # all blocks in one launch, ragged counts


@gpu
def test_scan_argument_errors(hv, oracle):
    """log2 3, a workspace one byte short, a misaligned workspace, a null level buffer with n > 0: non-zero with a message, and the context stays usable"""
    import torch
    from turingcodec_amd.havoc import RDOQ_JOB_DT
    bd, log2, count = 8, 4, 3
    case = tc.scan_case(oracle, bd, log2)
    lay = tc.scan_layout(case, bd, log2)
    d_src, d_pred, jobs = hv.up(lay["src"]), hv.up(lay["pred"]), hv.up(np.ascontiguousarray(lay["jobs"][:count]))
    with torch.cuda.stream(hv.tstream):
        rjobs = torch.from_numpy(np.ascontiguousarray(lay["rjobs"][:count], RDOQ_JOB_DT).view(np.uint8).reshape(-1).copy()).to(hv.device)
    coef = hv.up(np.full(lay["ncoef"], tc.COEF_SENTINEL, np.int16))
    levels = hv.up(np.full(lay["nlevel"], tc.LEVEL_SENTINEL, np.int16))
    work = hv.rdoq_workspace(count)
    need = tc.workspace_bytes(count)
    assert work.numel() * 8 >= need + 8

    def call(log2_, lv, wptr, wbytes):
        return hv.L.havoc_mi355x_tu_forward_scan(hv.h, 1, bd, log2_, coef.data_ptr(), d_src.data_ptr(), lay["ss"], d_pred.data_ptr(), lay["sp"], jobs.data_ptr(), count,
                                                 rjobs.data_ptr(), lv, wptr, wbytes)

    for what, rc in (("log2 3", call(3, levels.data_ptr(), work.data_ptr(), need)), ("workspace one byte short", call(log2, levels.data_ptr(), work.data_ptr(), need - 1)),
                     ("misaligned workspace", call(log2, levels.data_ptr(), work.data_ptr() + 8, need)), ("null level buffer", call(log2, None, work.data_ptr(), need))):
        assert rc != 0, what
        assert len(hv.L.havoc_mi355x_last_error()) > 0, what
    hv.sync()
    same(hv.down(coef, np.int16), np.full(lay["ncoef"], tc.COEF_SENTINEL, np.int16), "a refused call wrote coefficients")
    same(hv.down(levels, np.int16), np.full(lay["nlevel"], tc.LEVEL_SENTINEL, np.int16), "a refused call wrote levels")
    assert call(log2, levels.data_ptr(), work.data_ptr(), need) == 0
    same(hv.down(coef, np.int16), tc.expected_buffers(case, lay, log2, count)[0], "coefficients after the errors")
