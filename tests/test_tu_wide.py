"""The fused transform-unit chain (csrc/kernels_tu_fused.hip) at the layouts where 16-byte accesses to coefficient, level and sample rows can go wrong and
tests/test_tu_chain.py does not look: blocks that are not 16-, 8- or 4-byte aligned, blocks packed back to back or one word apart, level blocks RDOQ is to fill
at an odd multiple of 4 levels, reconstruction rows at an odd stride and an odd offset, in place.  Every buffer the device writes is sentinel-filled and compared
WHOLE with what the oracle (tu_chain_tools.oracle_forward / oracle_reconstruct / scan_case) leaves in the same buffer, so each comparison is a footprint check too.

Sizes: every log2 2 .. 5 (DST and DCT at 4x4), 8- and 10-bit; 1, 64 / N - 1 and 64 / N + 1 jobs (a lone block, a wavefront one block short, a wavefront and one
block; 1 and 3 at 32x32).  The 32x32 8-bit forward cases run again on the vector units (HAVOC_TU_MFMA=0) in an interpreter of their own.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cases
import tu_chain_tools as tc

pytestmark = pytest.mark.gpu

ROUTES = [(log2, tr, bd) for (log2, tr) in cases.TRANSFORMS for bd in (8, 10)]
routes = pytest.mark.parametrize("route", ROUTES, ids=[tc.route_id(r) for r in ROUTES])
SCAN_CASES = [(8, 4), (8, 5), (10, 4), (10, 5)]
scans = pytest.mark.parametrize("bd,log2", SCAN_CASES, ids=[f"n{1 << log2}dct-{bd}bit" for bd, log2 in SCAN_CASES])
SHIFTS = (1, 2, 4)      # int16 words: a block at n * n * slot + d is not 16-byte aligned, and not 8- (d 1, 2) or 4-byte (d 1) aligned either


def job_counts(log2):
    tpw = 64 >> log2
    return sorted({1, tpw - 1, tpw + 1} - {0})


@pytest.fixture(scope="module")
def hv():
    from turingcodec_amd import Havoc
    return Havoc(0)


def same(got, want, what):
    bad = np.flatnonzero(np.asarray(got).ravel() != np.asarray(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {np.asarray(want).size} differ, first at {bad[:8].tolist()}: got {np.asarray(got).ravel()[bad[:8]].tolist()}, " \
                          f"want {np.asarray(want).ravel()[bad[:8]].tolist()}"


def slot_layouts(count, n2, seed):
    """[(name, offsets of the blocks, buffer length)]: shuffled slots shifted by d words (neighbours touch; d sentinel words before the first block, n2 - d after the
    last), and the blocks one sentinel word apart (one before the first, one between neighbours, one after the last)"""
    o = tc.slot_order(count, seed)
    out = [(f"slots + {d}", (o * n2 + d).astype(np.int32), (count + 1) * n2) for d in SHIFTS]
    out.append(("one word apart", (1 + o * (n2 + 1)).astype(np.int32), count * (n2 + 1) + 1))
    return out


# ================================================================================================================== forward
_forward_cache = {}


def forward_case(route):
    log2, tr, bd = route
    if route not in _forward_cache:
        n, mx = 1 << log2, (1 << bd) - 1
        res = np.random.default_rng(500 + 10 * log2 + tr + bd).integers(-mx, mx + 1, (max(job_counts(log2)), n, n))
        _forward_cache[route] = tc.forward_layout(res, bd, 510 + log2)
    return _forward_cache[route]


@routes
def test_forward_unaligned_and_packed_coefficient_slots(hv, oracle, route):
    log2, tr, bd = route
    n2 = 1 << 2 * log2
    lay = forward_case(route)
    for count in job_counts(log2):
        for name, offs, ncoef in slot_layouts(count, n2, 520 + count):
            jobs = lay["jobs"][:count].copy()
            jobs[:, 0] = offs
            args = (bd, log2, tr, lay["src"], lay["ss"], lay["pred"], lay["sp"], jobs, ncoef)
            want = tc.oracle_forward(oracle, *args)
            assert (want == tc.COEF_SENTINEL).sum() >= ncoef - count * n2 > 0 and (want[offs] != tc.COEF_SENTINEL).any()
            same(tc.device_forward(hv, *args), want, f"{tc.route_id(route)}, {count} jobs, {name}: coefficient buffer")


def run_scan(hv, lay, bd, log2, count, nlevel):
    import torch
    from turingcodec_amd.havoc import RDOQ_JOB_DT
    d_src, d_pred = hv.up(lay["src"]), hv.up(lay["pred"])
    jobs = hv.up(np.ascontiguousarray(lay["jobs"][:count]))
    with torch.cuda.stream(hv.tstream):
        rjobs = torch.from_numpy(np.ascontiguousarray(lay["rjobs"][:count], RDOQ_JOB_DT).view(np.uint8).reshape(-1).copy()).to(hv.device)
    coef = hv.up(np.full(lay["ncoef"], tc.COEF_SENTINEL, np.int16))
    levels = hv.up(np.full(nlevel, tc.LEVEL_SENTINEL, np.int16))
    work = hv.rdoq_workspace(count)
    hv.tu_forward_scan_d(bd, log2, coef, d_src, lay["ss"], d_pred, lay["sp"], jobs, rjobs, levels, work)
    raw = hv.down(work, np.int64).view(np.uint8)
    return hv.down(coef, np.int16), hv.down(levels, np.int16), raw[tc.INFO_OFFSET:tc.INFO_OFFSET + tc.INFO_BYTES * count].copy().view(tc.INFO_DT)


@scans
def test_forward_scan_level_blocks_at_odd_multiples_of_four(hv, oracle, bd, log2):
    """tu_forward_scan with every RDOQ dst_off = 4 (2 m + 1) levels: the level blocks are 8- but not 16-byte aligned and touch each other; four sentinel words
    before the first, the rest of a slot after the last"""
    n2 = 1 << 2 * log2
    case = tc.scan_case(oracle, bd, log2)
    for count in job_counts(log2):
        lay = tc.scan_layout(case, bd, log2)
        dst = (4 + tc.slot_order(len(case["blocks"]), 530 + count) * n2).astype(np.int32)
        assert ((dst // 4) % 2 == 1).all() and (dst % 4 == 0).all()
        lay["rjobs"]["dst_off"] = dst
        nlevel = (len(case["blocks"]) + 1) * n2
        lay["nlevel"] = nlevel
        what = f"{1 << log2}x{1 << log2} {bd}-bit, {count} jobs"
        coef, zeroed, info = run_scan(hv, lay, bd, log2, count, nlevel)
        want_coef, want_zeroed, _ = tc.expected_buffers(case, lay, log2, count)
        assert (want_zeroed[:4] == tc.LEVEL_SENTINEL).all() and (want_zeroed == 0).sum() == count * n2
        same(coef, want_coef, f"{what}: coefficients")
        same(zeroed, want_zeroed, f"{what}: level buffer after the scan")
        for name in tc.INFO_DT.names:
            same(info[name], case["info"][name][:count], f"{what}: RdoqInfo.{name}")


def test_forward_32x32_8bit_on_the_vector_units():
    """HAVOC_TU_MFMA is read once per process: the 32x32 8-bit forward cases of this file again in an interpreter of their own with k_tu_forward<1, 5>"""
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-p", "no:cacheprovider", "-k",
                          "test_forward and n32dct-8bit and not vector_units"], capture_output=True, text=True, timeout=900, env=dict(os.environ, HAVOC_TU_MFMA="0"),
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0 and "failed" not in out.stdout and "skipped" not in out.stdout, out.stdout[-1500:] + out.stderr[-500:]
    assert int(re.search(r"(\d+) passed", out.stdout).group(1)) == 2      # the coefficient slots, the scan


# ================================================================================================================== reconstruct
def reconstruct_case(route, count, seed):
    """levels in [-48, 48] with a few large ones, prediction and source blocks; the reconstruction strip has an odd row stride and every block starts at an odd
    sample offset, a sentinel column before the first block, two between neighbours and one or two after the last"""
    log2, tr, bd = route
    n = 1 << log2
    S = tc.S_of(bd)
    dt = cases.sample_dtype(S)
    rng = np.random.default_rng(seed)
    levels = rng.integers(-48, 49, (count, n, n))
    levels[rng.random((count, n, n)) < 0.02] = rng.choice([-32768, -3000, 3000, 32767])
    pred, src = rng.integers(0, 1 << bd, (count, n, n)).astype(dt), rng.integers(0, 1 << bd, (count, n, n)).astype(dt)
    p, sp, po = tc.strip(pred, dt, 12, tc.slot_order(count, seed + 1))
    s, ss, so = tc.strip(src, dt, 4, tc.slot_order(count, seed + 2))
    sr = count * (n + 2) + 1
    ro = (1 + tc.slot_order(count, seed + 3) * (n + 2)).astype(np.int32)
    assert sr % 2 == 1 and (ro % 2 == 1).all()
    rec = np.full((n, sr), tc.sample_sentinel(S), dt)
    return dict(levels=levels.astype(np.int16), pred=pred, p=p, sp=sp, po=po, s=s, ss=ss, so=so, rec=rec, sr=sr, ro=ro)


@routes
def test_reconstruct_unaligned_level_slots_and_odd_strips(hv, oracle, route):
    log2, tr, bd = route
    n, n2 = 1 << log2, 1 << 2 * log2
    for count in job_counts(log2):
        c = reconstruct_case(route, count, 600 + 10 * log2 + count)
        for k, (name, offs, nlevel) in enumerate(slot_layouts(count, n2, 610 + count)):
            lv = np.full(nlevel, tc.LEVEL_SENTINEL, np.int16)
            for i in range(count):
                lv[offs[i]:offs[i] + n2] = c["levels"][i].ravel()
            what = f"{tc.route_id(route)}, {count} jobs, levels at {name}"
            if k != 1:
                jobs = np.stack([offs, c["so"], c["po"], c["ro"]], axis=1).astype(np.int32)
                args = (bd, log2, tr, [(27, 0, count)], c["rec"].ravel(), c["sr"], c["p"], c["sp"], c["s"], c["ss"], lv, jobs, count + 3)
            else:
                # in place: the prediction stands in the strip the reconstruction goes to
                rec = c["rec"].copy()
                for i in range(count):
                    rec[:, c["ro"][i]:c["ro"][i] + n] = c["pred"][i]
                jobs = np.stack([offs, c["so"], c["ro"], c["ro"]], axis=1).astype(np.int32)
                args = (bd, log2, tr, [(27, 0, count)], rec.ravel(), c["sr"], None, c["sr"], c["s"], c["ss"], lv, jobs, count + 3)
                what += ", in place"
            want_rec, want_ssd = tc.oracle_reconstruct(oracle, *args)
            got_rec, got_ssd = tc.device_reconstruct(hv, *args)
            same(got_rec, want_rec, f"{what}: reconstruction strip")
            same(got_ssd, want_ssd, f"{what}: ssd buffer")
            keep = np.ones(c["sr"], bool)
            for i in range(count):
                keep[c["ro"][i]:c["ro"][i] + n] = False
            assert keep.sum() == 2 * count + 1 and (want_rec.reshape(n, -1)[:, keep] == tc.sample_sentinel(tc.S_of(bd))).all() and (want_ssd[count:] == tc.SSD_SENTINEL).all()
