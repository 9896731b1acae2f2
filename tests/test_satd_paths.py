"""Every Hadamard SATD path of the device pinned at its 16-bit bounds, on every tile form (8x8, 4x4, 2x2) and in every launch class, for equality with the oracle:
`oracle.pu_satd`, `oracle.satd`, `oracle.pred_uni`, `oracle.intra`.  Generators, the numpy restatement and the layouts: tests/satd_tools.py.

  CPU     the numpy restatement equals the oracle (and, per tile, the reference where it is built); the family constants (a full-amplitude Walsh tile, the bent tile, the
          five- and six-stage peaks against 2^15); coverage (every Walsh pattern and sign, every impulse position, a tile whose sum is 2 mod 4, every tile kind and
          every `count` in every launch class); every block and interpolation window at least cases.PAD inside its buffer; both clips of the interpolation reached
          at fractional phases; the intra cases at full amplitude through modes 26 and 10
  part A  havoc_mi355x_satd: k_satd<S, 8 | 16 | 32 | 64>, every shape that fits each class over the mosaics, ragged job counts
  part B  havoc_mi355x_satd_multi: the row form (8, 16 lanes per job) and the tile form (4, 8, 8, 16, 32, 32, 64 lanes per job; satd_tile8_pk / satd_tile8_pk16 and the
          4x4 / 2x2 paths beside them in one launch), every `count`, `count` outside 1 .. 16, ragged job counts; the tile classes again under HAVOC_SATD_TILE=0
  part C  havoc_mi355x_subpel_satd: the mosaics at phase (0, 0) (the adversarial differences reach the kernel's Hadamard exactly), every phase pair on a uniform plane
          and on a plane of 0 / max steps, job counts around the per-workgroup counts
  part D  havoc_mi355x_intra_measure (tile SATDs of the full-amplitude mosaics) and havoc_mi355x_intra_satd35 (half-amplitude sources against flat neighbours, the
          separable Walsh patterns through modes 26 and 10, all 35 modes, both filter-mask polarities)

The output buffers are sentinel-filled, longer than the jobs need, and compared WHOLE: every comparison is also a footprint check.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cases
import satd_tools as st

gpu = pytest.mark.gpu
BDS = st.BIT_DEPTHS
bds = pytest.mark.parametrize("bd", BDS, ids=[f"{bd}bit" for bd in BDS])

SATD_CLASSES = [(8, 8), (16, 8), (16, 16), (64, 64)]                      # lanes per job 8 / 16 / 32 / 64
# (max_w, max_h), tile form?, lanes per job
MULTI_CLASSES = [((8, 8), False, 8), ((16, 8), False, 16), ((16, 16), True, 4), ((32, 16), True, 8), ((16, 32), True, 8), ((32, 32), True, 16), ((64, 32), True, 32),
                 ((32, 64), True, 32), ((64, 64), True, 64)]
MULTI_IDS = [f"{'tileform' if t else 'rowform'}{g}-{w}x{h}" for (w, h), t, g in MULTI_CLASSES]
MULTI_JOB_COUNTS = [1, 2, 3, 5, 8, 9, 33]
multi_classes = pytest.mark.parametrize("cls", [c[0] for c in MULTI_CLASSES], ids=MULTI_IDS)


@pytest.fixture(scope="module")
def hv():
    from turingcodec_amd import Havoc
    return Havoc(0)


def same(got, want, what, per_job=1, cells=None):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    assert got.size == want.size, f"{what}: {got.size} values, want {want.size}"
    bad = np.flatnonzero(got != want)
    if bad.size:
        job = int(bad[0]) // per_job
        where = f"{st.label(cells, job)}, slot {int(bad[0]) % per_job}" if cells is not None and job < len(cells) else f"job {job} (past the last job)" if cells is not None else ""
        raise AssertionError(f"{what}: {bad.size} of {want.size} differ, first at {bad[:8].tolist()} ({where}): got {got[bad[:8]].tolist()}, want {want[bad[:8]].tolist()}")


# ================================================================================================================== expected values: the oracle's, computed once
_pairs = {}


def oracle_pairs(oracle, bd, quads):
    """oracle.pu_satd of every (a_off, b_off, w, h) on the mosaic planes"""
    m = st.mosaic(bd)
    out = np.zeros(len(quads), np.int32)
    for i, q in enumerate(np.asarray(quads).tolist()):
        key = (bd, *q)
        if key not in _pairs:
            _pairs[key] = oracle.pu_satd(m.a, q[0], m.sa, m.b, q[1], m.sb, q[2], q[3])
        out[i] = _pairs[key]
    return out


def oracle_multi(oracle, bd, jobs):
    """[n, 16]: the oracle's value of every (a, b_k) pair, used or not"""
    quads = np.stack([np.repeat(jobs[:, 0], 16), jobs[:, 4:].ravel(), np.repeat(jobs[:, 1], 16), np.repeat(jobs[:, 2], 16)], axis=1)
    return oracle_pairs(oracle, bd, quads).reshape(-1, 16)


_subpel = {}


def oracle_subpel(oracle, plane_key, taps, bd, src, ss, ref, sr, jobs):
    """oracle.pred_uni into a 64-stride block, then oracle.pu_satd against the source (suite.LoopImpl.subpel_satd)"""
    out = np.zeros(len(jobs), np.int32)
    pred = np.zeros(64 * 64, ref.dtype)
    for i, j in enumerate(np.asarray(jobs).tolist()):
        key = (plane_key, taps, bd, *j[:6])
        if key not in _subpel:
            so, ro, w, h, xf, yf = j[:6]
            oracle.pred_uni(pred, 0, 64, ref, ro, sr, w, h, xf, yf, bd, taps)
            _subpel[key] = oracle.pu_satd(src, so, ss, pred, 0, 64, w, h)
        out[i] = _subpel[key]
    return out


def oracle_intra35(oracle, bd, case):
    """oracle.intra into a block, then oracle.pu_satd (8x8 tiles, one 4x4 for a 4x4 block), as suite.LoopImpl.intra_satd35 composes them"""
    jobs = case["jobs"].astype(np.int64)
    out = np.zeros((len(jobs), 35), np.int32)
    pred = np.zeros(32 * 32, case["nb"].dtype)
    for i, j in enumerate(jobs.tolist()):
        so, no, nfo, lo, hi, edge, log2 = j[:7]
        mask = (lo & 0xffffffff) | ((hi & 0xffffffff) << 32)
        for mode in range(35):
            # the job's `edge` says cIdx == 0; the edge filters of DC, 10 and 26 apply below 32x32 only (include/havoc_mi355x.h; suite.LoopImpl.intra)
            oracle.intra(pred, 0, 32, case["nb"], nfo if (mask >> mode) & 1 else no, log2, mode, 1 if (edge and log2 < 5) else 0, bd)
            out[i, mode] = oracle.pu_satd(case["src"], so, case["ss"], pred, 0, 32, 1 << log2, 1 << log2)
    return out


# ================================================================================================================== CPU: the restatement, the constants, the coverage
@bds
def test_numpy_restatement_equals_the_oracle(oracle, bd):
    """tiling 8x8 / 4x4 / 2x2 by shape, (s + 2) >> 2 / (s + 1) >> 1 / s, the 16-bit tables' extra >> 2: on every shape, over the mosaics (the block's own cell and
    another one) and over random data"""
    m = st.mosaic(bd)
    rng = np.random.default_rng(bd)
    ra, rb = cases.rand_plane(rng, m.S, bd).ravel(), cases.rand_plane(rng, m.S, bd, kind="extremes").ravel()
    W = cases.PLANE_W
    assert {st.kind_of(*s) for s in st.SHAPES} == {2, 4, 8} and set(cases.PU_SIZES) | set(cases.CHROMA_PU_SIZES) | set(st.EXTRA_SHAPES) == set(st.SHAPES)
    for (w, h) in st.SHAPES:
        cells = st.grid_positions(w, h)
        for (x, y) in cells[::max(1, len(cells) // 8)]:
            for k in (0, 3):
                bx, by = st.candidate_position(w, h, x, y, k)
                want = oracle.pu_satd(m.a, m.a_off(x, y), m.sa, m.b, m.b_off(bx, by), m.sb, w, h)
                assert st.np_pu_satd(m.block_a(x, y, w, h), m.block_b(bx, by, w, h), m.S) == want, (w, h, x, y, k)
        for _ in range(3):
            (ax, ay), (bx, by) = cases.rand_pos(rng, w, h), cases.rand_pos(rng, w, h)
            want = oracle.pu_satd(ra, cases.off(ax, ay), W, rb, cases.off(bx, by), W, w, h)
            assert st.np_pu_satd(ra.reshape(-1, W)[ay:ay + h, ax:ax + w], rb.reshape(-1, W)[by:by + h, bx:bx + w], m.S) == want, (w, h)


@bds
def test_numpy_restatement_equals_the_reference_per_tile(reference_c, oracle, bd):
    """every tile of the three families: the reference's own hadamard_satd table == the oracle == the numpy restatement"""
    m = st.mosaic(bd)
    for n, (y0, rows) in st.REGION.items():
        for y in range(y0, y0 + rows, n):
            for x in range(0, st.MW, n):
                want = reference_c.satd(m.a, m.a_off(x, y), m.sa, m.b, m.b_off(x, y), m.sb, n)
                assert oracle.satd(m.a, m.a_off(x, y), m.sa, m.b, m.b_off(x, y), m.sb, n) == want, (n, x, y)
                assert int(st.np_tile_satd(m.block_a(x, y, n, n).astype(np.int64) - m.block_b(x, y, n, n), m.S)) == want, (n, x, y)


def test_family_constants(oracle):
    """a full-amplitude Walsh tile costs 4080 / 2044 / 4092 and the bent tile 32640 / 16352 / 32736 at 8 / 9 / 10 bits (the oracle's values); the five stages between
    registers peak at exactly 32 mx (32736 at 10 bits: below 2^15), the sixth at 64 mx: above 2^15 at 10 bits only"""
    assert st.WALSH_COST == {8: 4080, 9: 2044, 10: 4092} and st.BENT_COST == {8: 32640, 9: 16352, 10: 32736}
    for bd in BDS:
        m = st.mosaic(bd)
        mx = m.mx
        fam = m.tiles[8]
        d = np.array([a - b for _, a, b in fam])
        tags = [t for t, _, _ in fam]
        sums = st.np_tile_sum(d)
        for i, tag in enumerate(tags):
            gx, gy = i % 16, i // 16
            cost = oracle.satd(m.a, m.a_off(8 * gx, 8 * gy), m.sa, m.b, m.b_off(8 * gx, 8 * gy), m.sb, 8)
            if tag[0] == "walsh":
                assert cost == st.WALSH_COST[bd] and sums[i] == 64 * mx, (bd, tag, cost)
                c = st.hadamard(8) @ d[i] @ st.hadamard(8).T
                assert np.count_nonzero(c) == 1 and c[tag[1], tag[2]] == tag[3] * 64 * mx, (bd, tag)
                assert st.np_stage_peaks(d[i])[4:] == [32 * mx, 64 * mx], (bd, tag)
            if tag[0] == "bent":
                assert cost == st.BENT_COST[bd] and sums[i] == 512 * mx == sums.max(), (bd, tag, cost)
                assert (np.abs(st.hadamard(8) @ d[i] @ st.hadamard(8).T) == 8 * mx).all(), (bd, tag)
        peaks = st.np_stage_peaks(d)
        assert peaks[4] == 32 * mx < 1 << 15 and peaks[5] == 64 * mx, (bd, peaks)
        assert (peaks[5] > 1 << 15) == (bd == 10)
    assert 32 * 1023 == 32736 and 64 * 255 == 16320 and 64 * 511 == 32704 and 64 * 1023 == 65472
    # the 4x4 analogues: 16 mx on one coefficient, every coefficient 4 mx on the bent tile
    for bd in BDS:
        m = st.mosaic(bd)
        for tag, a, b in m.tiles[4]:
            c = st.hadamard(4) @ (a - b) @ st.hadamard(4).T
            if tag[0] == "walsh":
                assert np.count_nonzero(c) == 1 and c[tag[1], tag[2]] == tag[3] * 16 * m.mx
            if tag[0] == "bent":
                assert (np.abs(c) == 4 * m.mx).all()


def kinds_in(jobs_wh):
    return {st.kind_of(int(w), int(h)) for w, h in jobs_wh}


@bds
def test_coverage(bd):
    """every (u, v, sign), every impulse position, a random tile whose sum is 2 mod 4 (the only ones that show the rounding term), all 16 sign patterns at 2x2; every
    launch class holds jobs of each tile kind that fits it -- among ALL its jobs and among the first of the ragged launches -- and, in part B, every count with each"""
    m = st.mosaic(bd)
    for n in (8, 4):
        tags = {t for t, _, _ in m.tiles[n]}
        assert {("walsh", u, v, s) for u in range(n) for v in range(n) for s in (1, -1)} <= tags
        assert {t[1] for t in tags if t[0] == "impulse"} == set(range(n * n)) and {t[2] for t in tags if t[0] == "impulse"} == {1, -1}
        assert {t[1] for t in tags if t[0] == "bent"} == {"plain", "negated", "transposed"}
        assert {t[1] for t in tags if t[0] == "random"} == {"uniform", "extremes"}
    assert {t[1] for t, _, _ in m.tiles[2] if t[0] == "signs"} == set(range(16))
    sums = {t: int(st.np_tile_sum(a - b)) for t, a, b in m.tiles[8]}
    assert any(s % 4 == 2 for t, s in sums.items() if t[0] == "random"), "no random tile shows the rounding term"
    assert all(s % 4 == 0 for t, s in sums.items() if t[0] != "random")
    assert m.sa != m.sb and m.ax % 2 == 1 and m.bx % 2 == 1 and (m.ax - m.bx) % 4 != 0            # unaligned, and a's and b's alignments differ
    # a 64x64 job covers 64 different family members
    assert len(set(m.tags_under(64, 0, 64, 64))) == 64

    def fitting(cls):
        return {st.kind_of(*s) for s in st.SHAPES if st.fits(s, *cls)}

    for cls in SATD_CLASSES:
        jobs, cells = st.pair_jobs(bd, *cls)
        assert kinds_in(jobs[:, 2:4]) == fitting(cls) == {2, 4, 8} and len(jobs) < 4000
        assert {(int(w), int(h)) for w, h in jobs[:, 2:4]} == set(st.shapes_of(*cls))
    for cls, tile, lanes in MULTI_CLASSES:
        jobs, cells = st.multi_jobs(bd, *cls)
        assert len(jobs) < 4000 and {(int(w), int(h)) for w, h in jobs[:, 1:3]} == set(st.shapes_of(*cls))
        assert {(st.kind_of(int(j[1]), int(j[2])), int(j[3])) for j in jobs} == {(k, c) for k in (2, 4, 8) for c in range(1, 17)}, cls
        assert kinds_in(jobs[:33, 1:3]) == {2, 4, 8} and kinds_in(jobs[:9, 1:3]) >= {8}, cls
        assert all(len(set(j[4:].tolist())) == 16 for j in jobs), "candidates must be distinct"
        if tile:
            assert {(12, 16), (4, 8), (8, 4), (6, 8), (2, 4)} <= {(int(w), int(h)) for w, h in jobs[:, 1:3]}
            # the lanes per job of csrc/kernels_metric.hip launch_satd_multi: the 8x8 tiles of the class's largest block
            assert lanes == (cls[0] // 8) * (cls[1] // 8)
    assert sorted({l for _, t, l in MULTI_CLASSES if t}) == [4, 8, 16, 32, 64]
    for taps in (8, 4):
        for cls in st.SUBPEL_CLASSES:
            jobs = st.subpel_mosaic_jobs(bd, taps, cls)
            assert kinds_in(jobs[:, 2:4]) == ({2, 4, 8}) and len(jobs) < 4000
            assert ({2, 6} & set(jobs[:, 2].tolist()) == {2, 6}) == (taps == 4)
            ph = st.subpel_phase_jobs(taps, cls)
            assert {(int(j[4]), int(j[5])) for j in ph} == set(st.phases(taps)) and len(st.phases(taps)) == (16 if taps == 8 else 64)
            assert kinds_in(ph[:, 2:4]) == ({2, 4, 8} if taps == 4 else {4, 8}) and int(ph[:, 2:4].max()) == cls


def margin(offs, w, h, stride, size, reach=(0, 0)):
    """the smallest distance between the blocks at `offs` (widened by `reach` samples before and after, the interpolation window) and the edges of their buffer"""
    y, x = np.divmod(np.asarray(offs, np.int64), stride)
    return int(min((x - reach[0]).min(), (y - reach[0]).min(), (stride - (x + w + reach[1])).min(), (size // stride - (y + h + reach[1])).min()))


@bds
def test_every_block_and_window_stays_inside_its_buffer(bd):
    """at least cases.PAD samples, the (w + taps - 1) x (h + taps - 1) window of the fused kernel included: windows at the buffer's edge are not this module's subject"""
    m = st.mosaic(bd)
    for cls, _, _ in MULTI_CLASSES:
        jobs, _ = st.multi_jobs(bd, *cls)
        assert margin(jobs[:, 0], jobs[:, 1], jobs[:, 2], m.sa, m.a.size) >= cases.PAD
        assert min(margin(jobs[:, 4 + k], jobs[:, 1], jobs[:, 2], m.sb, m.b.size) for k in range(16)) >= cases.PAD
    for cls in SATD_CLASSES:
        jobs, _ = st.pair_jobs(bd, *cls)
        assert margin(jobs[:, 0], jobs[:, 2], jobs[:, 3], m.sa, m.a.size) >= cases.PAD <= margin(jobs[:, 1], jobs[:, 2], jobs[:, 3], m.sb, m.b.size)
    src, ss, ref, sr = st.subpel_planes(bd, "steps")
    for taps in (8, 4):
        for cls in st.SUBPEL_CLASSES:
            for jobs, sizes in ((st.subpel_mosaic_jobs(bd, taps, cls), (m.sa, m.a.size, m.sb, m.b.size)), (st.subpel_phase_jobs(taps, cls), (ss, src.size, sr, ref.size))):
                assert margin(jobs[:, 0], jobs[:, 2], jobs[:, 3], sizes[0], sizes[1]) >= cases.PAD
                assert margin(jobs[:, 1], jobs[:, 2], jobs[:, 3], sizes[2], sizes[3], (3, 4)) >= cases.PAD
    for log2 in (2, 3, 4, 5):
        case = st.intra_case(bd, log2)
        assert margin(case["jobs"][:, 0], 1 << log2, 1 << log2, case["ss"], case["src"].size) >= cases.PAD
        jobs, _ = st.measure_jobs(bd, log2)
        assert margin(jobs[:, 1], 1 << log2, 1 << log2, m.sa, m.a.size) >= cases.PAD <= margin(jobs[:, 2], 1 << log2, 1 << log2, m.sb, m.b.size)


@pytest.mark.parametrize("taps", [8, 4])
@bds
def test_both_clips_of_the_interpolation_are_reached(oracle, bd, taps):
    """on the step plane, at fractional phases: predictions of the oracle that are 0 where the unclipped interpolation is negative and mx where it is above mx, in the
    jobs of part C (ii) themselves; elsewhere the oracle's prediction is the unclipped value"""
    src, ss, ref, sr = st.subpel_planes(bd, "steps")
    mx = (1 << bd) - 1
    below = above = 0
    for cls in st.SUBPEL_CLASSES:
        jobs = st.subpel_phase_jobs(taps, cls)
        kinds = set()
        for so, ro, w, h, xf, yf, _, _ in jobs.tolist():
            if not (xf or yf):
                continue
            pred = np.zeros(64 * 64, ref.dtype)
            oracle.pred_uni(pred, 0, 64, ref, ro, sr, w, h, xf, yf, bd, taps)
            p = pred.reshape(64, 64)[:h, :w].astype(np.int64)
            raw = st.np_pred_uni_unclipped(ref, sr, ro, w, h, xf, yf, bd, taps)
            assert np.array_equal(p, np.clip(raw, 0, mx)), (cls, w, h, xf, yf)
            lo, hi = int(((raw < 0) & (p == 0)).sum()), int(((raw > mx) & (p == mx)).sum())
            below, above = below + lo, above + hi
            if lo and hi:
                kinds.add(st.kind_of(w, h))
        assert kinds == ({2, 4, 8} if taps == 4 else {4, 8}), (cls, kinds)
    assert below > 100 and above > 100, (below, above)


@bds
def test_intra_cases_reach_full_amplitude(oracle, bd):
    """from the oracle alone: with flat neighbours every mode predicts flat; mode 26 / mode 10 against the complementary source cost a full-amplitude Walsh tile per tile"""
    for log2 in (2, 3, 4, 5):
        case = st.intra_case(bd, log2)
        n = 1 << log2
        want = oracle_intra35(oracle, bd, case)
        walsh = {8: st.WALSH_COST[bd], 4: ((16 * ((1 << bd) - 1) + 1) >> 1) >> (2 if bd > 8 else 0)}[min(n, 8)] * max(1, n // 8) ** 2
        seen = set()
        for i, tag in enumerate(case["tags"]):
            if tag[0] == "half":
                assert len(set(want[i].tolist())) == 1, (log2, tag)
            if tag[0] in ("top", "left"):
                assert want[i, 26 if tag[0] == "top" else 10] == walsh, (log2, tag, want[i].tolist())
                seen.add(tag)
        assert len(seen) == 2 * 2 * 2 * min(n, 8)
        masks = (case["jobs"][:, 3].astype(np.int64) & 0xffffffff) | ((case["jobs"][:, 4].astype(np.int64) & 7) << 32)
        assert (np.bitwise_or.reduce(masks) == (1 << 35) - 1) and np.bitwise_and.reduce(masks) == 0 and set(case["jobs"][:, 5].tolist()) == {0, 1}


# ================================================================================================================== device plumbing
_dev = {}


def planes(hv, bd):
    if bd not in _dev:
        m = st.mosaic(bd)
        _dev[bd] = (hv.up(m.a), hv.up(m.b))
    return _dev[bd]


def sentinels(hv, n):
    return hv.up(np.full(n, st.SENTINEL, np.int32))


# ================================================================================================================== part A: havoc_mi355x_satd
@gpu
@bds
@pytest.mark.parametrize("cls", SATD_CLASSES, ids=[f"{w}x{h}" for w, h in SATD_CLASSES])
def test_satd_classes(hv, oracle, bd, cls):
    """k_satd<S, G>: every shape that fits the class over the mosaics in ONE launch, then the first 1, 256 / G - 1, 256 / G, 256 / G + 1 jobs"""
    m = st.mosaic(bd)
    jobs, cells = st.pair_jobs(bd, *cls)
    want = oracle_pairs(oracle, bd, jobs)
    rows = ((cls[0] + 7) // 8) * cls[1]
    per = 256 // (8 if rows <= 8 else 16 if rows <= 16 else 32 if rows <= 32 else 64)
    a, b = planes(hv, bd)
    assert len(np.unique(want)) > 20 and max(st.WALSH_COST[bd], st.BENT_COST[bd]) in want.tolist()
    for count in [len(jobs), 1, per - 1, per, per + 1]:
        out = sentinels(hv, count + 7)
        hv.satd_d(a, m.sa, b, m.sb, hv.up(jobs[:count]), out, *cls)
        same(hv.down(out, np.int32), np.concatenate([want[:count], np.full(7, st.SENTINEL, np.int32)]), f"satd {cls} {bd}-bit, {count} jobs", 1, cells)


# ================================================================================================================== part B: havoc_mi355x_satd_multi
def multi_expected(table, counts, n):
    want = np.full((n + 1, 16), st.SENTINEL, np.int32)
    for i in range(n):
        c = min(max(int(counts[i]), 0), 16)
        want[i, :c] = table[i, :c]
    return want.ravel()


@gpu
@bds
@multi_classes
def test_satd_multi_classes(hv, oracle, bd, cls):
    """every shape that fits the class (in the tile classes that includes the 4x4- and 2x2-tiled ones, which take the row paths beside the tile path), every count
    1 .. 16, in ONE launch, then the first 1, 2, 3, 5, 8, 9, 33 jobs: slot k < count is the oracle's value of pair k, slots k >= count keep the sentinel"""
    m = st.mosaic(bd)
    jobs, cells = st.multi_jobs(bd, *cls)
    table = oracle_multi(oracle, bd, jobs)
    # a swap of two slots shows: for every two slots some job tells them apart
    assert (table[:, :, None] != table[:, None, :]).any(axis=0)[~np.eye(16, dtype=bool)].all()
    a, b = planes(hv, bd)
    for count in [len(jobs)] + MULTI_JOB_COUNTS:
        out = sentinels(hv, 16 * (count + 1))
        hv.satd_multi_d(a, m.sa, b, m.sb, hv.up(jobs[:count]), out, *cls)
        same(hv.down(out, np.int32), multi_expected(table, jobs[:, 3], count), f"satd_multi {cls} {bd}-bit, {count} jobs", 16, cells)


@gpu
@bds
@multi_classes
def test_satd_multi_classes_count_outside_1_to_16(hv, oracle, bd, cls):
    """include/havoc_mi355x.h: count <= 0 writes nothing, count > 16 acts as 16; the b_off slots past `count` hold in-range offsets"""
    m = st.mosaic(bd)
    jobs, cells = st.multi_jobs(bd, *cls)
    jobs = jobs[:36].copy()
    jobs[:, 3] = np.resize([0, -1, 17, 16, -2147483648, 2147483647, 1, 18, 1000, -7, 15, 32], len(jobs))
    table = oracle_multi(oracle, bd, jobs)
    a, b = planes(hv, bd)
    out = sentinels(hv, 16 * (len(jobs) + 1))
    hv.satd_multi_d(a, m.sa, b, m.sb, hv.up(jobs), out, *cls)
    want = multi_expected(table, jobs[:, 3], len(jobs))
    rows = want.reshape(-1, 16)[:-1]
    assert (rows[jobs[:, 3] <= 0] == st.SENTINEL).all() and (rows[jobs[:, 3] > 16] != st.SENTINEL).all() and (jobs[:, 3] <= 0).sum() >= 9 <= (jobs[:, 3] > 16).sum()
    same(hv.down(out, np.int32), want, f"satd_multi {cls} {bd}-bit, counts outside 1 .. 16", 16, cells)


@gpu
@bds
def test_satd_multi_tile_classes_on_the_row_kernels(bd):
    """the switch HAVOC_SATD_TILE is read once per process: part B's tile classes again in an interpreter of their own with the switch at 0 (k_satd_multi<S, 32 | 64>
    in its row form, which no class reaches otherwise)"""
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-p", "no:cacheprovider", "-k",
                          f"test_satd_multi_classes and tileform and {bd}bit"], capture_output=True, text=True, timeout=600, env=dict(os.environ, HAVOC_SATD_TILE="0"),
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0 and "failed" not in out.stdout and "skipped" not in out.stdout, out.stdout[-1500:] + out.stderr[-500:]
    assert int(re.search(r"(\d+) passed", out.stdout).group(1)) == 2 * sum(1 for c in MULTI_CLASSES if c[1])


# ================================================================================================================== part C: havoc_mi355x_subpel_satd
def run_subpel(hv, taps, bd, cls, d_src, ss, d_ref, sr, jobs):
    cost = sentinels(hv, len(jobs) + 7)
    hv.subpel_satd_d(taps, bd, cls, cls, d_src, ss, d_ref, sr, hv.up(jobs), cost)
    return hv.down(cost, np.int32)


def padded(want):
    return np.concatenate([want, np.full(7, st.SENTINEL, np.int32)])


def job_cells(jobs):
    return np.stack([jobs[:, 4], jobs[:, 5], jobs[:, 2], jobs[:, 3]], axis=1)      # labelled (xFrac, yFrac, w, h)


subpel_routes = pytest.mark.parametrize("taps,cls", [(t, c) for t in (8, 4) for c in st.SUBPEL_CLASSES], ids=[f"{t}tap-class{c}" for t in (8, 4) for c in st.SUBPEL_CLASSES])


@gpu
@bds
@subpel_routes
def test_subpel_satd_mosaics_at_phase_zero(hv, oracle, bd, taps, cls):
    """(i) source = mosaic plane a, reference = mosaic plane b, phase (0, 0): the prediction is the block of b, so the Walsh, bent and impulse differences reach the
    kernel's Hadamard exactly; every shape that fits the class (widths 2 and 6 with 4 taps only)"""
    m = st.mosaic(bd)
    jobs = st.subpel_mosaic_jobs(bd, taps, cls)
    want = oracle_subpel(oracle, "mosaic", taps, bd, m.a, m.sa, m.b, m.sb, jobs)
    assert st.BENT_COST[bd] in want.tolist() and st.WALSH_COST[bd] in want.tolist()
    same(want, oracle_pairs(oracle, bd, jobs[:, :4]), "pred_uni at phase (0, 0) is a copy")
    a, b = planes(hv, bd)
    same(run_subpel(hv, taps, bd, cls, a, m.sa, b, m.sb, jobs), padded(want), f"subpel_satd {taps}-tap class {cls} {bd}-bit over the mosaics", 1, job_cells(jobs))


@gpu
@bds
@subpel_routes
@pytest.mark.parametrize("kind", ["uniform", "steps"])
def test_subpel_satd_every_phase(hv, oracle, bd, taps, cls, kind):
    """(ii) every phase pair x an 8x8-tiled, a 4x4-tiled and (4 taps) a 2x2-tiled shape of the class, on a uniform plane and on the plane of 0 / max steps and
    checkerboards where both clips of the prediction are reached (test_both_clips_of_the_interpolation_are_reached)"""
    src, ss, ref, sr = st.subpel_planes(bd, kind)
    jobs = st.subpel_phase_jobs(taps, cls)
    want = oracle_subpel(oracle, kind, taps, bd, src, ss, ref, sr, jobs)
    got = run_subpel(hv, taps, bd, cls, hv.up(src), ss, hv.up(ref), sr, jobs)
    same(got, padded(want), f"subpel_satd {taps}-tap class {cls} {bd}-bit, {kind} plane (cells are xFrac, yFrac)", 1, job_cells(jobs))


@gpu
@bds
@subpel_routes
def test_subpel_satd_ragged_job_counts(hv, oracle, bd, taps, cls):
    """(iii) 1, J - 1, J, J + 1, 2 J + 1 jobs around the J = 32 / 8 / 2 / 1 jobs of a workgroup: the cost buffer keeps its sentinel past the last job"""
    src, ss, ref, sr = st.subpel_planes(bd, "uniform")
    jobs = st.subpel_phase_jobs(taps, cls)
    per = st.SUBPEL_JOBS_PER_WORKGROUP[cls]
    d_src, d_ref = hv.up(src), hv.up(ref)
    for count in sorted({1, per - 1, per, per + 1, 2 * per + 1} - {0}):
        want = oracle_subpel(oracle, "uniform", taps, bd, src, ss, ref, sr, jobs[:count])
        same(run_subpel(hv, taps, bd, cls, d_src, ss, d_ref, sr, jobs[:count]), padded(want), f"subpel_satd {taps}-tap class {cls} {bd}-bit, {count} jobs", 1, job_cells(jobs))


# ================================================================================================================== part D: the two intra stages
intra_sizes = pytest.mark.parametrize("log2", [2, 3, 4, 5], ids=["4x4", "8x8", "16x16", "32x32"])


@gpu
@bds
@intra_sizes
def test_intra_measure_tile_satds_over_the_mosaics(hv, oracle, bd, log2):
    """havoc_mi355x_intra_measure(with_satd = 1) takes its prediction from a plane: source = mosaic plane a, prediction = mosaic plane b; every tile SATD is
    oracle.satd of that tile (8x8 tiles in raster order, one 4x4 tile for a 4x4 block)"""
    m = st.mosaic(bd)
    n = 1 << log2
    ts = min(n, 8)
    tx = n // ts
    jobs, cells = st.measure_jobs(bd, log2)
    want = np.array([oracle.satd(m.a, j[1] + (t // tx) * ts * m.sa + (t % tx) * ts, m.sa, m.b, j[2] + (t // tx) * ts * m.sb + (t % tx) * ts, m.sb, ts)
                     for j in jobs.tolist() for t in range(tx * tx)], np.int32)
    walsh = st.WALSH_COST[bd] if ts == 8 else ((16 * m.mx + 1) >> 1) >> (2 if bd > 8 else 0)
    assert (want == walsh).sum() >= (128 if ts == 8 else 32) and (ts == 4 or st.BENT_COST[bd] in want.tolist())
    a, b = planes(hv, bd)
    co, co_dct = hv.zeros(len(jobs) * n * n, np.int16), hv.zeros(len(jobs) * n * n, np.int16)
    rec0, ssd0 = hv.zeros(len(jobs) * n * n, st.dtype_of(bd)), hv.zeros(len(jobs), np.uint32)
    satd = sentinels(hv, len(jobs) * tx * tx + 7)
    hv.intra_measure_d(bd, log2, co, co_dct if log2 == 2 else None, satd, rec0, ssd0, a, m.sa, b, m.sb, hv.up(jobs), True)
    same(hv.down(satd, np.int32), padded(want), f"intra_measure {n}x{n} {bd}-bit (slot = tile)", tx * tx, cells)


@gpu
@bds
@intra_sizes
def test_intra_satd35_at_half_and_full_amplitude(hv, oracle, bd, log2):
    """all 35 modes of every job of satd_tools.intra_case: half-amplitude Walsh sources against flat predictions, the separable Walsh patterns at full amplitude
    through modes 26 and 10, random blocks under a filter mask and its complement"""
    case = st.intra_case(bd, log2)
    want = oracle_intra35(oracle, bd, case)
    cost = sentinels(hv, 35 * len(case["jobs"]) + 7)
    hv.intra_satd35_d(bd, log2, hv.up(case["src"]), case["ss"], hv.up(case["nb"]), hv.up(case["jobs"]), cost)
    got = hv.down(cost, np.int32)
    bad = np.flatnonzero(got != padded(want.ravel()))
    assert bad.size == 0, f"intra_satd35 {1 << log2}x{1 << log2} {bd}-bit: {bad.size} differ, first job {bad[0] // 35} {case['tags'][min(bad[0] // 35, len(case['tags']) - 1)]} " \
                          f"mode {bad[0] % 35}: got {got[bad[:8]].tolist()}, want {padded(want.ravel())[bad[:8]].tolist()}"
