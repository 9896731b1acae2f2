"""Deblocking: the CPU oracle against the reference's OWN LoopFilter templates (compiled from its header by
oracle/Makefile, driven in the reference's CTU order), and the GPU kernel against the oracle.

The second half (from "every filter branch and table entry") holds havoc_mi355x_deblock against a numpy restatement of the reference's
templates (tests/deblock_tools.py) that records the branch every edge segment takes.  CPU: the restatement against the oracle and the
reference's templates on fresh pictures, against the reference's committed outputs (tests/golden/deblock_golden.npz), and the generator's
coverage.  GPU: the device against the golden file and the restatement, on whole pictures inside sentinels, on unaligned planes, band by band
as the banded decision step calls it, from a captured graph, and its argument checks.

Coverage of the 220 pictures the device is compared on (seeds 20000..20219), counted in edge segments by the restatement:
  every branch tag of deblock_tools.luma_tags() / chroma_tags() at least 10 times per edge direction; the rarest: strong_clipped V 12 / H 10,
  normal_pq_dEp0_dEq0 V 11, normal_pq_dEp1_dEq0 H 14, normal_pq_dEp0_dEq1 V 17, chroma pq (Cb, V) 17; strong_pq V 28 / H 39, clip_lo V 160 / H 159,
  clip_hi V 252 / H 180, tc0 V 6062 / H 5969, line_skipped_big_tc V 100 / H 94, p1_clipped V 2160 / H 2198, q1_clipped V 2170 / H 2271;
  every luma beta index 16..51 by at least 313 (V) / 328 (H) segments past the dE test, every tc index 18..53 by at least 69 / 93 of them and
  by at least 8 / 14 segments in which tC limited an output; every chroma tc index 0..53 by at least 2 (Cb) / 8 (Cr) vertical and 4 / 7
  horizontal segments.  On a failure the assertion prints the same figures (deblock_tools.coverage).
Sensitivity of the comparison, measured once on the CPU with altered copies of the restatement (not kept):
  tC table entry 53 raised by one: restatement vs oracle differs on 16 of those 220 pictures (727 luma samples) and on none of the inputs of
  test_gpu_deblock_equals_the_oracle (no luma sample differs there for any entry above 47; entry 48 shows in chroma only); entries 50 / 48 /
  19: 18 / 38 / 115 pictures.  beta table entry 16 / 19 / 46 / 51 raised by two: 28 / 30 / 5 / 6 pictures, none of the earlier inputs.
  Sign of the luma tc offset flipped: 261 747 luma samples in 39 531 4x4 cells of 183 pictures (earlier inputs: 1 994 samples, 544 cells,
  5 of 21 pictures); of the luma beta offset: 134 638 samples, 156 pictures (earlier: 22 samples, 1 picture).
"""
import ctypes
import os

import numpy as np
import pytest

import cases
import deblock_tools as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "deblock_golden.npz")
PLANES = ("y", "cb", "cr")


def block_map(rng, width, height, qp_lo=20, qp_hi=45, p_edge=0.6, p_disabled=0.04):
    """LoopFilter::Block arrays on the ((W+63)/64*8 + 1) x ((H+63)/64*8 + 1) grid: QpY and the filter-disabled bit per 8x8 region,
    2-bit strengths for its left edge (rows 0-3, 4-7) and top edge (columns 0-3, 4-7); no strength on the picture boundary"""
    bw, bh = (width + 63) // 64 * 8 + 1, (height + 63) // 64 * 8 + 1
    data = ((rng.integers(qp_lo, qp_hi + 1, (bh, bw)) << 1) | (rng.random((bh, bw)) < p_disabled)).astype(np.int8)
    bs = np.zeros((bh, bw), np.uint8)
    for k in range(4):
        v = np.where(rng.random((bh, bw)) < p_edge, rng.integers(1, 3, (bh, bw)), 0)
        bs |= (v << (2 * k)).astype(np.uint8)
    bs[:, 0] &= 0xF0    # left picture edge: no vertical-edge strength
    bs[0, :] &= 0x0F    # top picture edge
    return data.ravel(), bs.ravel()


def planes(rng, width, height, S, bd, kind):
    mx = (1 << bd) - 1
    dt = cases.sample_dtype(S)

    def one(w, h):
        if kind == "smooth":   # blocky but smooth content: what the filter is for (strong and normal filters both trigger)
            base = np.kron(rng.integers(0, mx + 1, (h // 8 + 1, w // 8 + 1)), np.ones((8, 8)))[:h, :w]
            return np.clip(base * 0.2 + mx * 0.4 + rng.integers(-2, 3, (h, w)), 0, mx).astype(dt)
        if kind in ("dark", "bright"):   # the same blocks within a few steps of 0 / of the maximum: the normal filter's Clip1 at either end
            base = np.kron(rng.integers(0, mx + 1, (h // 8 + 1, w // 8 + 1)), np.ones((8, 8)))[:h, :w]
            low = np.clip(base * 0.03 + rng.integers(-4, 5, (h, w)) * (1 << (bd - 8)), 0, mx)
            return (low if kind == "dark" else mx - low).astype(dt)
        if kind == "extremes":
            return (rng.integers(0, 2, (h, w)) * mx).astype(dt)
        return rng.integers(0, mx + 1, (h, w)).astype(dt)
    return one(width, height), one(width // 2, height // 2), one(width // 2, height // 2)


CASES = [(64, 64, 1, 8), (208, 120, 1, 8), (136, 72, 2, 10), (320, 192, 2, 9), (8, 8, 1, 8)]


@pytest.mark.parametrize("width,height,S,bd", CASES)
@pytest.mark.parametrize("kind", ["smooth", "uniform", "extremes", "dark", "bright"])
def test_oracle_deblock_equals_the_reference_templates(oracle, reference_c, width, height, S, bd, kind):
    rng = np.random.default_rng(width * 7 + height + bd)
    tags = D.new_tags()
    for tc2, beta2, cbq, crq in ((0, 0, 0, 0), (2, -3, 3, -4), (-6, 6, -12, 12)):
        y, cb, cr = planes(rng, width, height, S, bd, kind)
        data, bs = block_map(rng, width, height)
        a = [p.copy() for p in (y, cb, cr)]
        b = [p.copy() for p in (y, cb, cr)]
        oracle.deblock(a[0], width, a[1], a[2], width // 2, width, height, bd, data, bs, tc2, beta2, cbq, crq)
        reference_c.deblock(b[0], width, b[1], b[2], width // 2, width, height, bd, data, bs, tc2, beta2, cbq, crq)
        for k in range(3):
            assert np.array_equal(a[k], b[k]), (kind, k, tc2)
        if kind == "smooth" and width > 8:
            assert not np.array_equal(a[0], y) and not np.array_equal(a[1], cb)   # the filter did something
        if kind in ("dark", "bright"):
            D.restate(dict(W=width, H=height, bd=bd, S=S, y=y, cb=cb, cr=cr, data=data, bs=bs, tc2=tc2, beta2=beta2, cbq=cbq, crq=crq), tags)
    if kind in ("dark", "bright") and width > 8:                                   # ... and the luma Clip1 of that end was held against the reference
        end = "clip_lo" if kind == "dark" else "clip_hi"
        assert tags["V.luma." + end] > 0 and tags["H.luma." + end] > 0, tags


@pytest.mark.gpu
@pytest.mark.parametrize("width,height,S,bd", CASES + [(1920, 1080, 1, 8), (640, 360, 2, 10)])
def test_gpu_deblock_equals_the_oracle(oracle, width, height, S, bd):
    from turingcodec_amd import Havoc
    hv = Havoc(0)
    rng = np.random.default_rng(width + 3 * height + bd)
    for kind, (tc2, beta2, cbq, crq) in (("smooth", (0, 0, 0, 0)), ("uniform", (2, -3, 3, -4)), ("extremes", (-6, 6, -12, 12))):
        y, cb, cr = planes(rng, width, height, S, bd, kind)
        data, bs = block_map(rng, width, height)
        exp = [p.copy() for p in (y, cb, cr)]
        oracle.deblock(exp[0], width, exp[1], exp[2], width // 2, width, height, bd, data, bs, tc2, beta2, cbq, crq)
        got = hv.deblock(bd, y.ravel(), width, cb, cr, width // 2, width, height, data, bs, tc2, beta2, cbq, crq)
        assert np.array_equal(got[0].reshape(y.shape), exp[0]), (kind, "Y")
        assert np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2]), (kind, "C")


# ---- boundary strengths derived from the block structure (havoc_mi355x_derive_bs) -------------------------------------
PART = [[(0, 0, 4, 4)], [(0, 0, 4, 2), (0, 2, 4, 2)], [(0, 0, 2, 4), (2, 0, 2, 4)], [(0, 0, 4, 1), (0, 1, 4, 3)], [(0, 0, 4, 3), (0, 3, 4, 1)],
        [(0, 0, 1, 4), (1, 0, 3, 4)], [(0, 0, 3, 4), (3, 0, 1, 4)]]      # part modes in quarters of the unit size


def random_structure(rng, W, H, p_intra=0.25):
    """a random but legal block structure: coding quadtree down to 8x8, inter part modes with uni / bi motion from a few reference pictures
    (vectors clustered so that some neighbours match, some differ by less than a sample, some by more), transform trees one or two levels
    deep with random coded flags, a few bypass units, per-unit QP.  Returns unit lists (for the reference's event functions) and the same
    structure rasterised into 4x4 cells (for the oracle / device)."""
    from turingcodec_amd.havoc import CELL_DT, CELL_INTRA, CELL_CODED, CELL_NO_FILTER, CELL_PU_LEFT, CELL_PU_TOP
    cus, pus, tus = [], [], []
    cells = np.zeros((H // 4, W // 4), CELL_DT)
    cells["dpb_index"] = -1
    base = [np.array([12, 8]), np.array([-20, 4]), np.array([0, 0])]

    def motion():
        m = base[int(rng.integers(0, 3))] + rng.integers(-5, 6, 2)
        return int(m[0]), int(m[1])

    def tu(x, y, log2, intra, depth):
        if log2 > 2 and (log2 > 5 or (depth < 2 and rng.random() < 0.4)):
            for k in range(4):
                tu(x + (k & 1) * (1 << (log2 - 1)), y + (k >> 1) * (1 << (log2 - 1)), log2 - 1, intra, depth + 1)
            return
        cbf = int(rng.random() < 0.5)
        tus.append((x, y, log2, cbf, intra))
        c = cells[y // 4:(y + (1 << log2)) // 4, x // 4:(x + (1 << log2)) // 4]
        c["tu_log2"] = log2
        c["flags"] |= (CELL_CODED if cbf else 0)

    def cu(x, y, log2):
        if x >= W or y >= H:
            return
        size = 1 << log2
        if log2 > 3 and (x + size > W or y + size > H or rng.random() < (0.9 if log2 == 6 else 0.5)):
            for k in range(4):
                cu(x + (k & 1) * size // 2, y + (k >> 1) * size // 2, log2 - 1)
            return
        intra = int(rng.random() < p_intra)
        qp, bypass = int(rng.integers(20, 40)), int(rng.random() < 0.05)
        cus.append((x, y, log2, intra, qp, bypass))
        c = cells[y // 4:(y + size) // 4, x // 4:(x + size) // 4]
        c["qp_y"] = qp
        c["flags"] = (CELL_INTRA if intra else 0) | (CELL_NO_FILTER if bypass else 0)
        if not intra:
            modes = PART[:3] if log2 == 3 else PART
            q = size // 4
            for dx, dy, w4, h4 in modes[int(rng.integers(0, len(modes)))]:
                px, py, pw, ph = x + dx * q, y + dy * q, w4 * q, h4 * q
                kind = int(rng.integers(0, 3))      # list 0, list 1, both
                m0, m1 = motion(), motion()
                d0 = int(rng.integers(0, 3)) if kind != 1 else -1
                d1 = int(rng.integers(0, 3)) if kind != 0 else -1
                pus.append((px, py, pw, ph, m0[0], m0[1], m1[0], m1[1], d0, d1))
                pc = cells[py // 4:(py + ph) // 4, px // 4:(px + pw) // 4]
                pc["mv"][..., 0, :] = m0
                pc["mv"][..., 1, :] = m1
                pc["dpb_index"][..., 0] = d0
                pc["dpb_index"][..., 1] = d1
                pc["flags"][:, 0] |= CELL_PU_LEFT
                pc["flags"][0, :] |= CELL_PU_TOP
        tu(x, y, log2, intra, 0)

    for y in range(0, H, 64):
        for x in range(0, W, 64):
            cu(x, y, 6)
    return np.array(cus, np.int32), np.array(pus, np.int32).reshape(-1, 10), np.array(tus, np.int32), cells


@pytest.mark.parametrize("W,H,seed", [(128, 64, 1), (416, 240, 2), (200, 136, 3), (640, 360, 4)])
def test_oracle_boundary_strengths_equal_the_reference_derivation(oracle, reference_c, W, H, seed):
    """per-cell restatement (oracle_derive_bs) vs the reference's own processCu / processTu / processRc + sameMotion over the units"""
    cus, pus, tus, cells = random_structure(np.random.default_rng(seed), W, H)
    want = reference_c.derive_bs(W, H, cus, pus, tus)
    got = oracle.derive_bs(cells, W, H)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert len(pus) > 10 and (want[1] != 0).mean() > 0.3 and len(np.unique(want[1] & 3)) == 3      # strengths 0, 1 and 2 all occur


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,seed", [(128, 64, 1), (416, 240, 2), (1920, 1080, 5), (200, 136, 3)])
def test_device_boundary_strengths_equal_the_oracle_and_feed_the_filter(oracle, W, H, seed):
    from turingcodec_amd.havoc import Havoc
    rng = np.random.default_rng(seed)
    cus, pus, tus, cells = random_structure(rng, W, H)
    hv = Havoc()
    want = oracle.derive_bs(cells, W, H)
    got = hv.derive_bs(cells, W, H)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # ... and the derived arrays through the filter: device == oracle
    y, cb, cr = planes(rng, W, H, 1, 8, "smooth")
    ref = [p.copy() for p in (y, cb, cr)]
    oracle.deblock(ref[0], W, ref[1], ref[2], W // 2, W, H, 8, want[0], want[1])
    have = hv.deblock(8, y.ravel(), W, cb, cr, W // 2, W, H, got[0], got[1])
    assert all(np.array_equal(np.asarray(h).reshape(w.shape), w) for h, w in zip(have, ref))
    assert not np.array_equal(ref[0], y)


# ==== every filter branch and table entry (tests/deblock_tools.py) =========================================================================
GPU_SEEDS = range(20000, 20220)      # the pictures the device is held against the restatement on; test_generator_covers_every_branch


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _golden_seeds(golden):
    return sorted({int(k[1:]) for k in golden.files if k.startswith("y")})


def _golden_planes(golden, s, pic):
    return [(pic[k].astype(np.int32) + golden[f"{k}{s}"]).astype(pic[k].dtype) for k in PLANES]


def _same(got, want, what):
    for p, (g, w) in enumerate(zip(got, want)):
        bad = np.argwhere(np.asarray(g) != np.asarray(w))
        assert len(bad) == 0, (what, PLANES[p], len(bad), bad[:6])


def _assert_covered(tags):
    """every branch tag at least 5 times in each edge direction, every luma beta index 16..51 and tc index 18..53 by a segment past the dE
    test, every tc index 18..53 by a luma segment in which tC limited an output, every chroma tc index a QpY of 0..51 can reach"""
    missing, summary = D.coverage(tags, floor=5)
    assert not missing, (missing, summary)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_chroma_can_reach_every_tc_index():
    assert D.chroma_tc_indices() == set(range(54))


def test_generator_draws_what_it_says():
    seen = dict(bd=set(), tc2=set(), beta2=set(), cq=set(), qp=set(), dis=0, n=0, strong_share=0)
    for s in GPU_SEEDS:
        pic = D.make_picture(s)
        assert pic["W"] % 8 == 0 and pic["H"] % 8 == 0 and pic["cbq"] != pic["crq"]
        seen["bd"].add((pic["bd"], pic["S"]))
        seen["tc2"].add(pic["tc2"])
        seen["beta2"].add(pic["beta2"])
        seen["cq"] |= {pic["cbq"], pic["crq"]}
        seen["qp"] |= set((pic["data"] >> 1).tolist())
        seen["dis"] += int((pic["data"] & 1).sum())
        seen["n"] += pic["data"].size
        seen["strong_share"] += pic["beta2"] >= 3 and pic["tc2"] <= -3
    assert seen["bd"] == {(8, 1), (8, 2), (9, 2), (10, 2)}
    assert seen["tc2"] == set(range(-6, 7)) and seen["beta2"] == set(range(-6, 7)) and seen["cq"] == set(range(-12, 13))
    assert seen["qp"] == set(range(52)) and 0.06 < seen["dis"] / seen["n"] < 0.10 and seen["strong_share"] >= 60
    assert {(8, 8), (8, 120), (104, 8), (24, 24), (200, 120)} <= set(D.SIZES)      # no edge at all, 8 x N, N x 8, multiples of 8 but not of 16 / 64


def test_restatement_matches_golden(golden):
    seeds = _golden_seeds(golden)
    assert len(seeds) >= 30
    depths, changed, total = set(), 0, 0
    for s in seeds:
        pic = D.make_picture(s)
        depths.add((pic["bd"], pic["S"]))
        changed += sum(int(np.count_nonzero(golden[f"{k}{s}"])) for k in PLANES)
        total += sum(golden[f"{k}{s}"].size for k in PLANES)
        _same(D.restate(pic), _golden_planes(golden, s, pic), s)
    assert depths == {(8, 1), (8, 2), (9, 2), (10, 2)} and changed * 20 > total      # the file holds filtering, not zeros


def test_oracle_matches_golden(oracle, golden):
    for s in _golden_seeds(golden):
        pic = D.make_picture(s)
        _same(D.run_cpu(oracle, pic), _golden_planes(golden, s, pic), s)


def test_generator_covers_every_branch():
    """a condition on the inputs of test_device_matches_restatement_on_fresh_pictures, decided by the restatement"""
    tags = D.new_tags()
    for s in GPU_SEEDS:
        D.restate(D.make_picture(s), tags)
    _assert_covered(tags)


def test_restatement_matches_the_oracle_on_fresh_pictures(oracle):
    tags = D.new_tags()
    for s in range(10000, 10300):
        pic = D.make_picture(s)
        _same(D.restate(pic, tags), D.run_cpu(oracle, pic), s)
    _assert_covered(tags)


def test_restatement_matches_the_reference_on_fresh_pictures(reference_c):
    """the branches are recorded on the very pictures held against the reference's templates"""
    tags = D.new_tags()
    for s in range(10000, 10300):
        pic = D.make_picture(s)
        _same(D.restate(pic, tags), D.run_cpu(reference_c, pic), s)
    _assert_covered(tags)


@pytest.mark.parametrize("bd,S", [(8, 1), (8, 2), (9, 2), (10, 2)])
def test_restatement_matches_the_oracle_every_size_and_depth(oracle, bd, S):
    for k, (W, H) in enumerate(D.SIZES + ((8, 16), (16, 8), (328, 72))):
        pic = D.make_picture(700 + 10 * bd + S + k, W=W, H=H, bd=bd, S=S)
        got = D.restate(pic)
        _same(got, D.run_cpu(oracle, pic), (W, H, bd, S))
        if (W, H) == (8, 8):
            _same(got, [pic[k] for k in PLANES], "no edge inside an 8x8 picture")


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hv():
    from turingcodec_amd.havoc import Havoc
    return Havoc(stream="new")


def _block_map_d(hv, pic):
    with hv.torch.cuda.stream(hv.tstream):
        return hv.torch.from_numpy(pic["data"].copy()).to(hv.device), hv.torch.from_numpy(pic["bs"].copy()).to(hv.device)


def _device(hv, pic):
    """planes without padding, Cr straight after Cb: -> [Y, Cb, Cr]"""
    W, H, dt = pic["W"], pic["H"], pic["y"].dtype
    nc = W * H // 4
    d_y, d_c = hv.up(pic["y"].ravel()), hv.up(np.concatenate([pic["cb"].ravel(), pic["cr"].ravel()]))
    d_data, d_bs = _block_map_d(hv, pic)
    hv.deblock_d(pic["bd"], d_y, 0, W, d_c, 0, nc, W // 2, W, H, d_data, d_bs, *D.offsets(pic))
    c = hv.down(d_c, dt)
    return [hv.down(d_y, dt).reshape(H, W), c[:nc].reshape(H // 2, W // 2), c[nc:].reshape(H // 2, W // 2)]


@pytest.mark.gpu
def test_device_matches_golden(hv, golden):
    for s in _golden_seeds(golden):
        pic = D.make_picture(s)
        _same(_device(hv, pic), _golden_planes(golden, s, pic), s)


@pytest.mark.gpu
def test_device_matches_restatement_on_fresh_pictures(hv):
    """... and the pictures compared reach every branch and table entry: a green run says each of them was compared on the device"""
    tags = D.new_tags()
    for s in GPU_SEEDS:
        pic = D.make_picture(s)
        _same(_device(hv, pic), D.restate(pic, tags), s)
    _assert_covered(tags)


def _view(buf, off, stride, h, w):
    assert off >= 0 and off + (h - 1) * stride + w <= buf.size
    return np.lib.stride_tricks.as_strided(buf[off:], (h, w), (stride * buf.itemsize, buf.itemsize))


def _laid_out(hv, oracle, pic, ny, nc, oy, ocb, ocr, sy, sc, sentinel, cuts=None):
    """the picture's planes at element offsets oy (in a luma buffer of ny samples, row stride sy) and ocb / ocr (in one chroma buffer of nc
    samples, row stride sc), the sentinel everywhere else; deblocked on the device -- in one call, or band by band at the row `cuts` the way
    the banded decision step calls it -- and by the oracle on the same buffers.  -> (device luma, device chroma, oracle luma, oracle chroma,
    luma mask, chroma mask), the masks true outside the picture"""
    W, H, bd, dt = pic["W"], pic["H"], pic["bd"], pic["y"].dtype
    ly, lc = np.full(ny, sentinel, dt), np.full(nc, sentinel, dt)
    my, mc = np.ones(ny, bool), np.ones(nc, bool)
    for buf, mask, off, stride, k in ((ly, my, oy, sy, "y"), (lc, mc, ocb, sc, "cb"), (lc, mc, ocr, sc, "cr")):
        h, w = pic[k].shape
        assert not (~_view(mask, off, stride, h, w)).any(), "planes overlap"
        _view(buf, off, stride, h, w)[...] = pic[k]
        _view(mask, off, stride, h, w)[...] = False
    want_y, want_c = ly.copy(), lc.copy()
    oracle.deblock(want_y[oy:], sy, want_c[ocb:], want_c[ocr:], sc, W, H, bd, pic["data"], pic["bs"], *D.offsets(pic))
    d_y, d_c = hv.up(ly), hv.up(lc)
    d_data, d_bs = _block_map_d(hv, pic)
    bstride = (W + 63) // 64 * 8 + 1
    cuts = [0, H] if cuts is None else cuts
    assert cuts[0] == 0 and cuts[-1] == H
    for y0, y1 in zip(cuts[:-1], cuts[1:]):
        hv.deblock_d(bd, d_y, oy + y0 * sy, sy, d_c, ocb + (y0 // 2) * sc, ocr + (y0 // 2) * sc, sc, W, y1 - y0, d_data[(y0 // 8) * bstride:],
                     d_bs[(y0 // 8) * bstride:], *D.offsets(pic))
    return hv.down(d_y, dt), hv.down(d_c, dt), want_y, want_c, my, mc


def _padded(pic, pad, extra=0):
    """a layout with `pad` samples around every plane (luma and chroma alike) and strides `extra` wider still: the arguments of _laid_out"""
    W, H = pic["W"], pic["H"]
    sy, sc = W + 2 * pad + extra, W // 2 + 2 * pad + extra
    rows_c = H // 2 + 2 * pad
    return dict(ny=(H + 2 * pad) * sy, nc=2 * rows_c * sc, oy=pad * sy + pad, ocb=pad * sc + pad, ocr=rows_c * sc + pad * sc + pad, sy=sy, sc=sc)


def _check_laid_out(res, sentinel, what):
    gy, gc, wy, wc, my, mc = res
    assert (wy[my] == sentinel).all() and (wc[mc] == sentinel).all()                 # the checker itself stayed inside
    for name, g, w, m in (("luma", gy, wy, my), ("chroma", gc, wc, mc)):
        bad = np.flatnonzero((g != w) & ~m)
        assert len(bad) == 0, (what, name, "picture", len(bad), bad[:6])
        out = np.flatnonzero((g != sentinel) & m)
        assert len(out) == 0, (what, name, "written outside the picture", len(out), out[:6])


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(416, 240), (1920, 1080), (3840, 2160)])
@pytest.mark.parametrize("bd", [8, 10])
def test_device_whole_picture_writes_nothing_outside(hv, oracle, size, bd):
    W, H = size
    pic = D.make_picture(W + bd, W=W, H=H, bd=bd, S=1 if bd == 8 else 2)
    sentinel = (1 << bd) - 1 - 3
    res = _laid_out(hv, oracle, pic, sentinel=sentinel, **_padded(pic, 8, extra=3 if W == 416 else 0))
    _check_laid_out(res, sentinel, (size, bd))
    assert not np.array_equal(D.run_cpu(oracle, pic)[0], pic["y"])


@pytest.mark.gpu
@pytest.mark.parametrize("strides", [(1, 1, 1), (3, 1, 0), (0, 3, 0), (0, 0, 1), (4, 2, 2)])
def test_device_on_unaligned_planes(hv, oracle, strides):
    """odd luma / chroma strides and a Cr plane at an odd element offset"""
    ey, ec, gap = strides
    for k, bd in enumerate((8, 10)):
        pic = D.make_picture(60 + 7 * sum(strides) + k, W=200, H=136, bd=bd, S=1 + k)
        W, H = pic["W"], pic["H"]
        sy, sc = W + ey, W // 2 + ec
        ncb = (H // 2) * sc
        sentinel = (1 << bd) - 2
        res = _laid_out(hv, oracle, pic, ny=H * sy, nc=2 * ncb + gap, oy=0, ocb=0, ocr=ncb + gap, sy=sy, sc=sc, sentinel=sentinel)
        _check_laid_out(res, sentinel, (strides, bd))
        _same([_view(res[0], 0, sy, H, W), _view(res[1], 0, sc, H // 2, W // 2), _view(res[1], ncb + gap, sc, H // 2, W // 2)], D.restate(pic), (strides, bd))


@pytest.mark.gpu
@pytest.mark.parametrize("bd,S", [(8, 1), (10, 2)])
@pytest.mark.parametrize("cuts", [list(range(0, 328, 64)) + [328], [0, 128, 192, 328], [0, 64, 320, 328]])
def test_device_band_by_band_equals_the_whole_picture(hv, oracle, cuts, bd, S):
    """DecisionPicture.step_banded's form: per band the plane pointers at the band's first row, height = the band's rows, the block map
    from row y0 / 8 on.  Bands start on multiples of 64 rows (a multiple of 16 is what the chroma edges need); the call reads four sample
    rows and one block-map row above its first row"""
    pic = D.make_picture(77 + bd, W=200, H=328, bd=bd, S=S)
    sentinel = (1 << bd) - 1 - 3
    lay = _padded(pic, 8, extra=1)
    whole = _laid_out(hv, oracle, pic, sentinel=sentinel, **lay)
    _check_laid_out(whole, sentinel, ("whole", bd))
    banded = _laid_out(hv, oracle, pic, sentinel=sentinel, cuts=cuts, **lay)
    _check_laid_out(banded, sentinel, ("banded", cuts, bd))
    assert np.array_equal(banded[0], whole[0]) and np.array_equal(banded[1], whole[1])


@pytest.mark.gpu
def test_device_call_replays_from_a_graph(hv):
    """the planes and the block map replaced between replays; the offsets are the call's arguments, so both pictures have the first one's"""
    torch = hv.torch
    a, b = D.make_picture(41, W=416, H=240, bd=10, S=2), D.make_picture(42, W=416, H=240, bd=10, S=2)
    b.update(tc2=a["tc2"], beta2=a["beta2"], cbq=a["cbq"], crq=a["crq"])
    W, H = 416, 240
    nc = W * H // 4
    chroma = lambda p: np.concatenate([p["cb"].ravel(), p["cr"].ravel()])
    d_y, d_c = hv.up(a["y"].ravel()), hv.up(chroma(a))
    d_data, d_bs = _block_map_d(hv, a)
    hv.sync()
    g = hv.graph_capture(lambda: hv.deblock_d(10, d_y, 0, W, d_c, 0, nc, W // 2, W, H, d_data, d_bs, *D.offsets(a)))
    try:
        for pic in (a, b, a):
            nd, nb = _block_map_d(hv, pic)
            with torch.cuda.stream(hv.tstream):
                d_y.copy_(hv.up(pic["y"].ravel()))
                d_c.copy_(hv.up(chroma(pic)))
                d_data.copy_(nd)
                d_bs.copy_(nb)
            hv.graph_launch(g)
            hv.sync()
            c = hv.down(d_c, np.uint16)
            _same([hv.down(d_y, np.uint16).reshape(H, W), c[:nc].reshape(H // 2, W // 2), c[nc:].reshape(H // 2, W // 2)], D.restate(pic), "replay")
    finally:
        hv.graph_destroy(g)
    assert not np.array_equal(D.restate(a)[0], D.restate(b)[0])


@pytest.mark.gpu
def test_device_rejects_bad_arguments(hv):
    """one error per REQUIRE of havoc_mi355x_deblock, and the context is usable afterwards"""
    from turingcodec_amd.havoc import HavocError
    pic = D.make_picture(7, W=64, H=64, bd=8, S=1)
    wide = D.make_picture(7, W=64, H=64, bd=10, S=2)
    d_y, d_c = hv.up(pic["y"].ravel()), hv.up(np.concatenate([pic["cb"].ravel(), pic["cr"].ravel()]))
    d_y2 = hv.up(wide["y"].ravel())
    d_data, d_bs = _block_map_d(hv, pic)
    hv.sync()
    before = hv.down(d_y, np.uint8).copy()

    def call(ctx=True, S=1, bd=8, y=d_y, cb=d_c, cr=d_c, W=64, H=64, data=d_data, bs=d_bs, tc2=0, beta2=0):
        ptr = lambda t, off=0: None if t is None else ctypes.c_void_p(t.data_ptr() + off)
        hv._ck(hv.L.havoc_mi355x_deblock(hv.h if ctx else None, S, bd, ptr(y), 64, ptr(cb), ptr(cr, 1024 * S), 32, W, H, ptr(data), ptr(bs), tc2, beta2, 0, 0))
    for match, bad in (("null context", dict(ctx=False)), ("S \\(bytes per sample\\)", dict(S=3)), ("S \\(bytes per sample\\)", dict(S=0)),
                       ("bitDepth", dict(bd=9)), ("bitDepth", dict(bd=7)), ("bitDepth", dict(S=2, y=d_y2, bd=11)),
                       ("multiples of 8", dict(W=60)), ("multiples of 8", dict(H=68)), ("multiples of 8", dict(W=0)), ("multiples of 8", dict(H=4)),
                       ("null plane", dict(y=None)), ("null plane", dict(cb=None)), ("null plane", dict(cr=None)), ("null plane", dict(data=None)),
                       ("null plane", dict(bs=None)), ("-6\\.\\.6", dict(tc2=7)), ("-6\\.\\.6", dict(tc2=-7)), ("-6\\.\\.6", dict(beta2=7)),
                       ("-6\\.\\.6", dict(beta2=-7))):
        with pytest.raises(HavocError, match=match):
            call(**bad)
    hv.sync()
    assert np.array_equal(hv.down(d_y, np.uint8), before)              # a refused call launched nothing
    call(tc2=6, beta2=-6)                                              # the ends of the range are fine, and the context still works
    want = D.restate(dict(pic, tc2=6, beta2=-6, cbq=0, crq=0))
    c = hv.down(d_c, np.uint8)
    _same([hv.down(d_y, np.uint8).reshape(64, 64), c[:1024].reshape(32, 32), c[1024:].reshape(32, 32)], want, "after the refusals")


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,seed,extra", [(200, 136, 3, 5), (416, 240, 2, 1), (64, 64, 6, 16)])
def test_device_boundary_strengths_from_cells_in_a_wider_array(hv, oracle, W, H, seed, extra):
    """cells_stride > width / 4: the picture's cells are the left part of a wider array whose other cells are noise"""
    from turingcodec_amd.havoc import CELL_DT, HavocError
    torch = hv.torch
    rng = np.random.default_rng(seed)
    _, _, _, cells = random_structure(rng, W, H)
    stride = W // 4 + extra
    outer = rng.integers(0, 256, (H // 4 + 2, stride * CELL_DT.itemsize), dtype=np.uint8).view(CELL_DT)
    outer[:H // 4, :W // 4] = cells
    n = ((W + 63) // 64 * 8 + 1) * ((H + 63) // 64 * 8 + 1)
    with torch.cuda.stream(hv.tstream):
        d_cells = torch.from_numpy(np.ascontiguousarray(outer).view(np.uint8).reshape(-1)).to(hv.device)
        data = torch.full((n,), 77, dtype=torch.int8, device=hv.device)
        bs = torch.full((n,), 77, dtype=torch.uint8, device=hv.device)
    hv.derive_bs_d(d_cells, stride, W, H, data, bs)
    want = oracle.derive_bs(cells, W, H)
    assert np.array_equal(hv.down(data, np.int8), want[0]) and np.array_equal(hv.down(bs, np.uint8), want[1])
    for match, bad in (("multiple of 8", dict(stride=W // 4 - 1)), ("multiple of 8", dict(W=W - 4)), ("multiple of 8", dict(H=0)), ("null", dict(cells=None)),
                       ("null", dict(data=None)), ("null", dict(bs=None))):
        a = dict(cells=d_cells, stride=stride, W=W, H=H, data=data, bs=bs)
        a.update(bad)
        with pytest.raises(HavocError, match=match):
            hv.derive_bs_d(a["cells"], a["stride"], a["W"], a["H"], a["data"], a["bs"])
