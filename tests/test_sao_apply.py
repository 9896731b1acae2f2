"""The in-loop SAO of a picture (havoc_mi355x_sao_apply; the encoder's TaskSao -> LoopFilter::Picture::applySaoCTU -> filterBlockSao,
turing/LoopFilter.h:795-1008): what a picture holds after SAO, before it is padded and becomes a reference.

CPU: the restatement of tests/sao_apply_tools.py against the reference's own LoopFilter::Picture (tests/sao_apply_shim.cpp, compiled at
test time) in both of its forms, on fresh pictures with slices and disabled regions; the bounds helper against processCtu; the generator's
branch coverage; the difference from sao_decide's destination (computeSaoDistortion's form).  GPU: the device against the reference's
committed outputs (tests/golden/sao_apply_golden.npz) and the restatement, on whole pictures with a sentinel around every plane, chained
after sao_estimate and sao_decide, from a captured graph, and its argument checks."""
import os

import numpy as np
import pytest

import reflibs
import sao_apply_tools as A
import sao_decision_tools as T
import sao_merge_tools as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sao_apply_golden.npz")
needs_ref = pytest.mark.skipif(T.reference_dir() is None or not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "obj", "havoc.o")),
                               reason="reference sources or oracle/Makefile's ref objects not present (the shim compiles them at test time)")
PLANES = ("y", "cb", "cr")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def shim():
    return A.Shim()


def _golden_seeds(golden):
    return sorted({int(k[1:]) for k in golden.files if k.startswith("y")})


def _golden_planes(golden, s, pic):
    return [(pic["rec_" + k].astype(np.int32) + golden[f"{k}{s}"]).astype(pic["rec_" + k].dtype) for k in PLANES]


def _same(got, want, what):
    for p, (g, w) in enumerate(zip(got, want)):
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, PLANES[p], len(bad), bad[:6])


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_bounds_record_matches_the_header():
    import re
    from turingcodec_amd.havoc import SAO_BOUNDS_DT
    text = open(os.path.join(ROOT, "include", "havoc_mi355x.h")).read()
    assert re.search(r"\}\s*havoc_mi355x_sao_bounds;\s*/\*\s*32 bytes", text) and SAO_BOUNDS_DT.itemsize == 32
    body = text[text.index("int32_t left, top, right, bottom;"):text.index("havoc_mi355x_sao_bounds;")]
    assert "int32_t corners;" in body and "reserved[3]" in body
    assert [SAO_BOUNDS_DT.fields[k][1] for k in ("left", "top", "right", "bottom", "corners")] == [0, 4, 8, 12, 16]
    assert "int havoc_mi355x_sao_apply(" in text


def test_bounds_of_one_slice_are_the_picture_edges():
    from turingcodec_amd.havoc import sao_bounds_table
    b = sao_bounds_table(200, 136, 64)
    assert (b["left"] == 0).all() and (b["top"] == 0).all() and (b["right"] == 200).all() and (b["bottom"] == 136).all()
    c = b["corners"].reshape(3, 4)
    assert c[0, 0] == 8 and c[0, 3] == 4 and c[2, 0] == 2 and c[2, 3] == 1 and c[1, 1] == 15


def test_bounds_of_a_later_slice_are_set_by_the_later_ctu():
    """slice 1 starts at CTU 5 of a 4-wide picture without crossing: CTU 4 (slice 0) loses its right and bottom neighbours to CTUs 5 and
    8, which say so with THEIR flag; with slice 1 crossing they stay"""
    from turingcodec_amd.havoc import sao_bounds_table
    b = sao_bounds_table(256, 192, 64, (0, 5), (1, 0))
    assert b[4]["right"] == 64 and b[1]["bottom"] == 64 and b[4]["bottom"] == 128 and not b[4]["corners"] & 8
    assert b[5]["left"] == 64 and b[5]["top"] == 64 and b[9]["top"] == 0 and b[9]["left"] == 0
    b = sao_bounds_table(256, 192, 64, (0, 5), (0, 1))
    assert b[4]["right"] == 256 and b[4]["bottom"] == 192 and b[4]["corners"] & 8


@needs_ref
def test_bounds_are_the_references(shim):
    for s in range(40):
        pic = A.make_picture(3000 + s, slices=1 + s % 4)
        want = shim.bounds(pic["W"], pic["H"], pic["log2"], pic["slice_starts"], pic["across"])
        b = A.bounds_of(pic)
        got = np.stack([b["left"], b["top"], b["right"], b["bottom"], b["corners"]], 1)
        assert np.array_equal(got, want[:, :5]), s


def test_restatement_matches_golden(golden):
    seeds = _golden_seeds(golden)
    assert len(seeds) >= 30
    for s in seeds:
        pic = A.make_picture(s)
        _same(A.restate(pic), _golden_planes(golden, s, pic), s)


BRANCHES = {"c2_TL_only", "c2_BR_only", "c3_TR_partial", "c3_BL_partial", "band_wrap", "disabled", "partial"}
SIDES = {(e, side) for e in range(4) for side in "LRTB"}


def test_generator_covers_every_branch():
    tags = set()
    for s in range(300):
        A.restate(A.make_picture(5000 + s), tags)
    assert SIDES <= tags, SIDES - tags
    assert BRANCHES <= tags


@needs_ref
def test_restatement_matches_the_reference_on_fresh_pictures(shim):
    """the branches are recorded on the very pictures held against the reference"""
    tags = set()
    for s in range(300):
        pic = A.make_picture(10000 + s)
        enc, dec = shim.picture(pic)
        _same(A.restate(pic, tags), enc, s)
        _same(dec, enc, ("decoder form", s))
    assert SIDES <= tags and BRANCHES <= tags, (SIDES | BRANCHES) - tags


@needs_ref
@pytest.mark.parametrize("log2", [4, 5, 6])
@pytest.mark.parametrize("bd", [8, 9, 10])
def test_restatement_matches_the_reference_every_size_and_depth(shim, log2, bd):
    for k, (W, H) in enumerate(((72, 40), (200, 136), (16 << (log2 - 4), 8), (8, 120))):
        pic = A.make_picture(700 + 10 * log2 + bd + k, W=W, H=H, log2=log2, bd=bd)
        enc, _ = shim.picture(pic)
        _same(A.restate(pic), enc, (W, H, log2, bd))


def test_in_loop_output_differs_from_the_decisions_form_only_on_the_picture_edges():
    """one slice, no disabled regions: sao_decide's destination (computeSaoDistortion's form, filtered against the padding) and the in-loop
    output differ only in the picture's first or last row or column, and they do differ there"""
    oracle = reflibs.Oracle()
    differ = 0
    for s in range(12):
        mp = M.make_picture(400 + s, flags=3 | (4 * (s % 2)))
        recs, dy, dc, _ = M.decide_picture(oracle, mp)
        dec = np.ascontiguousarray(recs.astype(np.int32)).view(A.SAO_DECISION_DT).reshape(-1)
        Y, Cb, Cr = T.planes_of(mp, "rec")
        pic = dict(W=mp["W"], H=mp["H"], log2=mp["log2"], bd=mp["bd"], S=mp["S"], flags=mp["flags"] & 3, rec_y=np.ascontiguousarray(Y),
                   rec_cb=np.ascontiguousarray(Cb), rec_cr=np.ascontiguousarray(Cr), decisions=dec, slice_starts=(0,), across=(1,), block_data=None)
        got = A.restate(pic)
        want = T.planes_of(dict(mp, out_y=dy, out_c=dc), "out")
        for g, w in zip(got, want):
            d = g != w
            interior = d[1:-1, 1:-1]
            assert not interior.any(), (s, np.argwhere(interior)[:4])
            differ += int(d.sum())
    assert differ > 0


def test_decision_step_rejects_sao_on_the_host_route():
    from turingcodec_amd.decisions import DecisionPicture
    with pytest.raises(ValueError, match="device route"):
        DecisionPicture(None, 416, 240, sao=True, search_on_device=False)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hv():
    from turingcodec_amd.havoc import Havoc
    return Havoc(stream="new")


def _device(hv, pic):
    blk = pic.get("block_data")
    bounds = None if pic["slice_starts"] == (0,) and pic["across"] == (1,) and pic.get("default_bounds") else A.bounds_of(pic)
    return hv.sao_apply(pic["bd"], pic["flags"], pic["log2"], pic["rec_y"], pic["rec_cb"], pic["rec_cr"], pic["decisions"], bounds, blk)


@pytest.mark.gpu
def test_device_matches_golden(hv, golden):
    for s in _golden_seeds(golden):
        pic = A.make_picture(s)
        _same(_device(hv, pic), _golden_planes(golden, s, pic), s)


@pytest.mark.gpu
def test_device_matches_restatement_on_fresh_pictures(hv):
    for s in range(20000, 20220):
        pic = A.make_picture(s)
        if s % 3 == 0:
            pic = dict(pic, slice_starts=(0,), across=(1,), default_bounds=True)     # d_bounds = NULL
        _same(_device(hv, pic), A.restate(pic), s)


def _padded_device(hv, pic, pad, sentinel):
    """sao_apply_d over planes with `pad` samples of sentinel on every side (source and destination): -> the destination's three padded
    planes, 2-D"""
    torch = hv.torch
    W, H = pic["W"], pic["H"]
    sy, sc = W + 2 * pad, W // 2 + pad
    rows_y, rows_c = H + 2 * pad, H // 2 + pad
    dt = pic["rec_y"].dtype
    ry = np.full((rows_y, sy), sentinel, dt)
    ry[pad:pad + H, pad:pad + W] = pic["rec_y"]
    rc = np.full((2, rows_c, sc), sentinel, dt)
    pc = pad // 2
    rc[0, pc:pc + H // 2, pc:pc + W // 2] = pic["rec_cb"]
    rc[1, pc:pc + H // 2, pc:pc + W // 2] = pic["rec_cr"]
    d_ry, d_rc = hv.up(ry.ravel()), hv.up(rc.ravel())
    with torch.cuda.stream(hv.tstream):
        d_dy, d_dc = torch.full_like(d_ry, int(sentinel)), torch.full_like(d_rc, int(sentinel))
        d_dec = torch.from_numpy(pic["decisions"].view(np.uint8).reshape(-1).copy()).to(hv.device)
        d_b = torch.from_numpy(A.bounds_of(pic).view(np.uint8).reshape(-1).copy()).to(hv.device)
        blk = pic.get("block_data")
        d_blk = None if blk is None else torch.from_numpy(np.ascontiguousarray(blk).ravel()).to(hv.device)
    oy, ocb, ocr = pad * sy + pad, pc * sc + pc, rows_c * sc + pc * sc + pc
    hv.sao_apply_d(pic["bd"], pic["flags"], W, H, pic["log2"], d_ry, oy, d_rc, ocb, ocr, sy, sc, d_dy, oy, d_dc, ocb, ocr, sy, sc, d_dec, d_b, d_blk,
                   0 if blk is None else blk.shape[1])
    return hv.down(d_dy, dt).reshape(rows_y, sy), hv.down(d_dc, dt).reshape(2, rows_c, sc)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(416, 240), (1920, 1080), (3840, 2160)])
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("ctb", [16, 64])
def test_device_whole_picture_writes_nothing_outside(hv, size, bd, ctb):
    W, H = size
    log2 = ctb.bit_length() - 1
    pic = A.make_picture(W + bd + ctb, W=W, H=H, log2=log2, bd=bd, slices=3)
    pic["decisions"] = A.random_decisions(np.random.default_rng(W + ctb), len(pic["decisions"]), bd, dense=True)
    pad, sentinel = 8, (1 << bd) - 1 - 3
    dy, dc = _padded_device(hv, pic, pad, sentinel)
    want = A.restate(pic)
    pc = pad // 2
    _same([dy[pad:pad + H, pad:pad + W], dc[0, pc:pc + H // 2, pc:pc + W // 2], dc[1, pc:pc + H // 2, pc:pc + W // 2]], want, size)
    my = np.ones(dy.shape, bool)
    my[pad:pad + H, pad:pad + W] = False
    mc = np.ones(dc.shape[1:], bool)
    mc[pc:pc + H // 2, pc:pc + W // 2] = False
    assert (dy[my] == sentinel).all() and (dc[0][mc] == sentinel).all() and (dc[1][mc] == sentinel).all()


@pytest.mark.gpu
def test_device_chain_estimate_decide_apply(hv):
    """sao_estimate -> sao_decide -> sao_apply queued back to back (no host wait), against decide_picture and the restatement"""
    from turingcodec_amd.havoc import SAO_PARAMS_DT, SAO_DECISION_DT
    torch = hv.torch
    oracle = reflibs.Oracle()
    for seed, flags in ((31, 3), (32, 7), (33, 5), (34, 6)):
        mp = M.make_picture(seed, W=416, H=240, log2=5 + seed % 2, bd=8 + 2 * (seed % 2), flags=flags, mode="tiled_noisy")
        want_rec, _, _, _ = M.decide_picture(oracle, mp)
        L, ctus = mp["layout"], T.ctus(mp)
        W, H, P, pc = mp["W"], mp["H"], L["pad"], L["pad"] // 2
        sy, sc, ry, rc = hv.up(mp["src_y"]), hv.up(mp["src_c"]), hv.up(mp["rec_y"]), hv.up(mp["rec_c"])
        with torch.cuda.stream(hv.tstream):
            dy, dc = ry.clone(), rc.clone()
            oy, oc = torch.zeros_like(ry), torch.zeros_like(rc)
            d_ctus = torch.from_numpy(ctus.view(np.uint8).reshape(-1)).to(hv.device)
            params = torch.zeros(len(ctus) * SAO_PARAMS_DT.itemsize, dtype=torch.uint8, device=hv.device)
            dec = torch.zeros(len(ctus) * SAO_DECISION_DT.itemsize, dtype=torch.uint8, device=hv.device)
        work, work2 = hv.sao_workspace(len(ctus)), hv.sao_decide_workspace(len(ctus))
        sl = (L["stride_y"], L["stride_c"])
        hv.sao_estimate_d(mp["bd"], mp["q16"], flags & 3, sy, sc, *sl, ry, rc, *sl, dy, dc, *sl, d_ctus, work, params)
        hv.sao_decide_d(mp["bd"], mp["q16"], flags, sy, sc, *sl, ry, rc, *sl, dy, dc, *sl, d_ctus, M.ctus_x(mp), params, mp["ctx"][0], mp["ctx"][1],
                        work2, dec)
        oy0, ocb, ocr = P * L["stride_y"] + P, pc * L["stride_c"] + pc, L["size_c"] + pc * L["stride_c"] + pc
        hv.sao_apply_d(mp["bd"], flags & 3, W, H, mp["log2"], ry, oy0, rc, ocb, ocr, *sl, oy, oy0, oc, ocb, ocr, *sl, dec)
        got_dec = hv.down(dec, np.uint8).view(SAO_DECISION_DT)
        assert np.array_equal(got_dec.view(np.int32).reshape(-1, M.NREC).astype(np.int64), want_rec)
        Y, Cb, Cr = T.planes_of(mp, "rec")
        pic = dict(W=W, H=H, log2=mp["log2"], bd=mp["bd"], S=mp["S"], flags=flags & 3, rec_y=Y, rec_cb=Cb, rec_cr=Cr,
                   decisions=np.ascontiguousarray(want_rec.astype(np.int32)).view(SAO_DECISION_DT).reshape(-1), slice_starts=(0,), across=(1,))
        dt = mp["rec_y"].dtype
        got = T.planes_of(dict(mp, out_y=hv.down(oy, dt), out_c=hv.down(oc, dt)), "out")
        _same(got, A.restate(pic), seed)


@pytest.mark.gpu
def test_device_call_replays_from_a_graph(hv):
    torch = hv.torch
    a, b = A.make_picture(41, W=416, H=240, log2=6, bd=10, slices=2), A.make_picture(42, W=416, H=240, log2=6, bd=10, slices=2)
    b.update(slice_starts=a["slice_starts"], across=a["across"], block_data=a["block_data"])
    W, H = a["W"], a["H"]
    ry, rc = hv.up(a["rec_y"].ravel()), hv.up(np.concatenate([a["rec_cb"].ravel(), a["rec_cr"].ravel()]))
    with torch.cuda.stream(hv.tstream):
        oy, oc = torch.zeros_like(ry), torch.zeros_like(rc)
        dec = torch.from_numpy(a["decisions"].view(np.uint8).reshape(-1).copy()).to(hv.device)
        bnd = torch.from_numpy(A.bounds_of(a).view(np.uint8).reshape(-1).copy()).to(hv.device)
        blk = None if a["block_data"] is None else torch.from_numpy(np.ascontiguousarray(a["block_data"]).ravel()).to(hv.device)
    bs = 0 if a["block_data"] is None else a["block_data"].shape[1]
    nc = W * H // 4
    hv.sync()
    g = hv.graph_capture(lambda: hv.sao_apply_d(10, a["flags"], W, H, 6, ry, 0, rc, 0, nc, W, W // 2, oy, 0, oc, 0, nc, W, W // 2, dec, bnd, blk, bs))
    try:
        for pic in (a, b):
            with torch.cuda.stream(hv.tstream):
                ry.copy_(hv.up(pic["rec_y"].ravel()))
                rc.copy_(hv.up(np.concatenate([pic["rec_cb"].ravel(), pic["rec_cr"].ravel()])))
                dec.copy_(torch.from_numpy(pic["decisions"].view(np.uint8).reshape(-1).copy()).to(hv.device))
                oy.zero_()
                oc.zero_()
            hv.graph_launch(g)
            hv.sync()
            c = hv.down(oc, np.uint16)
            got = [hv.down(oy, np.uint16).reshape(H, W), c[:nc].reshape(H // 2, W // 2), c[nc:].reshape(H // 2, W // 2)]
            _same(got, A.restate(dict(pic, flags=a["flags"])), "replay")
    finally:
        hv.graph_destroy(g)


@pytest.mark.gpu
def test_device_rejects_bad_arguments(hv):
    from turingcodec_amd.havoc import HavocError
    torch = hv.torch
    pic = A.make_picture(7, W=64, H=64, log2=5, bd=8, disabled=True)
    W, H = 64, 64
    ry, rc = hv.up(pic["rec_y"].ravel()), hv.up(np.concatenate([pic["rec_cb"].ravel(), pic["rec_cr"].ravel()]))
    with torch.cuda.stream(hv.tstream):
        oy, oc = torch.zeros_like(ry), torch.zeros_like(rc)
        dec = torch.from_numpy(pic["decisions"].view(np.uint8).reshape(-1).copy()).to(hv.device)
        blk = torch.zeros(64, dtype=torch.int8, device=hv.device)
    nc = W * H // 4

    def call(bd=8, W=W, H=H, log2=5, src=(ry, rc), dst=(oy, oc), d=dec, b=None, bs=0, flags=3, offs=(0, nc)):
        hv.sao_apply_d(bd, flags, W, H, log2, src[0], 0, src[1], offs[0], offs[1], 64, 32, dst[0], 0, dst[1], offs[0], offs[1], 64, 32, d, None, b, bs)
    call()                                                          # the arguments as given are fine
    with pytest.raises(HavocError, match="overlaps"):
        call(dst=(ry, oc))
    with pytest.raises(HavocError, match="overlaps"):
        call(dst=(oy, rc))
    with pytest.raises(HavocError, match="destination planes overlap"):
        call(offs=(0, 8))
    with pytest.raises(HavocError, match="ctb_log2"):
        call(log2=3)
    with pytest.raises(HavocError, match="ctb_log2"):
        call(log2=7)
    with pytest.raises(HavocError, match="multiples of 8"):
        call(W=60)
    with pytest.raises(HavocError, match="multiples of 8"):
        call(H=0)
    with pytest.raises(HavocError, match="bitDepth"):
        call(bd=9)                                                  # 8-bit samples
    with pytest.raises(HavocError, match="bitDepth"):
        call(bd=11)
    with pytest.raises(HavocError, match="null"):
        call(d=None)
    with pytest.raises(HavocError, match="block_stride"):
        call(b=blk, bs=7)
    call(b=blk, bs=8)
    with pytest.raises(HavocError, match="flags"):
        call(flags=4)


def _strided_device(hv, pic, sy, sc, cr_gap, sentinel):
    """sao_apply_d over planes at row strides sy (luma) / sc (chroma), Cr starting cr_gap samples after Cb's last row, sentinel everywhere else; -> the
    three picture planes of the destination and whether every other destination sample kept the sentinel"""
    torch = hv.torch
    W, H = pic["W"], pic["H"]
    dt = pic["rec_y"].dtype
    ny, ncb = H * sy, (H // 2) * sc
    ocr = ncb + cr_gap
    ry = np.full(ny, sentinel, dt)
    ry.reshape(H, sy)[:, :W] = pic["rec_y"]
    rc = np.full(ocr + ncb, sentinel, dt)
    rc[:ncb].reshape(H // 2, sc)[:, :W // 2] = pic["rec_cb"]
    rc[ocr:].reshape(H // 2, sc)[:, :W // 2] = pic["rec_cr"]
    d_ry, d_rc = hv.up(ry), hv.up(rc)
    with torch.cuda.stream(hv.tstream):
        d_dy, d_dc = torch.full_like(d_ry, int(sentinel)), torch.full_like(d_rc, int(sentinel))
        d_dec = torch.from_numpy(pic["decisions"].view(np.uint8).reshape(-1).copy()).to(hv.device)
        d_b = torch.from_numpy(A.bounds_of(pic).view(np.uint8).reshape(-1).copy()).to(hv.device)
        blk = pic.get("block_data")
        d_blk = None if blk is None else torch.from_numpy(np.ascontiguousarray(blk).ravel()).to(hv.device)
    hv.sao_apply_d(pic["bd"], pic["flags"], W, H, pic["log2"], d_ry, 0, d_rc, 0, ocr, sy, sc, d_dy, 0, d_dc, 0, ocr, sy, sc, d_dec, d_b, d_blk,
                   0 if blk is None else blk.shape[1])
    dy, dc = hv.down(d_dy, dt), hv.down(d_dc, dt)
    Y, Cb, Cr = dy.reshape(H, sy), dc[:ncb].reshape(H // 2, sc), dc[ocr:].reshape(H // 2, sc)
    rest = np.concatenate([Y[:, W:].ravel(), Cb[:, W // 2:].ravel(), Cr[:, W // 2:].ravel(), dc[ncb:ocr]])
    return [Y[:, :W], Cb[:, :W // 2], Cr[:, :W // 2]], bool((rest == sentinel).all())


@pytest.mark.gpu
@pytest.mark.parametrize("strides", [(1, 1, 1), (3, 1, 0), (0, 3, 0), (0, 0, 1), (4, 2, 2)])
def test_device_on_unaligned_planes(hv, strides):
    """odd strides and a Cr plane at an odd offset take the per-sample loads and stores; aligned ones the dword / 8-byte ones: same result"""
    ey, ec, gap = strides
    for k, bd in enumerate((8, 10)):
        pic = A.make_picture(60 + 7 * sum(strides) + k, W=200, H=136, log2=5 - k, bd=bd, slices=2)
        got, kept = _strided_device(hv, pic, pic["W"] + ey, pic["W"] // 2 + ec, gap, (1 << bd) - 2)
        _same(got, A.restate(pic), (strides, bd))
        assert kept, (strides, bd)


# ---- the decision step with SAO (DecisionPicture(sao=True)) ----------------------------------------------------------------------------------
def _dp_planes(dp, y, c):
    """(Y, Cb, Cr) padded 2-D views of a luma buffer in recon's layout and a chroma buffer in crecon's"""
    return y[:dp.n].reshape(-1, dp.stride), c[:dp.cn].reshape(-1, dp.cstride), c[dp.cpe:dp.cpe + dp.cn].reshape(-1, dp.cstride)


def _inner(dp, planes):
    P, c2, W, H = dp.PAD, dp.PAD // 2, dp.W, dp.H
    return [np.ascontiguousarray(planes[0][P:P + H, P:P + W])] + [np.ascontiguousarray(p[c2:c2 + H // 2, c2:c2 + W // 2]) for p in planes[1:]]


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(416, 240), (1920, 1080)])
def test_decision_step_with_sao(hv, size):
    from turingcodec_amd.decisions import DecisionPicture
    from turingcodec_amd.havoc import sao_layout, sao_context_init
    oracle = reflibs.Oracle()
    W, H = size
    off = DecisionPicture(hv, W, H, 8, 32, seed=5)
    off.step()
    luma_off = _inner(off, _dp_planes(off, hv.down(off.recon, off.dt), hv.down(off.crecon, off.dt)))[0]
    dp = DecisionPicture(hv, W, H, 8, 32, seed=5, sao=True)
    _, field, _ = dp.step()
    P, c2, dt = dp.PAD, dp.PAD // 2, dp.dt
    deb = _inner(dp, _dp_planes(dp, hv.down(dp.deblocked, dt), hv.down(dp.cdeblocked, dt)))
    # 1. deblocking of the luma does not depend on SAO or on the chroma
    assert np.array_equal(deb[0], luma_off)
    # 2. the decisions are decide_picture's on (source, deblocked), WPP, the picture's lambda, a B slice's contexts
    pad = lambda a, p: np.pad(a, p, mode="edge").ravel()
    src = dp.host_planes[0].reshape(-1, dp.stride)[P:P + H, P:P + W]
    csrc = [dp.host_chroma[k].reshape(-1, dp.cstride)[c2:c2 + H // 2, c2:c2 + W // 2] for k in (0, 3)]
    mp = dict(W=W, H=H, log2=6, bd=8, S=1, q16=dp.rqt_plan["rl_q16"], flags=7, layout=sao_layout(W, H), ctx=sao_context_init(32, 2),
              src_y=pad(src, 8), rec_y=pad(deb[0], 8), src_c=np.concatenate([pad(c, 4) for c in csrc]), rec_c=np.concatenate([pad(c, 4) for c in deb[1:]]))
    want_rec, _, _, _ = M.decide_picture(oracle, mp)
    decisions = dp.sao_decisions
    assert np.array_equal(decisions.view(np.int32).reshape(-1, M.NREC).astype(np.int64), want_rec)
    assert (decisions["comp"]["type"] != 0).any()
    # 3. the final planes are the in-loop SAO of the deblocked picture
    n64 = (W + 63) // 64 * 8 + 1
    blk = hv.down(dp.d_data, np.int8).reshape(-1, n64)
    final_y, final_c = hv.down(dp.recon, dt), hv.down(dp.crecon, dt)
    fin = _dp_planes(dp, final_y, final_c)
    pic = dict(W=W, H=H, log2=6, bd=8, S=1, flags=3, rec_y=deb[0], rec_cb=deb[1], rec_cr=deb[2], decisions=decisions, slice_starts=(0,), across=(1,),
               block_data=blk)
    _same(_inner(dp, fin), A.restate(pic), size)
    # 4. the borders are padBlock's
    for plane, o, w, h, stride, p in ((final_y[:dp.n].copy(), dp.origin, W, H, dp.stride, P), (final_c[:dp.cn].copy(), dp.corigin, W // 2, H // 2, dp.cstride, c2),
                                      (final_c[dp.cpe:dp.cpe + dp.cn].copy(), dp.corigin, W // 2, H // 2, dp.cstride, c2)):
        padded = plane.copy()
        oracle.pad_block(padded, o, w, h, stride, p, 1, 1, 1, 1)
        assert np.array_equal(plane, padded)
    # 5. a second step (the graph replay) repeats it
    dp.step()
    assert np.array_equal(dp.sao_decisions, decisions)
    assert np.array_equal(hv.down(dp.recon, dt), final_y) and np.array_equal(hv.down(dp.crecon, dt), final_c)
    # 6. stopped after the chroma chain: the deblocking is oracle_deblock's on the reconstruction as the chain left it, with the step's strengths
    dp.merge_candidates(field)
    dp.predict(field)
    dp.sao_filter_inputs(field)
    hv.sync()
    rec = _inner(dp, _dp_planes(dp, hv.down(dp.recon, dt), hv.down(dp.crecon, dt)))
    data, bs = hv.down(dp.d_data, np.int8), hv.down(dp.d_bs, np.uint8)
    dp.sao_loop_filter()
    hv.sync()
    oracle.deblock(rec[0], W, rec[1], rec[2], W // 2, W, H, 8, data, bs)
    _same(_inner(dp, _dp_planes(dp, hv.down(dp.deblocked, dt), hv.down(dp.cdeblocked, dt))), rec, ("oracle_deblock", size))
    assert np.array_equal(hv.down(dp.recon, dt), final_y) and np.array_equal(hv.down(dp.crecon, dt), final_c)
    with pytest.raises(ValueError, match="step_banded"):
        dp.step_banded(hv)
