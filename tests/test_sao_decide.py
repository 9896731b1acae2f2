"""The merge / off decision of SAO per CTU (havoc_mi355x_sao_decide; turing/EncSao.h:1017-1120, the last step of rdSao).

CPU: the restatement of tests/sao_merge_tools.py against the reference's own rdSao and Search<sao>::go (tests/sao_merge_shim.cpp, compiled
at test time) on fresh pictures, with WPP on and off; the context initialisation and the rate of every state and bin against the
reference's; the generator's branch coverage.  GPU: the device against the reference's committed outputs
(tests/golden/sao_merge_golden.npz) and against the restatement on whole pictures, on a decision step's deblocked output, from a
captured graph, on exact cost ties, and its argument checks."""
import os

import numpy as np
import pytest

import reflibs
import sao_decision_tools as T
import sao_merge_tools as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sao_merge_golden.npz")
needs_ref = pytest.mark.skipif(T.reference_dir() is None, reason="reference sources not present (the shim compiles them at test time)")


@pytest.fixture(scope="module")
def oracle():
    return reflibs.Oracle()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def shim():
    return M.Shim()


def _golden_seeds(golden):
    return sorted(int(k[3:]) for k in golden.files if k.startswith("rec"))


def _mine(rec):
    r = np.asarray(rec, np.int64).copy()
    r[:, 25] = -2
    return r


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_record_matches_the_header():
    import re
    from turingcodec_amd.havoc import SAO_DECISION_DT
    text = open(os.path.join(ROOT, "include", "havoc_mi355x.h")).read()
    assert re.search(r"\}\s*havoc_mi355x_sao_decision;\s*/\*\s*128 bytes", text) and SAO_DECISION_DT.itemsize == 128
    assert SAO_DECISION_DT.fields["merge_left"][1] == 88 and SAO_DECISION_DT.fields["ctx_merge_before"][1] == 104
    assert SAO_DECISION_DT.fields["decided"][1] == 108


def test_context_init_is_the_specs():
    from turingcodec_amd.havoc import sao_context_init
    assert sao_context_init(26, 0) == sao_context_init(26, 1) != sao_context_init(26, 2)
    assert sao_context_init(-5, 1) == sao_context_init(0, 1) and sao_context_init(60, 2) == sao_context_init(51, 2)


def test_restatement_matches_golden(oracle, golden):
    seeds = _golden_seeds(golden)
    assert len(seeds) >= 30
    for s in seeds:
        rec, dy, dc, _ = M.decide_picture(oracle, M.make_picture(s), chroma_stats="reference")
        assert np.array_equal(_mine(rec), M.normalise_shim(golden[f"rec{s}"])), s
        assert np.array_equal(dy, golden[f"dst_y{s}"]) and np.array_equal(dc, golden[f"dst_c{s}"]), s


def test_generator_covers_every_branch(oracle):
    tags, widths = set(), set()
    for s in range(4000, 4300):
        pic = M.make_picture(s)
        M.decide_picture(oracle, pic, tags=tags)
        widths.add(M.ctus_x(pic))
    for w in ("estimate", "off", "up", "left"):
        assert ("win", w) in tags, w
    assert {"chain", "merge_off", "one_wide", "cmax"} <= tags
    assert {("flags", f) for f in range(8)} <= tags
    assert 1 in widths
    # (exact cost ties do not arise from pictures: rates are sums of table entries; test_restatement_keeps_the_first_of_a_tie makes them)


def _tie_case(oracle):
    """a 3 x 2 CTU picture with made-up estimate records: with reciprocal lambda 2, CTU 1's estimate costs exactly what "all off" costs
    (its dist_sao is dist_off + (rate_off - rate_est) / 2; rates are even), so the strict `<` keeps the estimate.  -> (picture, records)"""
    pic = M.make_picture(5, W=96, H=64, log2=5, bd=8, q16=2, flags=1, mode="mixed")
    pic["ctx"] = (14, 19)
    comp = [2, 1, 0, 2, 1, 1, 2, 0, 0, 0, 0]           # luma edge class 1, offsets 2 1 1 2
    est = np.zeros((6, T.NREC), np.int64)
    for i in range(6):
        est[i, :11] = comp if i in (0, 1, 3) else [0] * 11
        est[i, 23] = -1000000 if i == 1 else 10 + i                 # CTU 1: both tied candidates far below any merge's real SSD
        est[i, 22] = -2000000 if i in (0, 3) else est[i, 23]     # CTUs 0 and 3 keep their estimates: a merge with them costs the real SSD
    first = M.decide_picture(oracle, pic, est=(est.copy(), pic["rec_y"].copy(), pic["rec_c"].copy()))[0]
    m, t = int(first[1, 26]) & 255, int(first[1, 26]) >> 8 & 255      # the states at CTU 1 (they do not depend on CTU 1)
    m, r_merge = M.bin_cost(m, 0)
    _, r_type1 = M.bin_cost(t, 1)
    _, r_type0 = M.bin_cost(t, 0)
    r_est, r_off = r_merge + r_type1 + (M.bypass_bins(comp, 8) << 16), r_merge + r_type0
    est[1, 22] = est[1, 23] + (r_off - r_est) // 2
    return pic, est


@pytest.mark.parametrize("wpp", [0, 4])
def test_restatement_keeps_the_first_of_a_tie(oracle, wpp):
    pic, est = _tie_case(oracle)
    pic["flags"] |= wpp
    tags = set()
    rec, _, _, _ = M.decide_picture(oracle, pic, est=(est, pic["rec_y"].copy(), pic["rec_c"].copy()), tags=tags)
    assert "tie" in tags
    assert rec[1, 25] == 1          # the estimate, tried first, keeps CTU 1


@needs_ref
def test_context_init_and_rates_are_the_references(shim):
    from turingcodec_amd.havoc import sao_context_init
    for qp in range(-2, 56):
        for init_type in range(3):
            assert shim.context_states(min(max(qp, 0), 51), init_type) == sao_context_init(qp, init_type), (qp, init_type)
    table = shim.bin_table()
    for s in range(128):
        for b in range(2):
            ns, r = M.bin_cost(s, b)
            assert table[s, b] == ns | r << 8, (s, b)


@needs_ref
@pytest.mark.parametrize("wpp", [0, 4])
def test_restatement_matches_the_reference_on_fresh_pictures(oracle, shim, wpp):
    """>= 2 000 CTUs per WPP setting, both bit depth families, CTB 16 / 32 / 64: every record field, the final distortion, the context
    states and the final planes equal the reference's rdSao over the stand-in handle.  Pictures where a band search starts at position
    29 are left out: the reference reads past its band arrays there (undefined)."""
    nctus, tags, bds, ctbs = 0, set(), set(), set()
    for s in range(10000 + wpp * 1000, 10000 + wpp * 1000 + 700):
        pic = M.make_picture(s)
        pic["flags"] = (pic["flags"] & 3) | wpp
        und = []
        a, ay, ac, _ = M.decide_picture(oracle, pic, tags=tags, chroma_stats="reference", undefined=und)
        if np.array(und).any():
            continue
        b, by, bc = shim.picture(pic)
        assert np.array_equal(_mine(a), M.normalise_shim(b)), s
        assert (b[:, 28] == b[:, 11]).all()          # Cr shares chroma's type, as the device assumes
        assert np.array_equal(ay, by) and np.array_equal(ac, bc), s
        nctus += len(a)
        bds.add(pic["bd"])
        ctbs.add(pic["log2"])
    assert nctus >= 2000
    assert {8, 10} <= bds and ctbs == {4, 5, 6}
    assert {("win", "off"), ("win", "up"), ("win", "left"), "chain"} <= tags


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hv():
    from turingcodec_amd.havoc import Havoc
    return Havoc(stream="new")


def _device(hv, pic, chroma_stats="ctu", flags=None):
    L = pic["layout"]
    dec, _, dy, dc = hv.sao_decide(pic["bd"], pic["q16"], pic["src_y"], pic["src_c"], pic["rec_y"], pic["rec_c"], L["stride_y"], L["stride_c"],
                                   T.ctus(pic, chroma_stats), M.ctus_x(pic), pic["ctx"][0], pic["ctx"][1], pic["flags"] if flags is None else flags)
    return dec.view(np.int32).reshape(-1, M.NREC).astype(np.int64), dy, dc


def _same(hv, oracle, pic, chroma_stats="ctu"):
    want, wy, wc, _ = M.decide_picture(oracle, pic, chroma_stats=chroma_stats)
    got, gy, gc = _device(hv, pic, chroma_stats)
    bad = np.nonzero((got != want).any(1))[0]
    assert len(bad) == 0, (pic["W"], pic["H"], pic["bd"], pic["flags"], bad[:8], got[bad[:1]], want[bad[:1]])
    assert np.array_equal(gy, wy) and np.array_equal(gc, wc)
    return got


@pytest.mark.gpu
def test_device_matches_golden(hv, golden):
    for s in _golden_seeds(golden):
        got, gy, gc = _device(hv, M.make_picture(s), "reference")
        want = M.normalise_shim(golden[f"rec{s}"])
        bad = np.nonzero((_mine(got) != want).any(1))[0]
        assert len(bad) == 0, (s, bad[:8], got[bad[:1]], want[bad[:1]])
        assert np.array_equal(gy, golden[f"dst_y{s}"]) and np.array_equal(gc, golden[f"dst_c{s}"]), s


@pytest.mark.gpu
def test_device_matches_restatement_on_fresh_pictures(hv, oracle):
    tags = set()
    for s in range(20000, 20200):
        pic = M.make_picture(s)
        M.decide_picture(oracle, pic, tags=tags)
        _same(hv, oracle, pic, "reference" if s % 2 else "ctu")
    assert {("win", "off"), ("win", "up"), ("win", "left"), "chain"} <= tags


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(416, 240), (1920, 1080), (3840, 2160)])
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("ctb", [16, 64])
@pytest.mark.parametrize("wpp", [0, 4])
def test_device_whole_picture(hv, oracle, size, bd, ctb, wpp):
    W, H = size
    pic = M.make_picture(W + bd + ctb + wpp, W=W, H=H, log2=ctb.bit_length() - 1, bd=bd, q16=T.lambda_q16_for_qp(22 + (ctb + bd) % 16), flags=3 | wpp,
                         mode="tiled_noisy" if (W + ctb) % 3 else "mixed")
    g = _same(hv, oracle, pic)
    assert len(g) == ((W + ctb - 1) // ctb) * ((H + ctb - 1) // ctb)


@pytest.mark.gpu
def test_device_on_a_decision_steps_deblocked_output(hv, oracle):
    """the reconstruction of a real 416x240 decision step (deblocked), decided after sao_estimate: at least one merge wins"""
    from turingcodec_amd.decisions import DecisionPicture
    from turingcodec_amd.havoc import sao_layout, sao_context_init
    dp = DecisionPicture(hv, 416, 240, 8, 32, seed=5)
    dp.step()
    hv.sync()
    W, H, P = dp.W, dp.H, dp.PAD
    rec = hv.down(dp.recon, dp.dt)[:dp.n].reshape(-1, dp.stride)[P:P + H, P:P + W]
    src = dp.host_planes[0].reshape(-1, dp.stride)[P:P + H, P:P + W]
    cp = (dp.cstride - W // 2) // 2
    csrc = [dp.host_chroma[k].reshape(-1, dp.cstride)[cp:cp + H // 2, cp:cp + W // 2] for k in (0, 3)]
    crec = hv.down(dp.d_chroma, dp.dt).reshape(2, H // 2, W // 2)
    L = sao_layout(W, H)
    pad = lambda a, p: np.pad(a, p, mode="edge").ravel()
    merges = 0
    for flags, qp in ((3, 27), (7, 32), (3, 37), (7, 37)):
        pic = dict(W=W, H=H, log2=5, bd=8, S=1, q16=T.lambda_q16_for_qp(qp), flags=flags, layout=L, ctx=sao_context_init(qp, 0),
                   src_y=pad(src, 8), rec_y=pad(rec, 8), src_c=np.concatenate([pad(c, 4) for c in csrc]), rec_c=np.concatenate([pad(c, 4) for c in crec]))
        g = _same(hv, oracle, pic)
        merges += int((g[:, 22] | g[:, 23]).sum())
    assert merges > 0                                # merges win on a real reconstruction


@pytest.mark.gpu
def test_device_call_replays_from_a_graph(hv, oracle):
    from turingcodec_amd.havoc import SAO_PARAMS_DT, SAO_DECISION_DT
    torch = hv.torch
    pic = M.make_picture(777, W=416, H=240, log2=5, bd=10, flags=7, mode="tiled_noisy")
    L, ctus = pic["layout"], T.ctus(pic)
    want, wy, wc, _ = M.decide_picture(oracle, pic)
    sy, sc, ry, rc = hv.up(pic["src_y"]), hv.up(pic["src_c"]), hv.up(pic["rec_y"]), hv.up(pic["rec_c"])
    with torch.cuda.stream(hv.tstream):
        dy, dc = torch.zeros_like(ry), torch.zeros_like(rc)
        d_ctus = torch.from_numpy(ctus.view(np.uint8).reshape(-1)).to(hv.device)
        params = torch.zeros(len(ctus) * SAO_PARAMS_DT.itemsize, dtype=torch.uint8, device=hv.device)
        dec = torch.zeros(len(ctus) * SAO_DECISION_DT.itemsize, dtype=torch.uint8, device=hv.device)
    work, work2 = hv.sao_workspace(len(ctus)), hv.sao_decide_workspace(len(ctus))
    hv.sync()
    sl = (L["stride_y"], L["stride_c"])

    def body():
        hv.sao_estimate_d(pic["bd"], pic["q16"], 3, sy, sc, *sl, ry, rc, *sl, dy, dc, *sl, d_ctus, work, params)
        hv.sao_decide_d(pic["bd"], pic["q16"], 7, sy, sc, *sl, ry, rc, *sl, dy, dc, *sl, d_ctus, M.ctus_x(pic), params, pic["ctx"][0], pic["ctx"][1],
                        work2, dec)
    g = hv.graph_capture(body)
    try:
        for _ in range(2):
            with torch.cuda.stream(hv.tstream):
                dec.zero_()
                dy.zero_()
            hv.graph_launch(g)
            hv.sync()
            got = hv.down(dec, np.uint8).view(np.int32).reshape(-1, M.NREC).astype(np.int64)
            assert np.array_equal(got, want)
            Y, Cb, Cr = T.planes_of(dict(pic, out_y=hv.down(dy, np.uint16), out_c=hv.down(dc, np.uint16)), "out")
            WY, WCb, WCr = T.planes_of(dict(pic, out_y=wy, out_c=wc), "out")
            assert np.array_equal(Y, WY) and np.array_equal(Cb, WCb) and np.array_equal(Cr, WCr)
    finally:
        hv.graph_destroy(g)


@pytest.mark.gpu
@pytest.mark.parametrize("wpp", [0, 4])
def test_device_keeps_the_first_of_a_tie(hv, oracle, wpp):
    """made-up estimate records (test_restatement_keeps_the_first_of_a_tie) given straight to the decision"""
    from turingcodec_amd.havoc import SAO_PARAMS_DT, SAO_DECISION_DT
    torch = hv.torch
    pic, est = _tie_case(oracle)
    flags = pic["flags"] | wpp
    want, _, _, _ = M.decide_picture(oracle, dict(pic, flags=flags), est=(est, pic["rec_y"].copy(), pic["rec_c"].copy()))
    p = np.zeros(len(est), SAO_PARAMS_DT)
    p.view(np.int32).reshape(-1, 32)[:, :24] = est[:, :24]
    L, ctus = pic["layout"], T.ctus(pic)
    sy, sc, ry, rc = hv.up(pic["src_y"]), hv.up(pic["src_c"]), hv.up(pic["rec_y"]), hv.up(pic["rec_c"])
    with torch.cuda.stream(hv.tstream):
        dy, dc = ry.clone(), rc.clone()
        d_ctus = torch.from_numpy(ctus.view(np.uint8).reshape(-1)).to(hv.device)
        params = torch.from_numpy(p.view(np.uint8).reshape(-1).copy()).to(hv.device)
        dec = torch.zeros(len(ctus) * SAO_DECISION_DT.itemsize, dtype=torch.uint8, device=hv.device)
    sl = (L["stride_y"], L["stride_c"])
    hv.sao_decide_d(8, 2, flags, sy, sc, *sl, ry, rc, *sl, dy, dc, *sl, d_ctus, 3, params, pic["ctx"][0], pic["ctx"][1], hv.sao_decide_workspace(6), dec)
    got = hv.down(dec, np.uint8).view(np.int32).reshape(-1, M.NREC).astype(np.int64)
    assert np.array_equal(got, want)
    assert got[1, 25] == 1


@pytest.mark.gpu
def test_device_rejects_bad_arguments(hv):
    from turingcodec_amd.havoc import HavocError
    pic = M.make_picture(1, W=64, H=64, log2=5, bd=8, flags=3)
    with pytest.raises(HavocError, match="reciprocal_lambda_q16"):
        _device(hv, dict(pic, q16=0))
    with pytest.raises(HavocError, match="flags"):
        _device(hv, pic, flags=8)
    L = pic["layout"]
    with pytest.raises(HavocError, match="whole number of rows"):      # 3 CTUs per row given for a table of 2 x 2
        hv.sao_decide(8, pic["q16"], pic["src_y"], pic["src_c"], pic["rec_y"], pic["rec_c"], L["stride_y"], L["stride_c"], T.ctus(pic), 3, 14, 19)
    with pytest.raises(HavocError, match="context states"):
        _device(hv, dict(pic, ctx=(128, 0)))
