"""SAO parameter estimation and distortion per CTU (havoc_mi355x_sao_estimate; turing/EncSao.h:286-947).

CPU: the restatement of tests/sao_decision_tools.py against the reference's own functions (tests/sao_rd_shim.cpp, compiled at test time)
on fresh pictures and against their committed outputs (tests/golden/sao_decision_golden.npz); the case generator's branch coverage is
asserted.  GPU: the device call against both, on whole pictures up to 3840x2160, on a real decision step's deblocked output, replayed
from a captured graph, and with each slice flag."""
import os

import numpy as np
import pytest

import reflibs
import sao_decision_tools as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sao_decision_golden.npz")
needs_ref = pytest.mark.skipif(T.reference_dir() is None, reason="reference sources not present (the shim compiles them at test time)")


@pytest.fixture(scope="module")
def oracle():
    return reflibs.Oracle()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _golden_seeds(golden):
    return sorted(int(k[3:]) for k in golden.files if k.startswith("rec"))


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_records_match_the_header():
    import re
    from turingcodec_amd.havoc import SAO_CTU_DT, SAO_PARAMS_DT, SAO_COMPONENT_DT
    text = open(os.path.join(ROOT, "include", "havoc_mi355x.h")).read()
    sizes = dict(re.findall(r"\}\s*(havoc_mi355x_sao_(?:ctu|component|params));\s*/\*\s*(\d+) bytes", text))
    assert sizes == {"havoc_mi355x_sao_ctu": str(SAO_CTU_DT.itemsize), "havoc_mi355x_sao_component": str(SAO_COMPONENT_DT.itemsize),
                     "havoc_mi355x_sao_params": str(SAO_PARAMS_DT.itemsize)}
    assert SAO_PARAMS_DT.fields["dist_sao"][1] == 88 and SAO_PARAMS_DT.fields["ssd_sao"][1] == 96 and SAO_CTU_DT.fields["stat_src_cb"][1] == 48


def test_ctu_table_clips_the_last_column_and_row():
    from turingcodec_amd.havoc import sao_ctu_table, sao_layout
    t = sao_ctu_table(416, 240, 64)
    assert len(t) == 7 * 4
    assert set(t["w"][:7]) == {64, 32} and t["w"][6] == 32 and t["h"][-1] == 48 and (t["h"][:21] == 64).all()
    L = sao_layout(416, 240)
    assert t["src_y"][1] == 8 * L["stride_y"] + 8 + 64 and t["src_cr"][0] == L["size_c"] + t["src_cb"][0]
    assert (t["stat_src_cb"] == t["src_cb"]).all()
    r = sao_ctu_table(416, 240, 64, chroma_stats="reference")
    assert r["stat_src_cb"][8] == (64 // 4 + 4) * L["stride_c"] + 64 // 4 + 4      # CTU (1, 1): chroma (16, 16), not (32, 32)


def test_restatement_matches_golden(oracle, golden):
    seeds = _golden_seeds(golden)
    assert len(seeds) >= 40
    for s in seeds:
        rec, dy, dc = T.decide_picture(oracle, T.make_picture(s), chroma_stats="reference")
        assert np.array_equal(rec[:, :24], golden[f"rec{s}"][:, :24]), s
        assert np.array_equal(dy, golden[f"dst_y{s}"]) and np.array_equal(dc, golden[f"dst_c{s}"]), s


def test_generator_covers_every_branch(oracle):
    tags, n_undefined, always_off, always_on = set(), 0, [], []
    for s in range(3000, 3400):
        pic = T.make_picture(s)
        und = []
        rec, _, _ = T.decide_picture(oracle, pic, tags, undefined=und)
        n_undefined += int(np.array(und).any())
        types = rec[:, [0, 11]]
        if pic["q16"] == 1:
            always_off.append(types)
        elif pic["q16"] == 0x7FFFFFFF:
            always_on.append(types)
    for comp in ("Y", "C"):
        for t in ((0, -1), (1, -1), (2, 0), (2, 1), (2, 2), (2, 3)):
            assert (comp, ("type",) + t) in tags, (comp, t)
        for b in ("band_low", "band_high", "class1_intdiv", "clamp", "tie_class"):
            assert (comp, b) in tags, (comp, b)
    assert {("bd", 8), ("bd", 9), ("bd", 10), "clipped", "ssd_top"} <= tags
    assert n_undefined > 0                               # band position 29 occurs (the device takes band 32 as empty)
    assert (np.concatenate(always_off) == 0).all()       # lambda 65536: SAO never pays
    on = np.concatenate(always_on)
    assert (on != 0).mean() > 0.7                        # lambda 2^-15: SAO pays wherever the statistics hold any error
    # (the branch that turns a chosen type with four zero offsets off, EncSao.h:505, needs lambda <= 0: unreachable with q16 > 0)


@needs_ref
def test_restatement_matches_the_reference_on_fresh_pictures(oracle):
    """>= 2 000 CTUs: every parameter field, both distortions and the filtered planes equal the reference's own functions
    (computeSaoDistortion through the stand-in handle), chroma statistics read where the reference reads them.  CTUs whose band search
    starts at position 29 are left out: the reference reads past its arrays there (undefined)."""
    shim = T.Shim()
    nctus, tags = 0, set()
    for s in range(10000, 11000):
        pic = T.make_picture(s)
        und = []
        a, ay, ac = T.decide_picture(oracle, pic, tags, "reference", und)
        b, by, bc = shim.picture(pic)
        ok = ~np.array(und).any(1)
        assert np.array_equal(a[ok, :24], b[ok, :24]), s
        if ok.all():
            assert np.array_equal(ay, by) and np.array_equal(ac, bc), s
        nctus += int(ok.sum())
    assert nctus >= 2000
    assert {("Y", "class1_intdiv"), ("C", "class1_intdiv"), ("Y", "tie_class"), ("Y", "band_high"), ("C", "band_low")} <= tags


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hv():
    from turingcodec_amd.havoc import Havoc
    return Havoc(stream="new")


def _device(hv, pic, chroma_stats="ctu", flags=None):
    L = pic["layout"]
    return hv.sao_estimate(pic["bd"], pic["q16"], pic["src_y"], pic["src_c"], pic["rec_y"], pic["rec_c"], L["stride_y"], L["stride_c"],
                           T.ctus(pic, chroma_stats), pic["flags"] if flags is None else flags)


def _rows(params):
    return params.view(np.int32).reshape(-1, T.NREC).astype(np.int64)


def _same(hv, oracle, pic, chroma_stats="ctu"):
    want, wy, wc = T.decide_picture(oracle, pic, chroma_stats=chroma_stats)
    got, gy, gc = _device(hv, pic, chroma_stats)
    g = _rows(got)
    g[:, 24:30] = g[:, 24:30] & 0xFFFFFFFF     # the per-plane SSDs are uint32
    bad = np.nonzero((g != want).any(1))[0]
    assert len(bad) == 0, (pic["W"], pic["H"], pic["bd"], bad[:8], g[bad[:1]], want[bad[:1]])
    assert np.array_equal(gy, wy) and np.array_equal(gc, wc)
    return g


@pytest.mark.gpu
def test_device_matches_golden(hv, golden):
    for s in _golden_seeds(golden):
        got, gy, gc = _device(hv, T.make_picture(s), "reference")
        assert np.array_equal(_rows(got)[:, :24], golden[f"rec{s}"][:, :24]), s
        assert np.array_equal(gy, golden[f"dst_y{s}"]) and np.array_equal(gc, golden[f"dst_c{s}"]), s


@pytest.mark.gpu
def test_device_matches_restatement_on_fresh_pictures(hv, oracle):
    for s in range(20000, 20300):
        _same(hv, oracle, T.make_picture(s), "reference" if s % 2 else "ctu")


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(416, 240), (1920, 1080), (3840, 2160)])
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("ctb", [16, 32, 64])
def test_device_whole_picture(hv, oracle, size, bd, ctb):
    W, H = size
    pic = T.make_picture(size[0] + bd + ctb, W=W, H=H, log2=ctb.bit_length() - 1, bd=bd, q16=T.lambda_q16_for_qp(22 + (ctb + bd) % 16))
    g = _same(hv, oracle, pic)
    assert len(g) == ((W + ctb - 1) // ctb) * ((H + ctb - 1) // ctb)


@pytest.mark.gpu
def test_device_on_a_decision_steps_deblocked_output(hv, oracle):
    """the reconstruction of a real 416x240 decision step (deblocked, luma; the step's chroma planes are flat) against its source"""
    from turingcodec_amd.decisions import DecisionPicture
    from turingcodec_amd.havoc import sao_layout
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
    pic = dict(W=W, H=H, log2=5, bd=8, S=1, q16=T.lambda_q16_for_qp(32), flags=3, layout=L,
               src_y=pad(src, 8), rec_y=pad(rec, 8), src_c=np.concatenate([pad(c, 4) for c in csrc]), rec_c=np.concatenate([pad(c, 4) for c in crec]))
    assert not np.array_equal(pic["src_y"], pic["rec_y"])
    g = _same(hv, oracle, pic)
    assert (g[:, 0] != 0).any()                   # SAO pays somewhere on a real reconstruction


@pytest.mark.gpu
def test_device_call_replays_from_a_graph(hv, oracle):
    from turingcodec_amd.havoc import SAO_PARAMS_DT
    torch = hv.torch
    pic = T.make_picture(777, W=416, H=240, log2=6, bd=10)
    L, ctus = pic["layout"], T.ctus(pic)
    want, wy, wc = T.decide_picture(oracle, pic)
    sy, sc, ry, rc = hv.up(pic["src_y"]), hv.up(pic["src_c"]), hv.up(pic["rec_y"]), hv.up(pic["rec_c"])
    with torch.cuda.stream(hv.tstream):
        dy, dc = torch.zeros_like(ry), torch.zeros_like(rc)
        d_ctus = torch.from_numpy(ctus.view(np.uint8).reshape(-1)).to(hv.device)
        params = torch.zeros(len(ctus) * SAO_PARAMS_DT.itemsize, dtype=torch.uint8, device=hv.device)
    work = hv.sao_workspace(len(ctus))
    hv.sync()
    g = hv.graph_capture(lambda: hv.sao_estimate_d(pic["bd"], pic["q16"], 3, sy, sc, L["stride_y"], L["stride_c"], ry, rc, L["stride_y"], L["stride_c"],
                                                   dy, dc, L["stride_y"], L["stride_c"], d_ctus, work, params))
    try:
        for _ in range(2):
            with torch.cuda.stream(hv.tstream):
                params.zero_()
            hv.graph_launch(g)
            hv.sync()
            got = _rows(hv.down(params, np.uint8).view(SAO_PARAMS_DT))
            got[:, 24:30] &= 0xFFFFFFFF
            assert np.array_equal(got, want)
    finally:
        hv.graph_destroy(g)
    Y, Cb, Cr = T.planes_of(dict(pic, out_y=hv.down(dy, np.uint16), out_c=hv.down(dc, np.uint16)), "out")
    WY, WCb, WCr = T.planes_of(dict(pic, out_y=wy, out_c=wc), "out")
    assert np.array_equal(Y, WY) and np.array_equal(Cb, WCb) and np.array_equal(Cr, WCr)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [1, 2, 3])
def test_device_slice_flags(hv, oracle, flags):
    for s in range(30000, 30040):
        pic = T.make_picture(s, flags=flags)
        g = _same(hv, oracle, pic)
        if not flags & 1:
            assert (g[:, :11] == 0).all()
        if not flags & 2:
            assert (g[:, 11:22] == 0).all()


@pytest.mark.gpu
def test_device_rejects_bad_arguments(hv):
    from turingcodec_amd.havoc import HavocError
    pic = T.make_picture(1, W=64, H=64, log2=6, bd=8)
    with pytest.raises(HavocError, match="reciprocal_lambda_q16"):
        _device(hv, dict(pic, q16=0))
    with pytest.raises(HavocError, match="flags"):
        _device(hv, pic, flags=4)
