"""DecisionPicture(cu_close=True): every transform-tree unit of the picture closed as the reference closes an inter coding unit (turing/Search.hpp:2362-2568) inside the
replayed graph: the prediction's SSD in three planes (havoc_mi355x_unit_pred_ssd), then the CU's own CABAC bits and the residual / no-residual decision
(havoc_mi355x_cu_close) over what rqt_decide_tree and pu_rate left on the device.  -m gpu.

The host recomputation is independent of the picture's own table builder: the job records are derived again from the units and the searched units, the tree decisions,
masks and rates are the downloaded ones, the L0 rates and snapshots the Python restatement's from the downloaded candidate records (tests/pu_rate_tools.py), the SSDs
numpy's over the host source and the downloaded prediction, and the close the Python restatement's (tests/cu_close_tools.py, pinned against the reference's own syntax
functions by tests/test_cu_close.py).
"""
import collections

import numpy as np
import pytest

import cu_close_tools as CC
import pu_rate_tools as PR

pytestmark = pytest.mark.gpu

PICTURE = (128, 64)     # two CTUs: two context snapshots; eight tree units of 32x32, each of them a searched unit on this seed
SEED = 18
QP = 32                 # on this seed and QP units are coded and units are left without residual (asserted below)
SLICE = PR.Slice(1, 5, 0, 0, 0)


@pytest.fixture(scope="module")
def hv():
    from turingcodec_amd.havoc import Havoc
    h = Havoc(stream="new")
    yield h
    h.close()


@pytest.fixture(scope="module")
def pictures(hv):
    """the picture with cu_close, with cu_close=False and as built without any option: three steps each, the third replayed from the graph"""
    from turingcodec_amd.decisions import DecisionPicture
    out = {}
    for name, options in (("close", dict(tree_rates=True, pu_modes=True, cu_close=True)), ("off", dict(tree_rates=True, pu_modes=True, cu_close=False)), ("default", {})):
        dp = DecisionPicture(hv, *PICTURE, 8, QP, seed=SEED, threads=8, intra=False, **options)
        for _ in range(3):
            searched = dp.step()
        assert all(dp._graphs.values()) and len(dp._graphs) == 1
        out[name] = (dp, searched)
    return out


def host_case(dp):
    """the inputs of havoc_mi355x_cu_close for the picture's units, made on the host -> (cu_close_tools case, lambda Q16)"""
    from turingcodec_amd.havoc import CU_CLOSE_JOB_DT, CU_CLOSE_MIN_CB, PRED_SSD_JOB_DT
    u, pus, d = dp.units, dp.pus, dp.pu_decisions
    n = len(u)
    # the L0 candidate of the searched unit of the same place and size: its rate and the snapshot it leaves, by the restatement from the CTU's snapshot
    l0 = d["jobs"][:, 0].copy()
    l0["out_index"] = np.arange(len(pus))
    rates, after, why = PR.walk_jobs(l0, SLICE, dp.pu_syntax_states)
    assert all(w is None for w in why) and np.array_equal(rates, d["rates"][:, 0])
    jobs = np.zeros(n, CU_CLOSE_JOB_DT)
    for i in range(n):
        m = np.flatnonzero((pus["x0"] == u["x0"][i]) & (pus["y0"] == u["y0"][i]) & (pus["w"] == 1 << u["log2_size"][i]) & (pus["h"] == pus["w"]))
        ctu = (u["y0"][i] // 64) * dp.cx + u["x0"][i] // 64
        jobs[i]["ctx_index"] = jobs[i]["pu_before_index"] = ctu
        jobs[i]["unit_index"], jobs[i]["log2_cb_size"] = i, u["log2_size"][i]
        jobs[i]["pu_rate_index"], jobs[i]["pu_after_index"] = (m[0], m[0]) if len(m) else (-1, 0)
        jobs[i]["flags"] = CU_CLOSE_MIN_CB if u["log2_size"][i] == 3 else 0
    # the whole-tree rates as tree_rate wrote them: out_index = 2 * unit + depth
    tree_rate = np.zeros(2 * n, np.int64)
    for key, t in dp.rqt_plan["tree_jobs"].items():
        tree_rate[t["jobs"]["out_index"]] = dp.rqt_rates[key]
    # SSD(source, prediction) per plane in numpy
    W, H, hw, hh, c2 = dp.W, dp.H, dp.W // 2, dp.H // 2, dp.PAD // 2
    sj = np.zeros(n, PRED_SSD_JOB_DT)
    for i in range(n):
        x, y = int(u["x0"][i]), int(u["y0"][i])
        oc = (y // 2 + c2) * dp.cstride + x // 2 + c2
        sj[i]["src_off"] = [(y + dp.PAD) * dp.stride + x + dp.PAD, oc, len(dp.host_chroma[0]) + oc]
        sj[i]["pred_off"] = [y * W + x, (y // 2) * hw + x // 2, hw * hh + (y // 2) * hw + x // 2]
        sj[i]["log2_size"] = u["log2_size"][i]
    src_c = np.concatenate([dp.host_chroma[0], dp.host_chroma[3]])
    pred_ssd = CC.unit_ssd(dp.host_planes[0], dp.stride, src_c, dp.cstride, dp.hv.down(dp.pred, dp.dt), W, dp.hv.down(dp.cpred, dp.dt), hw, sj)
    case = dict(cu_syntax=dp.cu_syntax_states, pu_before=dp.pu_syntax_states, pu_after=after, pu_rate=rates, choice=dp.rqt_results, tree_choice=dp.rqt_tree_results,
                tree_rate=tree_rate, pred_ssd=pred_ssd, jobs=jobs)
    return case, int((1.0 / dp.lam) * 65536 + 0.5)


def test_every_units_record_is_the_host_recomputation(pictures):
    dp, _ = pictures["close"]
    d = dp.cu_decisions
    n = len(dp.units)
    assert n == 8 and len(np.unique(dp.units["ctx_index"])) == 2 and len(dp.pus) == 42
    case, lam = host_case(dp)
    # the picture's own records name a unit's L0 candidate by its place among all candidates (pu_plan: unit p's start at first[p]); otherwise byte for byte
    own, first = d["jobs"].copy(), dp.pu_plan["first"]
    assert np.array_equal(own["pu_rate_index"], first[case["jobs"]["pu_rate_index"]]) and np.array_equal(own["pu_after_index"], first[case["jobs"]["pu_after_index"]])
    own["pu_rate_index"], own["pu_after_index"] = case["jobs"]["pu_rate_index"], case["jobs"]["pu_after_index"]
    assert np.array_equal(own.view(np.uint8), case["jobs"].view(np.uint8)) and np.array_equal(d["searched"], case["jobs"]["pu_rate_index"])
    assert np.array_equal(d["pred_ssd"], case["pred_ssd"]), (d["pred_ssd"], case["pred_ssd"])
    sl = CC.Slice(1, 5, 1.0 / dp.lam)
    assert CC.lambda_q16(sl.reciprocal_lambda) == lam
    tags = collections.Counter()
    want, cu, pu, why = CC.walk_jobs(case, sl, tags)
    rec = d["records"]
    print("outcomes", rec["outcome"].tolist(), "have_residual", rec["have_residual"].tolist())
    print("cost_coded", rec["cost_coded"].tolist(), "cost_no_residual", rec["cost_no_residual"].tolist())
    assert all(w is None for w in why)
    for k in CC.CHOICE_FIELDS:
        assert np.array_equal(rec[k], want[k]), (k, rec[k], want[k])
    assert np.array_equal(d["cu_syntax"], cu) and np.array_equal(d["pu_syntax"], pu)
    # the snapshots moved from the CTU's (the reserved and split_cu_flag bytes did not); the record is what rate + lambdaDistortion says
    before = dp.cu_syntax_states[dp.units["ctx_index"]]
    assert (d["cu_syntax"][:, 3:12] != before[:, 3:12]).any(1).all() and np.array_equal(d["cu_syntax"][:, :3], before[:, :3]) and np.array_equal(d["cu_syntax"][:, 12:], before[:, 12:])
    assert np.array_equal(rec["cost"], rec["rate"] + rec["lambda_distortion"]) and (rec["rate"] > 0).all()
    # units are coded and units are left without residual on this seed and QP
    assert {CC.CODED, CC.NO_RESIDUAL} <= set(rec["outcome"].tolist()), rec["outcome"]
    out = dp.results()
    assert len(out) == 3 and out[2]["cu_close"] is d


def test_the_step_itself_is_unchanged(pictures):
    """the two launches write only their own buffers: the picture with cu_close leaves the reconstruction, cells, tree decisions and prediction-unit decisions of the
    same picture with cu_close=False; and the default picture's step is the one a picture built with every option off runs"""
    (close, rc), (off, ro), (default, rd) = pictures["close"], pictures["off"], pictures["default"]
    assert not hasattr(off, "cu_plan") and not hasattr(default, "cu_plan") and not hasattr(default, "pu_plan")
    down = lambda dp, t: dp.hv.down(t, dp.dt)

    def picture_area(dp):
        """the samples of the reconstruction inside the picture, luma, Cb, Cr (the borders hold the dump areas the candidates that lost are written to, in any order)"""
        c2, hw, hh = dp.PAD // 2, dp.W // 2, dp.H // 2
        y = down(dp, dp.recon)[:dp.n].reshape(-1, dp.stride)[dp.PAD:dp.PAD + dp.H, dp.PAD:dp.PAD + dp.W]
        c = down(dp, dp.crecon)
        return [y] + [c[k * dp.cpe:k * dp.cpe + dp.cn].reshape(-1, dp.cstride)[c2:c2 + hh, c2:c2 + hw] for k in (0, 1)]

    assert all(np.array_equal(a, b) and a.any() for a, b in zip(picture_area(close), picture_area(off)))
    assert np.array_equal(close.cells.view(np.uint8), off.cells.view(np.uint8))
    assert close.rqt_results.tobytes() == off.rqt_results.tobytes() and close.rqt_tree_results.tobytes() == off.rqt_tree_results.tobytes()
    a, b = close.pu_decisions, off.pu_decisions
    assert all(np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)) for k in a)
    for dp, r in ((close, rc), (off, ro)):
        assert np.array_equal(r[0], rd[0]) and np.array_equal(r[1], rd[1]) and np.array_equal(dp.bi_results, default.bi_results)
        assert np.array_equal(down(dp, dp.pred), down(default, default.pred))
    with pytest.raises(ValueError, match="cu_close"):
        off.cu_decisions


def test_cu_close_is_refused_where_it_is_not_built(hv, pictures):
    from turingcodec_amd.decisions import DecisionPicture
    for options in (dict(tree_rates=True, pu_modes=True, search_on_device=False), dict(tree_rates=True), dict(pu_modes=True), {}):
        with pytest.raises(ValueError):
            DecisionPicture(hv, *PICTURE, 8, QP, seed=SEED, threads=8, intra=False, cu_close=True, **options)
    with pytest.raises(ValueError, match="cu_close"):
        DecisionPicture(hv, *PICTURE, 8, QP, seed=SEED, threads=8, intra=False, cu_close=True)
    with pytest.raises(ValueError):
        pictures["close"][0].step_banded(hv)
