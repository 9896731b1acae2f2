"""DecisionPicture(pu_modes=True): every searched prediction unit's inter mode -- uni L0, uni L1 or bi -- decided on the device the way go2 decides it
(turing/Search.hpp:1844-1902): the candidates of the search's own records predicted in three planes, measured with the SATD, priced with the reference's CABAC bits
(havoc_mi355x_pu_rate) and compared (havoc_mi355x_pu_decide) inside the replayed graph.  -m gpu.

The host recomputation is independent of the picture's own table builder: the candidates' job records are derived again from the downloaded search records, the
predictions and SATDs are the plain-C oracle's over the host planes, the rates the Python restatement's (tests/pu_rate_tools.py, pinned against the reference's own
syntax functions by tests/test_pu_rate.py) and the decision the numpy form's.
"""
import numpy as np
import pytest

import pu_rate_tools as PR
import reflibs

pytestmark = pytest.mark.gpu

PICTURE = (128, 64)     # two CTUs: two context snapshots, units of 64 to 8
SEED = 18               # on this seed (42 units: 2 of 64, 8 of 32, 24 of 16, 8 of 8) units choose each of L0, L1 and bi (asserted below)
SLICE = PR.Slice(1, 5, 0, 0, 0)


@pytest.fixture(scope="module")
def hv():
    from turingcodec_amd.havoc import Havoc
    h = Havoc(stream="new")
    yield h
    h.close()


@pytest.fixture(scope="module")
def pictures(hv):
    """the picture with pu_modes, with pu_modes=False and as built without the option: three steps each, the third replayed from the graph"""
    from turingcodec_amd.decisions import DecisionPicture
    out = {}
    for name, options in (("modes", dict(pu_modes=True)), ("off", dict(pu_modes=False)), ("default", {})):
        dp = DecisionPicture(hv, *PICTURE, 8, 32, seed=SEED, threads=8, intra=False, **options)
        for _ in range(3):
            searched = dp.step()
        assert all(dp._graphs.values()) and len(dp._graphs) == 1
        out[name] = (dp, searched)
    return out


def _jobs_from_records(dp, res, bi):
    """the three candidates of every unit as PU_RATE_JOB_DT [n, 3], from the search records alone"""
    from turingcodec_amd.havoc import PU_RATE_JOB_DT
    pus = dp.pus
    jobs = np.zeros((len(pus), 3), PU_RATE_JOB_DT)
    for p, pu in enumerate(pus):
        for k in range(3):
            j = jobs[p, k]
            j["ctx_index"] = (pu["y0"] // 64) * dp.cx + pu["x0"] // 64
            j["pred"], j["w"], j["h"], j["cqt_depth"] = k, pu["w"], pu["h"], pu["cqt_depth"]
            for l in (0, 1):
                if k == l:
                    j["mvd"][l], j["mvp_flag"][l] = res[2 * p + l]["mvd"], res[2 * p + l]["mvp_flag"]
                elif k == 2:
                    j["mvd"][l], j["mvp_flag"][l] = bi[2 * p + l]["mvd"], bi[2 * p + l]["mvp_flag"]
    return jobs


def _oracle_satd(dp, oracle, res, bi):
    """measurePuCost's three SATDs of every candidate by the oracle: HavocPredUni / HavocPredBi (8-tap luma, 4-tap chroma) at the records' vectors over the host
    planes, the Hadamard SATD against the source -> int64 [n, 3 candidates, 3 planes]"""
    out = np.zeros((len(dp.pus), 3, 3), np.int64)
    planes = [(dp.host_planes[0], np.concatenate(dp.host_planes[1:3]), len(dp.host_planes[1]), dp.stride, dp.origin, 1, 2, 8),
              (dp.host_chroma[0], np.concatenate(dp.host_chroma[1:3]), len(dp.host_chroma[1]), dp.cstride, dp.corigin, 2, 3, 4),
              (dp.host_chroma[3], np.concatenate(dp.host_chroma[4:6]), len(dp.host_chroma[4]), dp.cstride, dp.corigin, 2, 3, 4)]
    for p, pu in enumerate(dp.pus):
        for c, (src, refs, second, stride, origin, div, sh, taps) in enumerate(planes):
            w, h = int(pu["w"]) // div, int(pu["h"]) // div
            here = origin + (int(pu["y0"]) // div) * stride + int(pu["x0"]) // div
            dst = np.zeros(w * h, src.dtype)
            at = lambda mv, l: l * second + here + (int(mv[1]) >> sh) * stride + (int(mv[0]) >> sh)
            fr = (1 << sh) - 1
            for k in range(3):
                if k < 2:
                    mv = res[2 * p + k]["mv"]
                    oracle.pred_uni(dst, 0, w, refs, at(mv, k), stride, w, h, int(mv[0]) & fr, int(mv[1]) & fr, dp.bd, taps)
                else:
                    m0, m1 = bi[2 * p]["mv"], bi[2 * p + 1]["mv"]
                    oracle.pred_bi(dst, 0, w, refs, at(m0, 0), at(m1, 1), stride, w, h, int(m0[0]) & fr, int(m0[1]) & fr, int(m1[0]) & fr, int(m1[1]) & fr, dp.bd, taps)
                out[p, k, c] = oracle.pu_satd(src, here, stride, dst, 0, w, w, h)
    return out


def test_every_units_mode_is_the_host_recomputation(pictures):
    dp, (res, field, _) = pictures["modes"]
    bi, d = dp.bi_results, dp.pu_decisions
    n = len(dp.pus)
    assert n >= 8 and {int(w) for w in dp.pus["w"]} >= {64, 32, 16, 8} and len(np.unique((dp.pus["y0"] // 64) * dp.cx + dp.pus["x0"] // 64)) == 2
    # ---- the job records: the search's own records, field by field
    jobs = _jobs_from_records(dp, res, bi)
    assert np.array_equal(np.sort(d["jobs"]["out_index"].ravel()), np.arange(3 * n))
    jobs["out_index"] = d["jobs"]["out_index"]
    assert np.array_equal(d["jobs"].reshape(-1).view(np.uint8), jobs.reshape(-1).view(np.uint8))
    assert (np.abs(jobs["mvd"]).reshape(n, -1).max(1) > 0).any() and jobs["mvp_flag"].any()
    # ---- the SATDs: the oracle's predictions at the records' vectors against the source
    satd = _oracle_satd(dp, reflibs.Oracle(), res, bi)
    assert np.array_equal(d["satd"], satd), np.argwhere(d["satd"] != satd)[:8]
    # ---- the rates and snapshots: the restatement from the CTU's snapshot; the decision: the numpy form
    flat = jobs.reshape(-1).copy()
    flat["out_index"] = np.arange(3 * n)
    rates, after, why = PR.walk_jobs(flat, SLICE, dp.pu_syntax_states)
    assert all(w is None for w in why) and np.array_equal(d["rates"], rates.reshape(n, 3))
    lam = PR.lambda_q16(float(dp.params.reciprocal_sqrt_lambda))
    first, count = 3 * np.arange(n), np.full(n, 3)
    cost, best, best_cost, best_syntax = PR.pu_decide(first, count, rates, d["satd"][:, :, 0].ravel(), d["satd"][:, :, 1].ravel(), d["satd"][:, :, 2].ravel(), lam, after)
    assert np.array_equal(d["costs"], cost.reshape(n, 3)) and np.array_equal(d["mode"], best) and np.array_equal(d["cost"], best_cost)
    assert np.array_equal(d["syntax"], best_syntax)
    assert np.array_equal(d["cost"], d["costs"].min(1)) and (d["costs"] > 0).all()
    # the winner's snapshot moved from its CTU's, the reserved bytes did not
    before = dp.pu_syntax_states[(dp.pus["y0"] // 64) * dp.cx + dp.pus["x0"] // 64]
    assert (d["syntax"][:, :12] != before[:, :12]).any(1).all() and np.array_equal(d["syntax"][:, 12:], before[:, 12:])
    # every mode is chosen somewhere on this seed
    assert set(d["mode"].tolist()) == {0, 1, 2}, np.bincount(d["mode"], minlength=3)
    out = dp.results()
    assert len(out) == 3 and out[2]["pu_modes"] is d


def test_default_step_is_unchanged(pictures):
    """pu_modes=False launches what a picture built without the option launches, and the option itself writes nothing the default step reads: the three pictures
    leave the same transform results, reconstruction, merge decisions and search records"""
    (modes, rm), (off, ro), (default, rd) = pictures["modes"], pictures["off"], pictures["default"]
    assert len(off.results()) == 2 and len(default.results()) == 2 and not hasattr(off, "pu_plan") and not hasattr(default, "pu_plan")
    for dp, r in ((off, ro), (modes, rm)):
        got, want = dp.results(), default.results()
        for a, b in zip(got[0], want[0]):
            assert a["log2"] == b["log2"] and all(np.array_equal(a[k], b[k]) for k in ("coef", "level", "cbf", "ssd"))
        assert np.array_equal(got[1], want[1])
        assert all(np.array_equal(dp.merge[k], default.merge[k]) for k in ("vectors", "satd", "cost", "best"))
        assert np.array_equal(r[0], rd[0]) and np.array_equal(r[1], rd[1]) and np.array_equal(dp.bi_results, default.bi_results)
        assert np.array_equal(dp.hv.down(dp.pred, dp.dt), default.hv.down(default.pred, default.dt))
        assert np.array_equal(dp.hv.down(dp.cpred, dp.dt), default.hv.down(default.cpred, default.dt))


def test_pu_modes_are_refused_where_they_are_not_built(hv, pictures):
    from turingcodec_amd.decisions import DecisionPicture
    with pytest.raises(ValueError, match="pu_modes"):
        DecisionPicture(hv, *PICTURE, 8, 32, seed=SEED, threads=8, intra=False, pu_modes=True, search_on_device=False)
    with pytest.raises(ValueError, match="pu_modes"):
        pictures["modes"][0].step_banded(hv)
