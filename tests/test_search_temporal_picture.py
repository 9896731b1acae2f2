"""DecisionPicture(col=..., temporal_mvp=True): the temporal candidates a picture derives from a decided picture's motion store enter its search walk's predictors
(havoc_mi355x_search_temporal), with no host round trip between the two.  -m gpu.

Picture A (POC 8, list 0 -> POC 0, list 1 -> POC 16) runs with unit_trees, cqt, commit, finish and motion, as in tests/test_cqt_motion_picture.py; picture B (POC 4,
list 0 -> POC 0, list 1 -> POC 8 = A) runs with col = A's store -- without temporal_mvp (the candidates ride in the replayed graph, nothing reads them), with it (they
are made before the searches and the walk consumes them), and with it under pu_modes, cu_close and cqt.  136 x 72 and 416 x 240, 8-bit, QP 32, three steps each.
"""
import numpy as np
import pytest

import search_temporal_tools as T
import search_tools as st

pytestmark = pytest.mark.gpu

BASE = dict(tree_rates=True, pu_modes=True, cu_close=True, cqt=True, unit_trees=True, commit=True, finish=True)
QP, MOTION = 32, (8, 0, 16)
COL = dict(col_poc=8, cur_poc=4, target_poc=(0, 8), all_backwards=0, collocated_from_l0=1)
CLOSED = dict(tree_rates=True, pu_modes=True, cu_close=True, cqt=True)


@pytest.fixture(scope="module")
def hv():
    from turingcodec_amd.havoc import Havoc
    h = Havoc(stream="new")
    yield h
    h.close()


def _legacy_outputs(dp):
    """recon, the picture's part of crecon (its lower padding holds the legacy plan's dump block, different from run to run), cells, the loop filter's edge data"""
    c2, c = dp.PAD // 2, dp.hv.down(dp.crecon, dp.dt)
    chroma = np.stack([c[k * dp.cpe:k * dp.cpe + dp.cn].reshape(-1, dp.cstride)[c2:c2 + dp.H // 2, c2:c2 + dp.W // 2] for k in (0, 1)])
    return dict(recon=dp.hv.down(dp.recon, dp.dt), chroma=chroma, cells=np.ascontiguousarray(dp.cells).view(np.uint8), data=dp.hv.down(dp.d_data, np.int8),
                bs=dp.hv.down(dp.d_bs, np.uint8), rqt=np.frombuffer(dp.rqt_results.tobytes(), np.uint8))


def _same(a, b):
    assert set(a) == set(b)
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in a)


def _snapshot(dp, out):
    s = dict(res=out[0].copy(), field=out[1].copy(), bi=dp.bi_results.copy())
    if dp.col is not None:
        s["cands"] = dp.temporal_candidates().copy()
    return s


def _steps(dp):
    """three steps (the third from the graph); what each left behind"""
    shots = [_snapshot(dp, dp.step()) for _ in range(3)]
    assert all(dp._graphs.values()) and len(dp._graphs) == 1
    return shots


@pytest.fixture(scope="module", params=list(T.PICTURES))
def pictures(hv, request):
    from turingcodec_amd.decisions import DecisionPicture
    w, h = T.PICTURES[request.param]
    out = {}
    a = DecisionPicture(hv, w, h, 8, QP, seed=21, threads=8, intra=False, **dict(BASE, motion=MOTION))
    out["a"] = (a, _steps(a))
    a_before = dict(store=hv.down(a.cqt_store, np.uint8).copy(), cells=hv.down(a.cqt_cells, np.uint8).copy(), res=out["a"][1][-1]["res"])
    col = dict(COL, store=a.cqt_store)
    for name, options in (("plain", {}), ("col", dict(col=col)), ("mvp", dict(col=col, temporal_mvp=True)), ("closed_col", dict(CLOSED, col=col)),
                          ("closed_mvp", dict(CLOSED, col=col, temporal_mvp=True))):
        dp = DecisionPicture(hv, w, h, 8, QP, seed=22, threads=8, intra=False, **options)
        out[name] = (dp, _steps(dp))
    out["a_before"] = a_before
    return out


def test_three_steps_are_identical(pictures):
    for name in ("col", "mvp", "closed_mvp"):
        shots = pictures[name][1]
        for s in shots[1:]:
            assert _same(s, shots[0]), name


def test_candidates_are_the_same_records_with_and_without_temporal_mvp(pictures):
    """made inside the graph behind everything (col alone) or before the searches, outside it (temporal_mvp): the same records from the same store"""
    col, mvp = pictures["col"][1][-1]["cands"], pictures["mvp"][1][-1]["cands"]
    assert col.dtype == T.CAND_DT and col.shape == (len(pictures["col"][0].pus), 2) and col.tobytes() == mvp.tobytes()
    assert col["available"].any() and col["mv"].any()
    assert pictures["closed_mvp"][1][-1]["cands"].tobytes() == col.tobytes()


def test_search_with_temporal_mvp_is_the_temporal_walk_over_the_downloaded_candidates(pictures):
    dp, shots = pictures["mvp"]
    case = dict(W=dp.W, H=dp.H, bd=8, planes=dp.host_planes, stride=dp.stride, pus=np.ascontiguousarray(dp.pus), ctu_first=np.ascontiguousarray(dp.ctu_first, np.int32),
                cx=dp.cx, cy=dp.cy, params=dp.params, mvp_rate=dp.mvp_rate)
    res, field, bi, rep = T.Client("oracle").walk(case, shots[-1]["cands"], report=True)
    got = shots[-1]
    assert T.same_records(got["res"], res) and np.array_equal(got["field"], field) and got["bi"].tobytes() == bi.tobytes()
    consumed = int((rep[..., 2:6] != rep[..., 6:10]).any(-1).sum())
    print(dp.W, dp.H, "derivations that consumed the candidate", consumed, "of", rep.shape[0] * 2)
    assert consumed > 0
    # ... and differs from the search without it
    plain = pictures["col"][1][-1]
    differing = sum(a.tobytes() != b.tobytes() for a, b in zip(got["res"], plain["res"]))
    assert differing > 0, "search records that differ between col and col + temporal_mvp: %d" % differing
    assert not np.array_equal(got["field"], plain["field"])


def test_col_alone_is_the_picture_without_col(pictures):
    """without temporal_mvp nothing reads the candidates: search results, refinements, recon, crecon, cells, edge data and tree decisions byte-identical to the picture
    made without col; temporal_launch rides in the one graph"""
    (off, s_off), (on, s_on) = pictures["plain"], pictures["col"]
    assert not hasattr(off, "_d_temporal") and on.temporal_mvp is False
    for k in ("res", "field", "bi"):
        assert s_on[-1][k].tobytes() == s_off[-1][k].tobytes(), k
    assert _same(_legacy_outputs(on), _legacy_outputs(off)) and _legacy_outputs(on)["recon"].any()
    assert len(on._graphs) == 1 and len(off._graphs) == 1


def test_a_is_untouched(pictures, hv):
    a, before = pictures["a"][0], pictures["a_before"]
    assert hv.down(a.cqt_store, np.uint8).tobytes() == before["store"].tobytes() and hv.down(a.cqt_cells, np.uint8).tobytes() == before["cells"].tobytes()
    out = a.step()
    assert np.array_equal(out[0], before["res"]) and hv.down(a.cqt_store, np.uint8).tobytes() == before["store"].tobytes()


def test_downstream_stages_run_over_the_new_results(pictures, hv):
    """pu_modes, cu_close and cqt behind a search with temporal_mvp: the candidate table pu_rate reads holds the new searches' mvd and mvp_flag, and the decisions exist"""
    (dp, shots), (ref, ref_shots) = pictures["closed_mvp"], pictures["closed_col"]
    res = shots[-1]["res"]
    assert res.tobytes() == pictures["mvp"][1][-1]["res"].tobytes()               # the same searches as without the downstream stages
    assert res.tobytes() != ref_shots[-1]["res"].tobytes()
    P = dp._pu_plan()
    for l in (0, 1):
        assert np.array_equal(P["jobs"]["mvd"][P["first"] + l, l], res["mvd"][l::2]) and np.array_equal(P["jobs"]["mvp_flag"][P["first"] + l, l], res["mvp_flag"][l::2])
    assert hv.down(P["d_jobs"], np.uint8).tobytes() == P["jobs"].tobytes()
    changed = int((res["mvd"] != ref_shots[-1]["res"]["mvd"]).any(-1).sum() + (res["mvp_flag"] != ref_shots[-1]["res"]["mvp_flag"]).sum())
    assert changed > 0
    for name in ("pu_decisions", "cu_decisions", "cqt_decisions"):
        got = getattr(dp, name)
        assert got is not None and len(got) > 0, name


def test_refusals(pictures, hv):
    from turingcodec_amd.decisions import DecisionPicture
    a, b = pictures["a"][0], pictures["mvp"][0]
    make = lambda **o: DecisionPicture(hv, a.W, a.H, 8, QP, seed=22, threads=8, intra=False, **o)
    with pytest.raises(ValueError, match="temporal_mvp"):
        make(temporal_mvp=True)
    with pytest.raises(ValueError, match="col"):
        make(temporal_mvp=True, col=dict(COL, store=a.cqt_store, temporal_mvp=True))      # a constructor keyword, not a key of col
    with pytest.raises(ValueError, match="temporal"):
        b.step_banded(hv)
