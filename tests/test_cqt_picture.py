"""DecisionPicture(cqt=True): the coding quadtree of every CTU decided over the closed coding units of the picture (turing/Search.hpp:808-886) inside the replayed graph
(havoc_mi355x_cqt_decide behind cu_close's two launches).  -m gpu.

The host recomputation is independent of the picture's own table builder: the node table is derived again from the units, the candidates are the downloaded cu_close
records, and the walk is the Python restatement's (tests/cqt_tools.py, pinned against the reference's own writer and Syntax<coding_quadtree>::go by tests/test_cqt.py).
Two sizes: 56 x 56, the smallest picture of the existing picture tests whose width and height are no multiples of 64 -- one CTU whose every level holds forced splits
and deleted quadtrees -- and 416 x 240, 7 x 4 CTUs with a partial last row and column: the context chain over real rows.
"""
import numpy as np
import pytest

import cqt_tools as Q

pytestmark = pytest.mark.gpu

PICTURES = {"56x56": (56, 56, 21), "416x240": (416, 240, 21)}       # width, height, seed
OPTIONS = dict(tree_rates=True, pu_modes=True, cu_close=True)


@pytest.fixture(scope="module")
def hv():
    from turingcodec_amd.havoc import Havoc
    h = Havoc(stream="new")
    yield h
    h.close()


@pytest.fixture(scope="module", params=list(PICTURES))
def pictures(hv, request):
    """the picture with cqt, with cqt=False and as built without any option: three steps each, the third replayed from the graph"""
    from turingcodec_amd.decisions import DecisionPicture
    w, h, seed = PICTURES[request.param]
    out = {}
    for name, options in (("cqt", dict(OPTIONS, cqt=True)), ("off", OPTIONS), ("default", {})):
        dp = DecisionPicture(hv, w, h, 8, 32, seed=seed, threads=8, intra=False, **options)
        for _ in range(3):
            searched = dp.step()
        assert all(dp._graphs.values()) and len(dp._graphs) == 1
        out[name] = (dp, searched)
    return out


def host_case(dp):
    """the inputs of havoc_mi355x_cqt_decide for the picture, made on the host from its units and the downloaded cu_close records"""
    u = dp.units
    node_cu = np.full((dp.cx * dp.cy, 85), -1, np.int32)
    for i in range(len(u)):
        x, y, l = int(u["x0"][i]), int(u["y0"][i]), int(u["log2_size"][i])
        d, z = 6 - l, 0
        for b in range(d):      # the z-order index of the unit's place among the nodes of its depth
            z |= ((x % 64) >> l >> b & 1) << (2 * b) | ((y % 64) >> l >> b & 1) << (2 * b + 1)
        node_cu[(y // 64) * dp.cx + x // 64, Q.first(d) + z] = i
    return dict(width=dp.W, height=dp.H, ctb_log2=6, min_cb_log2=3, flags=Q.WPP, cu_syntax=dp.cu_syntax_states[0], node_cu=node_cu,
                choice=dp.cu_decisions["records"].view(Q.CHOICE_DT))


def test_every_record_is_the_host_recomputation(pictures):
    dp, _ = pictures["cqt"]
    d = dp.cqt_decisions
    assert not d["gave_up"]
    case = host_case(dp)
    assert np.array_equal(d["node_cu"], case["node_cu"])
    want = Q.decide_picture(case)
    assert Q.same(d, want) is None, Q.same(d, want)
    ctus, nodes = d["ctus"], d["nodes"]
    print("CTUs", len(ctus), "decided", int(ctus["decided"].sum()), "coding units", int(ctus["n_cus"].sum()), "coded flags' bits", float(ctus["flag_rate"].sum()) / 65536)
    # today's limit: no 64x64 node has a candidate, so a CTU's root is split without a comparison -- forced by the picture edge or for want of a candidate
    ok = ctus["decided"] == 1
    root = nodes[ok, 0]
    assert (root["choice"] == Q.SPLIT).all() and ((root["flags"] & (Q.MUST_SPLIT | Q.NO_CANDIDATE)) != 0).all() and (root["cost_full"] == -1).all()
    # a CTU is refused exactly when one of its tree units inside the picture has a refused record: its 32x32 (16x16, 8x8) node then has no candidate down to MinCb
    refused_unit = dp.cu_decisions["records"]["outcome"] == Q.REFUSED
    by_ctu = np.bincount(dp.units["ctx_index"][refused_unit], minlength=len(ctus)) > 0
    assert np.array_equal(~ok, by_ctu)
    # the partial last row and column: forced splits and deleted quadtrees, where the picture has them
    if dp.W % 64:
        last = nodes[dp.cx - 1::dp.cx][ok[dp.cx - 1::dp.cx]]
        assert ((last["flags"][:, 0] & Q.MUST_SPLIT) != 0).all() and ((last["choice"] == Q.DELETED).any(1)).all()
    cells = d["depth"]
    assert cells.shape == (8 * dp.cy, 8 * dp.cx) and not cells[dp.H // 8:].any() and not cells[:, dp.W // 8:].any()
    # the snapshots: three bytes moved by the chain, thirteen as the slice's
    assert np.array_equal(d["cu_syntax"][:, 3:], np.tile(dp.cu_syntax_states[0, 3:], (len(ctus), 1)))
    out = dp.results()
    assert len(out) == 3 and out[2]["cqt"] is d and out[2]["cu_close"] is dp.cu_decisions


def test_the_step_itself_is_unchanged(pictures):
    """the launch writes only its own buffers: the picture with cqt leaves the reconstruction, cells, tree decisions and closed units of the same picture with
    cqt=False; the default picture builds nothing of it"""
    (on, r_on), (off, r_off), (default, r_def) = pictures["cqt"], pictures["off"], pictures["default"]
    assert not hasattr(off, "cqt_plan") and not hasattr(default, "cqt_plan") and not hasattr(default, "cu_plan")
    down = lambda dp, t: dp.hv.down(t, dp.dt)

    def picture_area(dp):
        c2, hw, hh = dp.PAD // 2, dp.W // 2, dp.H // 2
        y = down(dp, dp.recon)[:dp.n].reshape(-1, dp.stride)[dp.PAD:dp.PAD + dp.H, dp.PAD:dp.PAD + dp.W]
        c = down(dp, dp.crecon)
        return [y] + [c[k * dp.cpe:k * dp.cpe + dp.cn].reshape(-1, dp.cstride)[c2:c2 + hh, c2:c2 + hw] for k in (0, 1)]

    assert all(np.array_equal(a, b) and a.any() for a, b in zip(picture_area(on), picture_area(off)))
    assert np.array_equal(on.cells.view(np.uint8), off.cells.view(np.uint8))
    assert on.rqt_results.tobytes() == off.rqt_results.tobytes() and on.rqt_tree_results.tobytes() == off.rqt_tree_results.tobytes()
    a, b = on.cu_decisions, off.cu_decisions
    assert all(np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)) for k in a)
    for dp, r in ((on, r_on), (off, r_off)):
        assert np.array_equal(r[0], r_def[0]) and np.array_equal(r[1], r_def[1]) and np.array_equal(down(dp, dp.pred), down(default, default.pred))
    with pytest.raises(ValueError, match="cqt"):
        off.cqt_decisions
    assert len(off.results()) == 3 and "cqt" not in off.results()[2] and len(default.results()) == 2


def test_cqt_is_refused_where_it_is_not_built(hv, pictures):
    from turingcodec_amd.decisions import DecisionPicture
    w, h = pictures["cqt"][0].W, pictures["cqt"][0].H
    for options in (dict(OPTIONS, search_on_device=False), dict(tree_rates=True, pu_modes=True), dict(tree_rates=True), {}):
        with pytest.raises(ValueError):
            DecisionPicture(hv, w, h, 8, 32, seed=21, threads=8, intra=False, cqt=True, **options)
    with pytest.raises(ValueError, match="cu_close"):
        DecisionPicture(hv, w, h, 8, 32, seed=21, threads=8, intra=False, cqt=True)
    with pytest.raises(ValueError):
        pictures["cqt"][0].step_banded(hv)
