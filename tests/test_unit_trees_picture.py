"""DecisionPicture(unit_trees=True): every searched unit gets the transform tree of its own winning prediction, is closed with the winner's rate, and the coding
quadtree compares full against split on a picture (turing/Search.hpp:808-886 over :2362-2568 over turing/Reconstruct.cpp:1296-1428), inside the replayed graph.  -m gpu.

The host recomputation takes the DOWNLOADED candidate predictions, levels and SSDs of the unit plan and restates everything above them: the unit prediction planes
(the block of pu_decisions["mode"]), the tree rates (tests/tree_rate_tools.py, (6, 1) included), the decision (tests/unit_tree_tools.decide_units), the prediction's
SSD (numpy), the close (tests/cu_close_tools.py, given the winner's rate and snapshot) and the quadtree (tests/cqt_tools.py).  Two pictures: 136 x 72 -- 2 x 2 CTUs,
one 64x64 unit whole, the last column and row 8 wide / high, so every level there holds forced splits and deleted quadtrees -- and 416 x 240.
"""
import numpy as np
import pytest

import cqt_tools as Q
import cu_close_tools as CC
import tree_rate_tools as TR
import unit_tree_tools as UT

pytestmark = pytest.mark.gpu

PICTURES = {"136x72": (136, 72, 21), "416x240": (416, 240, 21)}       # width, height, seed
BASE = dict(tree_rates=True, pu_modes=True, cu_close=True, cqt=True)


@pytest.fixture(scope="module")
def hv():
    from turingcodec_amd.havoc import Havoc
    h = Havoc(stream="new")
    yield h
    h.close()


@pytest.fixture(scope="module", params=list(PICTURES))
def pictures(hv, request):
    """the picture with unit_trees, the same picture without it and as built without any option: three steps each, the third replayed from the graph"""
    from turingcodec_amd.decisions import DecisionPicture
    w, h, seed = PICTURES[request.param]
    out = {}
    for name, options in (("on", dict(BASE, unit_trees=True)), ("off", BASE), ("default", {})):
        dp = DecisionPicture(hv, w, h, 8, 32, seed=seed, threads=8, intra=False, **options)
        for _ in range(3):
            searched = dp.step()
        assert all(dp._graphs.values()) and len(dp._graphs) == 1
        out[name] = (dp, searched)
    return out


@pytest.fixture(scope="module")
def host(pictures):
    """what the unit plan left on the device, downloaded once: the candidate predictions, the planes, the levels, flags and SSDs of every candidate"""
    dp, _ = pictures["on"]
    hv, P, U = dp.hv, dp.pu_plan, dp.unit_plan
    return dict(cand=[[hv.down(q["d_dst"], dp.dt) for q in g["planes"]] for g in P["groups"]], d=dp.unit_tree_decisions(planes=True),
                levels={s: hv.down(g["level"], np.int16) for s, g in U["sizes"].items()}, clevels={s: hv.down(g["level"], np.int16) for s, g in U["csizes"].items()},
                sizes={s: dict(cbf=hv.down(g["cbf"], np.int32), ssd=hv.down(g["ssd"], np.uint32)) for s, g in U["sizes"].items()},
                csizes={s: dict(cbf=hv.down(g["cbf"], np.int32), ssd=hv.down(g["ssd"], np.uint32)) for s, g in U["csizes"].items()})


def test_units_are_the_searched_units_and_the_planes_hold_the_winners(pictures, host):
    dp, _ = pictures["on"]
    pus, d, mode = dp.pus, host["d"], dp.pu_decisions["mode"]
    u = d["units"]
    assert len(u) == len(pus) and np.array_equal(u["x0"], pus["x0"]) and np.array_equal(u["y0"], pus["y0"]) and np.array_equal(1 << u["log2_size"], pus["w"])
    assert np.array_equal(u["ctx_index"], (pus["y0"] // 64) * dp.cx + pus["x0"] // 64)
    sizes = set(int(v) for v in u["log2_size"])      # (the searched units of a partial CTU go straight to 8x8: the small picture has 64x64 and 8x8 units only)
    assert ({3, 4, 5, 6} == sizes if dp.W == 416 else {3, 6} <= sizes) and (mode >= 0).all() and len(set(mode.tolist())) > 1
    seen = 0
    for g, cand in zip(dp.pu_plan["groups"], host["cand"]):
        for i, p in enumerate(g["sel"]):
            x, y, L, m = int(u["x0"][p]), int(u["y0"][p]), int(u["log2_size"][p]), int(mode[p])
            n, c = 1 << L, 1 << (L - 1)
            assert np.array_equal(d["pred"][6 - L, y:y + n, x:x + n], cand[0][(3 * i + m) * n * n:(3 * i + m + 1) * n * n].reshape(n, n)), p
            for k in (0, 1):
                assert np.array_equal(d["cpred"][6 - L, k, y // 2:y // 2 + c, x // 2:x // 2 + c], cand[1 + k][(3 * i + m) * c * c:(3 * i + m + 1) * c * c].reshape(c, c)), (p, k)
            seen += 1
    assert seen == len(pus)
    first = dp.pu_plan["first"]
    assert np.array_equal(d["unit_cand"], first + mode) and np.array_equal(d["unit_rate"], dp.pu_decisions["rates"][np.arange(len(pus)), mode])


def test_tree_rates_and_decisions_are_the_host_recomputation(pictures, host):
    dp, _ = pictures["on"]
    U, d = dp.unit_plan, host["d"]
    u, n = d["units"], len(d["units"])
    tree_rate, tree_cbf = np.zeros(2 * n, np.int64), np.zeros(2 * n, np.uint32)
    got_rate, got_cbf = d["tree_rate"].reshape(-1), d["tree_cbf"].reshape(-1)
    sizes = set(int(v) for v in u["log2_size"])
    assert set(U["tree_jobs"]) == {(L, depth) for L in sizes for depth in (0, 1) if (L, depth) != (6, 0)} and (6, 1) in U["tree_jobs"]
    for (L, depth), t in U["tree_jobs"].items():
        jobs = t["jobs"]
        r, m, _, _ = TR.walk_jobs(L, depth, host["levels"][t["luma"]], host["clevels"][t["chroma"]], dp.rdoq_states, dp.syntax_states, jobs)
        at = jobs["out_index"]
        assert np.array_equal(got_rate[at], r[at]) and np.array_equal(got_cbf[at], m[at]), (L, depth)
        assert np.array_equal(at, 2 * np.flatnonzero(u["log2_size"] == L) + depth) and (jobs["flags"] == (0 if L == 6 else 1)).all()
        tree_rate[at], tree_cbf[at] = r[at], m[at]
    is64 = u["log2_size"] == 6
    assert (tree_rate > 0).any() and is64.any() and not got_rate[0::2][is64].any() and not got_cbf[0::2][is64].any()      # entry 2 i of a 64x64 unit: nobody's
    want, want_tree = UT.decide_units(u, U["zero_at"], U["one_at"], host["sizes"], host["csizes"], U["chroma_at"], tree_rate, tree_cbf, U["rl_q16"])
    assert d["choice"].tobytes() == want.tobytes() and d["tree_choice"].tobytes() == want_tree.tobytes()
    c = d["choice"]
    assert (c["tried_zero"][is64] == 0).all() and np.array_equal(c["depth"][is64], (tree_cbf[1::2][is64] != 0).astype(np.int32)) and (c["depth"] >= 0).all()
    print("units", n, "| 64x64:", int(is64.sum()), "coded", int(c["depth"][is64].sum()), "| 8..32: untried", int((c["tried_zero"][~is64] == 0).sum()),
          "depth 0", int(((c["depth"] == 0) & (c["tried_zero"] == 1)).sum()), "depth 1", int((c["depth"][~is64] == 1).sum()))


def host_close_case(dp, d):
    """the inputs of havoc_mi355x_cu_close over the searched units, made on the host: the winner's rate and snapshot, the unit plan's records, numpy's SSDs"""
    from turingcodec_amd.havoc import CU_CLOSE_JOB_DT, CU_CLOSE_MIN_CB, PRED_SSD_JOB_DT
    u, n = d["units"], len(d["units"])
    jobs = np.zeros(n, CU_CLOSE_JOB_DT)
    jobs["ctx_index"] = jobs["pu_before_index"] = u["ctx_index"]
    jobs["unit_index"] = jobs["pu_rate_index"] = jobs["pu_after_index"] = np.arange(n)
    jobs["log2_cb_size"], jobs["flags"] = u["log2_size"], np.where(u["log2_size"] == 3, CU_CLOSE_MIN_CB, 0)
    W, H, hw, hh, c2 = dp.W, dp.H, dp.W // 2, dp.H // 2, dp.PAD // 2
    sj = np.zeros(n, PRED_SSD_JOB_DT)
    for i in range(n):
        x, y, plane = int(u["x0"][i]), int(u["y0"][i]), 6 - int(u["log2_size"][i])
        oc = (y // 2 + c2) * dp.cstride + x // 2 + c2
        sj[i]["src_off"] = [(y + dp.PAD) * dp.stride + x + dp.PAD, oc, len(dp.host_chroma[0]) + oc]
        sj[i]["pred_off"] = [plane * W * H + y * W + x, 2 * plane * hw * hh + (y // 2) * hw + x // 2, (2 * plane + 1) * hw * hh + (y // 2) * hw + x // 2]
        sj[i]["log2_size"] = u["log2_size"][i]
    src_c = np.concatenate([dp.host_chroma[0], dp.host_chroma[3]])
    pred_ssd = CC.unit_ssd(dp.host_planes[0], dp.stride, src_c, dp.cstride, d["pred"].reshape(-1), W, d["cpred"].reshape(-1), hw, sj)
    return dict(cu_syntax=dp.cu_syntax_states, pu_before=dp.pu_syntax_states, pu_after=dp.pu_decisions["syntax"], pu_rate=d["unit_rate"], choice=d["choice"],
                tree_choice=d["tree_choice"], tree_rate=d["tree_rate"].reshape(-1).copy(), pred_ssd=pred_ssd, jobs=jobs)


def host_node_table(dp, u):
    node_cu = np.full((dp.cx * dp.cy, 85), -1, np.int32)
    for i in range(len(u)):
        x, y, l = int(u["x0"][i]), int(u["y0"][i]), int(u["log2_size"][i])
        d, z = 6 - l, 0
        for b in range(d):      # the z-order index of the unit's place among the nodes of its depth
            z |= ((x % 64) >> l >> b & 1) << (2 * b) | ((y % 64) >> l >> b & 1) << (2 * b + 1)
        node_cu[(y // 64) * dp.cx + x // 64, Q.first(d) + z] = i
    return node_cu


def test_close_and_quadtree_are_the_host_recomputation_and_live(pictures, host):
    dp, _ = pictures["on"]
    d, cu = host["d"], dp.cu_decisions
    u, n = d["units"], len(d["units"])
    case = host_close_case(dp, d)
    assert np.array_equal(cu["jobs"].view(np.uint8), case["jobs"].view(np.uint8)) and np.array_equal(cu["searched"], np.arange(n))
    assert np.array_equal(cu["pred_ssd"], case["pred_ssd"])
    sl = CC.Slice(1, 5, 1.0 / dp.lam)
    want, cu_syn, pu_syn, why = CC.walk_jobs(case, sl)
    rec = cu["records"]
    assert all(w is None for w in why)
    for k in CC.CHOICE_FIELDS:
        assert np.array_equal(rec[k], want[k]), k
    assert np.array_equal(cu["cu_syntax"], cu_syn) and np.array_equal(cu["pu_syntax"], pu_syn)
    # ---- the quadtree over those records
    q = dp.cqt_decisions
    assert not q["gave_up"]
    qcase = dict(width=dp.W, height=dp.H, ctb_log2=6, min_cb_log2=3, flags=Q.WPP, cu_syntax=dp.cu_syntax_states[0], node_cu=host_node_table(dp, u),
                 choice=rec.view(Q.CHOICE_DT))
    assert np.array_equal(q["node_cu"], qcase["node_cu"])
    wantq = Q.decide_picture(qcase)
    assert Q.same(q, wantq) is None, Q.same(q, wantq)
    # ---- liveness, whatever the content: no unit refused, every CTU decided, every searched unit whose four sub-units were searched is compared
    assert (rec["outcome"] != Q.REFUSED).all()
    ctus, nodes = q["ctus"], q["nodes"]
    assert (ctus["decided"] == 1).all()
    have = {(int(a), int(b), int(c)) for a, b, c in zip(u["x0"], u["y0"], u["log2_size"])}
    by_depth = {0: 0, 1: 0, 2: 0}
    for x, y, l in have:
        h = 1 << (l - 1)
        if l > 3 and all((x + dx, y + dy, l - 1) in have for dx in (0, h) for dy in (0, h)):
            by_depth[6 - l] += 1
    visited = (nodes["choice"] == Q.CU) | (nodes["choice"] == Q.SPLIT)      # (a node nobody visited, or a deleted one, keeps zeroed costs)
    both = visited & (nodes["cost_full"] != -1) & (nodes["cost_split"] != -1)
    got_depth = {k: 0 for k in by_depth}
    for c, k in zip(*np.nonzero(both)):
        got_depth[Q.depth_of(int(k))] += 1
    assert got_depth == by_depth, (got_depth, by_depth)
    if dp.W == 416:      # (the small picture's whole 64x64 units have no searched sub-units on this seed: they stand, NO_SPLIT_CANDIDATE)
        assert by_depth[0] > 0 and by_depth[1] > 0
    else:
        assert ((nodes["flags"][:, 0] & Q.NO_SPLIT_CANDIDATE) != 0).any() and ((nodes["flags"][:, 0] & Q.MUST_SPLIT) != 0).any() and (nodes["choice"] == Q.DELETED).any()
    alone = (nodes["choice"] == Q.CU) & ((nodes["flags"] & Q.NO_SPLIT_CANDIDATE) != 0)
    print("CTUs", len(ctus), "decided", int(ctus["decided"].sum()), "coding units", int(ctus["n_cus"].sum()), "| comparisons per depth", got_depth, ": the unit stood",
          int((both & (nodes["choice"] == Q.CU)).sum()), "the split won", int((both & (nodes["choice"] == Q.SPLIT)).sum()), "| units kept without searched sub-units",
          int(alone.sum()))
    out = dp.results()
    assert len(out) == 3 and out[2]["unit_trees"] is dp.unit_tree_decisions() and out[2]["cqt"] is q


def test_the_step_is_otherwise_unchanged(pictures):
    """with unit_trees the legacy plan still makes recon, crecon, the cells, pred and cpred, the search results and rqt_results / rqt_tree_results of the same picture
    without it; the default picture builds none of the new plans"""
    (on, r_on), (off, r_off), (default, r_def) = pictures["on"], pictures["off"], pictures["default"]
    assert not hasattr(off, "unit_plan") and not hasattr(default, "unit_plan") and not hasattr(default, "pu_plan") and not hasattr(default, "cu_plan")
    down = lambda dp, t: dp.hv.down(t, dp.dt)

    def picture_area(dp):
        c2, hw, hh = dp.PAD // 2, dp.W // 2, dp.H // 2
        y = down(dp, dp.recon)[:dp.n].reshape(-1, dp.stride)[dp.PAD:dp.PAD + dp.H, dp.PAD:dp.PAD + dp.W]
        c = down(dp, dp.crecon)
        return [y] + [c[k * dp.cpe:k * dp.cpe + dp.cn].reshape(-1, dp.cstride)[c2:c2 + hh, c2:c2 + hw] for k in (0, 1)]

    assert all(np.array_equal(a, b) and a.any() for a, b in zip(picture_area(on), picture_area(off)))
    assert np.array_equal(on.cells.view(np.uint8), off.cells.view(np.uint8))
    assert on.rqt_results.tobytes() == off.rqt_results.tobytes() and on.rqt_tree_results.tobytes() == off.rqt_tree_results.tobytes()
    assert np.array_equal(down(on, on.cpred), down(off, off.cpred))
    a, b = on.pu_decisions, off.pu_decisions
    assert all(np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)) for k in a)
    for dp, r in ((on, r_on), (off, r_off)):
        assert np.array_equal(r[0], r_def[0]) and np.array_equal(r[1], r_def[1]) and np.array_equal(dp.bi_results, default.bi_results)
        assert np.array_equal(down(dp, dp.pred), down(default, default.pred))
    with pytest.raises(ValueError, match="unit_trees"):
        off.unit_tree_decisions()
    assert "unit_trees" not in off.results()[2] and len(default.results()) == 2
    # the parent's limit, still there without the option: tree units the search did not visit come back refused and refuse their CTUs
    assert len(off.cu_decisions["records"]) == len(off.units) and len(on.cu_decisions["records"]) == len(on.pus)


def test_unit_trees_are_refused_where_they_are_not_built(hv, pictures):
    from turingcodec_amd.decisions import DecisionPicture
    w, h = pictures["on"][0].W, pictures["on"][0].H
    for options in (dict(pu_modes=True, cu_close=True), dict(tree_rates=True, cu_close=True), dict(tree_rates=True, pu_modes=True), {},
                    dict(tree_rates=True, pu_modes=True, cu_close=True, search_on_device=False)):
        with pytest.raises(ValueError):
            DecisionPicture(hv, w, h, 8, 32, seed=21, threads=8, intra=False, unit_trees=True, **options)
    with pytest.raises(ValueError, match="unit_trees"):
        DecisionPicture(hv, w, h, 8, 32, seed=21, threads=8, intra=False, unit_trees=True, tree_rates=True, pu_modes=True)
    with pytest.raises(ValueError):
        pictures["on"][0].step_banded(hv)
