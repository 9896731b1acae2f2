"""The two primitives between the searched units and their transform trees: havoc_mi355x_rqt_decide_units -- the three-plane tree decision for units that overlap
one another, 64x64 units with their inferred split included, without final job records -- and havoc_mi355x_unit_pred_select -- the winning candidate's prediction
of every unit into unit prediction planes, with the winner's rate.

CPU (-m "not gpu"): the numpy restatement of the decision (tests/unit_tree_tools.decide_units) against search/tu_decision.hpp's decideRqt through
tests/unit_decide_client.cpp on made units of 8 .. 64; the library surface.  GPU (-m gpu): the kernels against numpy on made cases, and their contracts.
"""
import os

import numpy as np
import pytest

import tree_rate_tools as TR
import unit_tree_tools as UT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_numpy_decide_units_is_tu_decision_hpp():
    """decide_units against decideRqt with the unit's own size: the inferred split is reached for 64x64 units only, where nothing of depth 0 is asked for"""
    client = UT.UnitDecisionClient()
    T = UT.random_units(5, 400)
    units, tree_cbf = T[0], T[7]
    is64 = units["log2_size"] == 6
    assert {3, 4, 5, 6} == set(int(v) for v in units["log2_size"]) and is64.sum() > 40
    for rl in (1, 40000, 1234567):
        rec, tree = UT.decide_units(*T, rl)
        want = client.decide(UT.unit_client_rows(*T), rl)
        assert np.array_equal(rec["depth"], want[:, 0]) and np.array_equal(rec["tried_zero"], want[:, 1])
        assert np.array_equal(rec["cost_zero"], want[:, 2]) and np.array_equal(rec["cost_one"], want[:, 3])
        assert np.array_equal(want[:, 4], rec["tried_zero"]) and np.array_equal(want[:, 5], rec["tried_zero"])      # depth 0 is evaluated only when it is tried
        assert (want[is64, 4] == 0).all() and (want[is64, 1] == 0).all()
        UT.made_units_hold(rec, tree)
    coded64 = is64 & (tree_cbf[1::2] != 0)
    assert (rec["depth"][coded64] == 1).all() and (rec["depth"][is64 & ~coded64] == 0).all() and coded64.sum() > 10 and (is64 & ~coded64).sum() > 3
    chroma_only64 = coded64 & ((tree_cbf[1::2] & 0xf) == 0)
    assert chroma_only64.sum() > 3
    small = ~is64
    assert (rec["depth"][small] == 1).any() and ((rec["depth"][small] == 0) & (rec["tried_zero"][small] == 1)).any() and (rec["tried_zero"][small] == 0).any()


def test_units_of_8_to_32_are_decide_tree():
    """on trees of 8 .. 32 decide_units IS tree_rate_tools.decide_tree"""
    T = TR.random_trees(9, 120)
    a, b = UT.decide_units(*T, 40000), TR.decide_tree(*T, 40000)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_library_surface():
    from turingcodec_amd import havoc
    L, names = havoc._load()
    assert L.havoc_mi355x_rqt_decide_units and L.havoc_mi355x_unit_pred_select and {"rqt_decide_units", "unit_pred_select"} <= set(names)
    assert havoc.PRED_SELECT_JOB_DT.itemsize == 32 and havoc.PRED_SELECT_JOB_DT.fields["log2_size"][1] == 24 and havoc.PRED_SELECT_JOB_DT.fields["unit"][1] == 28
    header = open(os.path.join(ROOT, "include", "havoc_mi355x.h")).read()
    for name in ("havoc_mi355x_rqt_decide_units(", "havoc_mi355x_unit_pred_select(", "} havoc_mi355x_pred_select_job;     /* sizeof: 32 */", "(6, 1) is accepted"):
        assert name in header, name


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def hv():
    from turingcodec_amd.havoc import Havoc
    h = Havoc(stream="new")
    yield h
    h.close()


def _tables(hv, sizes, csizes, with_jobs):
    """-> (the two uint64 [4, 5] tables, the tensors they point to, {(which, log2): the d_final tensor}); with_jobs False: d_stats, d_jobs and d_final are NULL"""
    tables, keep, fins = [np.zeros((4, 5), np.uint64), np.zeros((4, 5), np.uint64)], [], {}
    for which, group in enumerate((sizes, csizes)):
        for s, z in group.items():
            m = len(z["cbf"])
            if not m:
                continue
            d = [hv.up(z["cbf"]), hv.up(z["ssd"]), None, None, None]
            if with_jobs:
                jobs = np.stack([np.arange(m) * 7, np.arange(m) * 11 + 1, np.arange(m) * 13 + 2, np.full(m, -5)], 1).astype(np.int32)
                d[3], d[4] = hv.up(jobs), hv.zeros(4 * m, np.int32)
                fins[which, s] = d[4]
            keep.append(d)
            tables[which][s - 2] = [t.data_ptr() if t is not None else 0 for t in d]
    return tables, keep, fins


def _decide_units(hv, T, rl, with_jobs=False):
    import torch
    from turingcodec_amd.decisions import RQT_RESULT_DT
    from turingcodec_amd.havoc import RQT_TREE_RESULT_DT
    units, zero_at, one_at, sizes, csizes, chroma_at, tree_rate, tree_cbf = T
    tables, keep, fins = _tables(hv, sizes, csizes, with_jobs)
    with torch.cuda.stream(hv.tstream):
        d_rate = torch.from_numpy(np.ascontiguousarray(tree_rate, np.int64)).to(hv.device)
    out, tree_out = hv.zeros(len(units) * 26, np.int32), hv.zeros(len(units) * 4, np.int32)
    hv.rqt_decide_units_d(hv.up(np.ascontiguousarray(units).view(np.int32)).view(-1, 4), hv.up(zero_at), hv.up(one_at), tables[0], tables[1],
                          hv.up(np.ascontiguousarray(chroma_at).view(np.int32)), d_rate, hv.up(tree_cbf), rl, out, tree_out)
    finals = {k: hv.down(f, np.int32).copy() for k, f in fins.items()}
    return hv.down(out, np.int32).view(RQT_RESULT_DT).copy(), hv.down(tree_out, np.int32).view(RQT_TREE_RESULT_DT).copy(), finals


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_decide_units_is_the_numpy_restatement(hv, n):
    """random trees of 8 .. 64 (a workgroup decides 256 units), the made cases among them, with NULL d_stats / d_jobs / d_final"""
    T = UT.random_units(40 + n, n)
    got, got_tree, _ = _decide_units(hv, T, 40000)
    want, want_tree = UT.decide_units(*T, 40000)
    assert got.tobytes() == want.tobytes() and got_tree.tobytes() == want_tree.tobytes()
    if n >= UT.MADE_UNITS:
        UT.made_units_hold(got, got_tree)
        is64 = T[0]["log2_size"] == 6
        assert is64.sum() > 30 and (got["tried_zero"][is64] == 0).all() and (got["depth"][is64] == 1).any() and (got["depth"][is64] == 0).any()


@pytest.mark.gpu
def test_decide_units_equals_decide_tree_on_units_of_8_to_32_and_writes_no_final_record(hv):
    """the same tables through both entry points: the records byte for byte; rqt_decide_tree writes every final job record, rqt_decide_units none"""
    import torch
    from turingcodec_amd.decisions import RQT_RESULT_DT
    from turingcodec_amd.havoc import RQT_TREE_RESULT_DT
    T = TR.random_trees(77, 300)
    units, zero_at, one_at, sizes, csizes, chroma_at, tree_rate, tree_cbf = T
    rl = 40000
    got, got_tree, finals = _decide_units(hv, T, rl, with_jobs=True)
    assert finals and all((f == 0).all() for f in finals.values())      # given, and never touched
    tables, keep, fins = _tables(hv, sizes, csizes, True)
    with torch.cuda.stream(hv.tstream):
        d_rate = torch.from_numpy(np.ascontiguousarray(tree_rate, np.int64)).to(hv.device)
    out, tree_out = hv.zeros(len(units) * 26, np.int32), hv.zeros(len(units) * 4, np.int32)
    hv.rqt_decide_tree_d(hv.up(np.ascontiguousarray(units).view(np.int32)).view(-1, 4), hv.up(zero_at), hv.up(one_at), tables[0], tables[1],
                         hv.up(np.ascontiguousarray(chroma_at).view(np.int32)), d_rate, hv.up(tree_cbf), 1000, 512, 99, 5000, 9000, 256, 77, rl, out, tree_out)
    ref, ref_tree = hv.down(out, np.int32).view(RQT_RESULT_DT), hv.down(tree_out, np.int32).view(RQT_TREE_RESULT_DT)
    assert got.tobytes() == ref.tobytes() and got_tree.tobytes() == ref_tree.tobytes()
    assert all((hv.down(f, np.int32) != 0).any() for f in fins.values())
    want, want_tree = TR.decide_tree(*T, rl)
    assert got.tobytes() == want.tobytes() and got_tree.tobytes() == want_tree.tobytes()


@pytest.mark.gpu
def test_decide_tree_still_refuses_size_6_and_decide_units_other_sizes(hv):
    import torch
    from turingcodec_amd.decisions import RQT_RESULT_DT
    from turingcodec_amd.havoc import HavocError
    T = UT.random_units(3, 12)
    units, zero_at, one_at, sizes, csizes, chroma_at, tree_rate, tree_cbf = T
    bad = units.copy()
    bad["log2_size"][5], bad["log2_size"][7] = 7, 2
    got, got_tree, _ = _decide_units(hv, (bad,) + T[1:], 5)
    want, want_tree = UT.decide_units(*T, 5)
    keep = [i for i in range(12) if i not in (5, 7)]
    assert (got["depth"][[5, 7]] == -1).all() and got[keep].tobytes() == want[keep].tobytes() and got_tree[keep].tobytes() == want_tree[keep].tobytes()
    assert not got_tree[[5, 7]].view(np.int32).any()
    # the sibling: a 64x64 unit is refused with depth -1 as before (its tables are never read)
    only64 = units[units["log2_size"] == 6][:2].copy()
    tables, keep_alive, _ = _tables(hv, sizes, csizes, True)
    d = hv.zeros(64, np.int32)
    with torch.cuda.stream(hv.tstream):
        d_rate = torch.zeros(8, dtype=torch.int64, device=hv.device)
    out, tree_out = hv.zeros(2 * 26, np.int32), hv.zeros(2 * 4, np.int32)
    hv.rqt_decide_tree_d(hv.up(np.ascontiguousarray(only64).view(np.int32)).view(-1, 4), d, d, tables[0], tables[1], d, d_rate, d, 1000, 512, 99, 5000, 9000, 256, 77, 5,
                         out, tree_out)
    assert (hv.down(out, np.int32).view(RQT_RESULT_DT)["depth"] == -1).all()
    # EINVAL: the sibling's rules, minus the dropped arguments
    z = np.zeros((4, 5), np.uint64)
    for kwargs in (dict(rl=-1), dict(chroma_at=None), dict(out=None)):
        with pytest.raises(HavocError):
            hv.rqt_decide_units_d(d.view(-1, 4)[:8], d, d, z, z, kwargs.get("chroma_at", d), d_rate, d, kwargs.get("rl", 5), kwargs.get("out", d), d)
    with pytest.raises(HavocError, match="chroma size table"):
        c = z.copy()
        c[0, 0] = d.data_ptr()
        hv.rqt_decide_units_d(d.view(-1, 4)[:8], d, d, z, c, d, d_rate, d, 5, d, d)
    with pytest.raises(HavocError, match="size table"):
        c = z.copy()
        c[1, 1] = d.data_ptr()
        hv.rqt_decide_units_d(d.view(-1, 4)[:8], d, d, c, z, d, d_rate, d, 5, d, d)


@pytest.mark.gpu
@pytest.mark.parametrize("bit_depth", [8, 10])
def test_unit_pred_select(hv, bit_depth):
    """units of all four sizes, best 0, 1, 2 and -1 at each, blocks of different sizes overlapping in picture position but not in plane, sentinel-filled planes:
    every winner's block arrives, every other sample is still the sentinel, unit_rate / unit_cand are the winner's, a unit without a winner writes nothing"""
    c = UT.select_case(11 + bit_depth, bit_depth)
    assert {3, 4, 5, 6} == {L for L, _, _ in c["place"]}
    got_y, got_c, unit_rate, unit_cand = hv.unit_pred_select(bit_depth, c["cand_y"], c["cand_c"], c["dst_y"], c["stride"], c["dst_c"], c["cstride"], c["first"], c["best"],
                                                             c["rate"], c["jobs"])
    assert np.array_equal(got_y, c["want_y"]) and np.array_equal(got_c, c["want_c"])
    assert np.array_equal(unit_rate, c["unit_rate"]) and np.array_equal(unit_cand, c["unit_cand"])
    none = c["best"] < 0
    assert none.sum() >= 4 and (unit_rate[none] == -1).all() and (unit_cand[none] == -1).all() and (unit_rate[~none] >= 0).all()
    written_y, written_c = (c["want_y"] != c["sentinel"]).sum(), (c["want_c"] != c["sentinel"]).sum()
    assert 0 < written_y < c["want_y"].size // 2 and 0 < written_c < c["want_c"].size // 2      # most of every plane is sentinel, and stays so
    # jobs in another order, and a subset of them: the units not named keep what they had
    half = c["jobs"][::2][::-1].copy()
    got_y2, got_c2, unit_rate2, unit_cand2 = hv.unit_pred_select(bit_depth, c["cand_y"], c["cand_c"], c["dst_y"], c["stride"], c["dst_c"], c["cstride"], c["first"],
                                                                 c["best"], c["rate"], half)
    named = np.zeros(len(c["best"]), bool)
    named[half["unit"]] = True
    assert np.array_equal(unit_rate2[named], c["unit_rate"][named]) and (unit_rate2[~named] == 0).all() and (unit_cand2[~named] == 0).all()
    assert ((got_y2 == c["want_y"]) | (got_y2 == c["sentinel"])).all() and (got_y2 != c["sentinel"]).sum() < written_y


@pytest.mark.gpu
def test_unit_pred_select_contract(hv):
    """the inputs are never written; refusals; a captured graph replays with another winner in place"""
    import torch
    from turingcodec_amd.havoc import HavocError, PRED_SELECT_JOB_DT
    c = UT.select_case(5, 8)
    t = torch
    with t.cuda.stream(hv.tstream):
        up = lambda a: t.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(hv.device)
        cand_y, cand_c, dst_y, dst_c = up(c["cand_y"]), up(c["cand_c"]), up(c["dst_y"]), up(c["dst_c"])
        first, best, rate, jobs = up(c["first"]), up(c["best"]), up(c["rate"]), up(c["jobs"].view(np.uint8))
        unit_rate = t.zeros(len(c["best"]), dtype=t.int64, device=hv.device)
        unit_cand = t.zeros(len(c["best"]), dtype=t.int32, device=hv.device)
    args = [8, cand_y, cand_c, dst_y, c["stride"], dst_c, c["cstride"], first, best, rate, jobs, unit_rate, unit_cand]
    graph = hv.graph_capture(lambda: hv.unit_pred_select_d(*args))
    hv.graph_launch(graph)
    assert np.array_equal(hv.down(dst_y, np.uint8), c["want_y"]) and np.array_equal(hv.down(dst_c, np.uint8), c["want_c"])
    assert np.array_equal(hv.down(unit_rate, np.int64), c["unit_rate"])
    for tensor, a in ((cand_y, c["cand_y"]), (cand_c, c["cand_c"]), (first, c["first"]), (best, c["best"]), (rate, c["rate"]), (jobs, c["jobs"])):
        assert hv.down(tensor, np.uint8).tobytes() == np.ascontiguousarray(a).tobytes()
    # replay: every unit's winner moved on by one (-1 -> 0 -> 1 -> 2 -> -1), the planes reset to the sentinel
    best2 = ((c["best"] + 2) % 4 - 1).astype(np.int32)
    with t.cuda.stream(hv.tstream):
        best.copy_(t.from_numpy(best2.view(np.uint8).copy()))
        dst_y.fill_(c["sentinel"])
        dst_c.fill_(c["sentinel"])
    hv.graph_launch(graph)
    cand2 = hv.down(unit_cand, np.int32)
    assert np.array_equal(cand2, np.where(best2 >= 0, c["first"] + best2, -1))
    got_y = hv.down(dst_y, np.uint8)
    for k, job in enumerate(c["jobs"]):
        n, b = 1 << int(job["log2_size"]), int(best2[k])
        rows = int(job["dst_off"][0]) + np.arange(n)[:, None] * c["stride"] + np.arange(n)
        if b < 0:
            assert (got_y[rows] == c["sentinel"]).all()
        else:
            assert np.array_equal(got_y[rows], c["cand_y"][int(job["cand_off"][0]) + b * n * n:int(job["cand_off"][0]) + (b + 1) * n * n].reshape(n, n)), k
    hv.graph_destroy(graph)
    for k in (1, 2, 3, 5, 7, 8, 9, 11, 12):
        bad = list(args)
        bad[k] = None
        with pytest.raises(HavocError, match="null"):
            hv.unit_pred_select_d(*bad)
    for k, v, what in ((0, 7, "bit_depth"), (4, 0, "stride"), (6, -1, "stride")):
        bad = list(args)
        bad[k] = v
        with pytest.raises(HavocError, match=what):
            hv.unit_pred_select_d(*bad)
    bad = list(args)
    bad[3] = cand_y
    with pytest.raises(HavocError, match="input"):
        hv.unit_pred_select_d(*bad)
    assert PRED_SELECT_JOB_DT.itemsize == 32
