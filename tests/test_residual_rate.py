"""The CABAC rate of residual_coding per transform block (havoc_mi355x_residual_rate) and the transform-tree decision that uses it
(havoc_mi355x_rqt_decide_rated, DecisionPicture(residual_rates=True)).

CPU (-m "not gpu"): the plain-Python restatement tests/residual_rate_tools.walk_block against (a) the reference's own CodedData::storeResidual +
EncodeResidual::inner<EstimateRate> (tests/residual_rate_shim.cpp, compiled at test time where the reference sources are) on fresh blocks and (b) the committed
outputs of that shim (tests/golden/residual_rate_golden.npz); the branches the golden blocks reach; the library's exports; the numpy decideRqt against
tu_decision.hpp's.  GPU (-m gpu): the kernel against the golden file and the restatement -- every rate, all 128 state bytes after every job -- its contract
(untouched memory, refusals, graph replay), the rated decision against the stand-in path and the numpy restatement, and the picture step.
"""
import collections
import os

import numpy as np
import pytest

import reflibs
import residual_rate_tools as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "residual_rate_golden.npz")
needs_ref = pytest.mark.skipif(R.reference_dir() is None, reason="reference sources not present (the shim compiles them at test time)")
SIZES = [2, 3, 4, 5]


@pytest.fixture(scope="module")
def oracle():
    return reflibs.Oracle()


@pytest.fixture(scope="module")
def golden():
    from turingcodec_amd.havoc import RESIDUAL_RATE_JOB_DT
    g = np.load(GOLDEN)
    return {log2: dict(levels=g[f"l{log2}.levels"], states=g[f"l{log2}.states"], jobs=g[f"l{log2}.jobs"].copy().view(RESIDUAL_RATE_JOB_DT).reshape(-1),
                       rates=g[f"l{log2}.rates"], after=g[f"l{log2}.after"]) for log2 in SIZES}


@pytest.fixture(scope="module")
def shim():
    return R.Shim()


@pytest.fixture(scope="module")
def restated(golden):
    """the restatement over the golden blocks, computed once: {log2: (rates, states after, branch counters)}"""
    out = {}
    for log2, g in golden.items():
        tags = collections.Counter()
        rates, after = R.walk_jobs(log2, g["levels"], g["states"], g["jobs"], tags)
        out[log2] = (rates, after, tags)
    return out


# ------------------------------------------------------------------------------------------------------------------ CPU
@needs_ref
@pytest.mark.parametrize("log2", SIZES)
def test_restatement_matches_the_reference_on_fresh_blocks(oracle, shim, log2):
    """about 300 RDOQ blocks per size the golden file has not seen, plus the hand-made ones: the rate of every block and all 128 state bytes after every job"""
    levels, states, jobs = R.make_cases(oracle, 77 + log2, log2, 300)
    got, got_after = R.walk_jobs(log2, levels, states, jobs)
    want, want_after = shim.walk_jobs(log2, levels, states, jobs)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert np.array_equal(got_after, want_after)
    assert (want > 0).sum() > 200 and (want == 0).any() and (want_after != states[jobs["ctx_index"]]).any()


@pytest.mark.parametrize("log2", SIZES)
def test_restatement_matches_golden(golden, restated, log2):
    g, (rates, after, _) = golden[log2], restated[log2]
    assert len(g["jobs"]) >= 257
    assert np.array_equal(rates, g["rates"]) and np.array_equal(after, g["after"])
    # bytes outside the residual contexts pass through
    other = np.setdiff1d(np.arange(128), R.RESIDUAL_BYTES)
    assert np.array_equal(after[:, other], g["states"][g["jobs"]["ctx_index"]][:, other])


@pytest.mark.parametrize("log2", SIZES)
def test_golden_blocks_reach_every_branch(restated, log2):
    tags = restated[log2][2]
    missing = [k for k in R.required_tags(log2) if not tags[k]]
    assert not missing, missing


def test_library_exports_the_entry_points():
    from turingcodec_amd import havoc
    L, _ = havoc._load()
    assert L.havoc_mi355x_residual_rate and L.havoc_mi355x_rqt_decide_rated
    assert havoc.RESIDUAL_RATE_JOB_DT.itemsize == 32


def _random_trees(seed, n):
    """n units of 8x8 .. 32x32 with random candidate outcomes, laid out as DecisionPicture._rqt_plan lays them out"""
    from turingcodec_amd.decisions import RQT_CU_DT
    rng = np.random.default_rng(seed)
    units = np.zeros(n, RQT_CU_DT)
    units["log2_size"] = rng.integers(3, 6, n)
    units["x0"], units["y0"] = 32 * (np.arange(n) % 8), 32 * (np.arange(n) // 8)
    count = {s: 0 for s in SIZES}
    zero_at, one_at = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i, L in enumerate(units["log2_size"]):
        zero_at[i], one_at[i] = count[L], count[L - 1]
        count[L] += 1
        count[L - 1] += 4
    sizes = {}
    for s, m in count.items():
        cbf = rng.integers(0, 40, m) * (rng.random(m) < 0.6)
        nonzero = np.where(cbf != 0, rng.integers(1, 30, m), 0)
        sizes[s] = dict(cbf=cbf.astype(np.int32), ssd=rng.integers(0, 60000, m).astype(np.uint32), nonzero=nonzero.astype(np.int32),
                        sum_abs=(nonzero * rng.integers(1, 4, m)).astype(np.int32))
    return units, zero_at, one_at, sizes


def test_numpy_decide_rqt_is_tu_decision_hpp():
    """decide_rqt with the stand-in's rates against search/tu_decision.hpp's decideRqt (tests/search_client.cpp: client_rqt_decide takes a rate per tree): the
    restatement is pinned before it judges the device"""
    import search_tools as st
    cpu = st.Client("oracle")
    units, zero_at, one_at, sizes = _random_trees(5, 600)
    for s in sizes.values():
        s["rate"] = R.tu_rate(s["cbf"], s["nonzero"], s["sum_abs"])
    rl = 1234567
    got = R.decide_rqt(units, zero_at, one_at, sizes, rl)
    rows = np.zeros((len(units), 6), np.int64)
    for i, u in enumerate(units):
        s0, s1, j0, j1 = sizes[int(u["log2_size"])], sizes[int(u["log2_size"]) - 1], int(zero_at[i]), int(one_at[i])
        rows[i] = (int((s1["cbf"][j1:j1 + 4] != 0).any()), int(s1["ssd"][j1:j1 + 4].astype(np.int64).sum()), int(s1["rate"][j1:j1 + 4].sum()), int(s0["ssd"][j0]),
                   int(s0["rate"][j0]), rl)
    want = cpu.rqt_decide(rows)
    assert np.array_equal(got["depth"], want[:, 0]) and np.array_equal(got["tried_zero"], want[:, 1])
    assert (got["depth"] == 1).any() and ((got["depth"] == 0) & (got["tried_zero"] == 1)).any() and (got["tried_zero"] == 0).any()
    # the costs are the sums the decision compares
    i = int(np.flatnonzero(got["tried_zero"] == 1)[0])
    j1 = int(one_at[i])
    s1 = sizes[int(units["log2_size"][i]) - 1]
    assert got["cost_one"][i] == int(s1["rate"][j1:j1 + 4].sum()) + rl * int(s1["ssd"][j1:j1 + 4].astype(np.int64).sum())


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def hv():
    from turingcodec_amd.havoc import Havoc
    h = Havoc(stream="new")
    yield h
    h.close()


def _torch_u8(hv, a):
    import torch
    with torch.cuda.stream(hv.tstream):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(hv.device)


@pytest.mark.gpu
@pytest.mark.parametrize("log2", SIZES)
def test_device_matches_golden_and_restatement(hv, golden, restated, log2):
    """launches of 1, 63, 64, 65 and 257 jobs (wavefront and workgroup boundaries); jobs of 1..4 blocks and several snapshots in every launch"""
    g, (rates, after, _) = golden[log2], restated[log2]
    for njobs in (1, 63, 64, 65, 257):
        jobs = g["jobs"][:njobs]
        got, got_after = hv.residual_rate(log2, g["levels"], g["states"], jobs)
        nr = len(got)
        assert nr == int(jobs["rate_index"][-1]) + int(jobs["count"][-1])
        assert np.array_equal(got, g["rates"][:nr]), (njobs, np.flatnonzero(got != g["rates"][:nr])[:8])
        assert np.array_equal(got, rates[:nr])
        assert np.array_equal(got_after, g["after"][:njobs]) and np.array_equal(got_after, after[:njobs])
    assert len(np.unique(g["jobs"]["count"][:63])) == 4 and len(np.unique(g["jobs"]["ctx_index"][:63])) > 3


@pytest.mark.gpu
def test_device_contract(hv, golden):
    """d_states_out = NULL gives the same rates; d_states is not written; rates and levels outside the jobs' ranges are untouched; a replay from a graph gives the
    same bytes"""
    import torch
    log2 = 3
    g = golden[log2]
    jobs = g["jobs"][:130].copy()
    pad = 64
    jobs["level_off"] += pad
    jobs["rate_index"] += 5
    nr = int(jobs["rate_index"][-1]) + int(jobs["count"][-1])
    nl = int(jobs["level_off"][-1]) + int(jobs["count"][-1]) * 64
    levels = np.full(nl + pad, 12345, np.int16)
    levels[pad:nl] = g["levels"][:nl - pad]
    d_levels, d_states, d_jobs = hv.up(levels), _torch_u8(hv, g["states"]), _torch_u8(hv, jobs)
    with torch.cuda.stream(hv.tstream):
        d_rates = torch.full((nr + 7,), -77, dtype=torch.int64, device=hv.device)
        d_rates2 = torch.full((nr + 7,), -77, dtype=torch.int64, device=hv.device)
        d_after = torch.full((len(jobs) * 128 + 64,), 201, dtype=torch.uint8, device=hv.device)
    hv.residual_rate_d(log2, d_levels, d_states, d_jobs, d_rates, d_after)
    hv.residual_rate_d(log2, d_levels, d_states, d_jobs, d_rates2, None)
    rates, rates2 = hv.down(d_rates, np.int64), hv.down(d_rates2, np.int64)
    want = g["rates"][:nr - 5]
    assert np.array_equal(rates[5:nr], want) and np.array_equal(rates2, rates)
    assert (rates[:5] == -77).all() and (rates[nr:] == -77).all()
    assert np.array_equal(hv.down(d_levels, np.int16), levels)
    assert np.array_equal(hv.down(d_states, np.uint8), g["states"].reshape(-1))
    after = hv.down(d_after, np.uint8)
    assert np.array_equal(after[:len(jobs) * 128].reshape(-1, 128), g["after"][:len(jobs)]) and (after[len(jobs) * 128:] == 201).all()
    # the same launch from a captured graph
    with torch.cuda.stream(hv.tstream):
        d_rates.fill_(-1)
        d_after.fill_(7)
    graph = hv.graph_capture(lambda: hv.residual_rate_d(log2, d_levels, d_states, d_jobs, d_rates, d_after))
    for _ in range(2):
        with torch.cuda.stream(hv.tstream):
            d_rates.fill_(-77)
            d_after.fill_(201)
        hv.graph_launch(graph)
        assert np.array_equal(hv.down(d_rates, np.int64), rates) and np.array_equal(hv.down(d_after, np.uint8), after)
    hv.graph_destroy(graph)


@pytest.mark.gpu
def test_device_refusals(hv, golden):
    import torch
    from turingcodec_amd.havoc import HavocError
    g = golden[4]
    jobs = g["jobs"][:8].copy()
    d_levels, d_states, d_jobs = hv.up(g["levels"]), _torch_u8(hv, g["states"]), _torch_u8(hv, jobs)
    with torch.cuda.stream(hv.tstream):
        d_rates = torch.zeros(64, dtype=torch.int64, device=hv.device)
    for log2 in (1, 6):
        with pytest.raises(HavocError, match="log2TrafoSize"):
            hv.residual_rate_d(log2, d_levels, d_states, d_jobs, d_rates)
    for args in ((None, d_states, d_jobs, d_rates), (d_levels, None, d_jobs, d_rates), (d_levels, d_states, d_jobs, None)):
        with pytest.raises(HavocError, match="null"):
            hv.residual_rate_d(4, *args)
    with pytest.raises(HavocError, match="null"):
        hv._ck(hv.L.havoc_mi355x_residual_rate(hv.h, 4, d_levels.data_ptr(), d_states.data_ptr(), None, 1, d_rates.data_ptr(), None))
    with pytest.raises(HavocError, match="njobs"):
        hv._ck(hv.L.havoc_mi355x_residual_rate(hv.h, 4, d_levels.data_ptr(), d_states.data_ptr(), d_jobs.data_ptr(), -1, d_rates.data_ptr(), None))
    # jobs the entry point excludes: nothing of them is walked, their rates are -1, their snapshot passes through; the good jobs beside them are priced
    bad = g["jobs"][:8].copy()
    bad["rate_index"] = 4 * np.arange(8)
    bad["level_off"][[1, 2, 3, 4, 5]] = 1 << 30      # (would fault if read)
    bad["count"][1], bad["count"][2], bad["c_idx"][3], bad["scan_idx"][4], bad["scan_idx"][5] = 0, 5, 3, 3, 1      # (scan 1 with 16x16 blocks)
    rates, after = hv.residual_rate(4, g["levels"], g["states"], bad)
    want, want_after = R.walk_jobs(4, g["levels"], g["states"], bad)
    assert np.array_equal(rates, want) and np.array_equal(after, want_after)
    assert rates[4] == -1 and (rates[8:12] == -1).all() and rates[12] == -1 and rates[16] == -1 and rates[20] == -1 and rates[5] == 0 and rates[0] >= 0
    assert np.array_equal(after[1:6], g["states"][bad["ctx_index"][1:6]])
    # chroma with 32x32 blocks
    g5 = golden[5]
    bad = g5["jobs"][:2].copy()
    bad["c_idx"][1] = 1
    rates, _ = hv.residual_rate(5, g5["levels"], g5["states"], bad)
    assert (rates[int(bad["rate_index"][1]):] == -1).all() and np.array_equal(rates[:int(bad["rate_index"][1])], g5["rates"][:int(bad["rate_index"][1])])


def _device_trees(hv, units, zero_at, one_at, sizes, rated, rl, with_stats=True):
    """havoc_mi355x_rqt_decide / _rated over random outcomes -> (RQT_RESULT_DT records, {log2: final jobs int32 [m, 4]})"""
    import torch
    from turingcodec_amd.decisions import RQT_RESULT_DT
    table, rates, keep, fins = np.zeros((4, 5), np.uint64), np.zeros(4, np.uint64), [], {}
    for s, z in sizes.items():
        m = len(z["cbf"])
        jobs = np.stack([np.arange(m) * 7, np.arange(m) * 11 + 1, np.arange(m) * 13 + 2, np.full(m, -5)], 1).astype(np.int32)
        stats = np.stack([z["nonzero"], z["sum_abs"]], 1).astype(np.int32)
        d = [hv.up(z["cbf"]), hv.up(z["ssd"]), hv.up(stats), hv.up(jobs), hv.zeros(4 * m, np.int32)]
        with torch.cuda.stream(hv.tstream):
            d.append(torch.from_numpy(np.ascontiguousarray(z["rate"], np.int64)).to(hv.device))
        keep.append(d)
        table[s - 2] = [t.data_ptr() for t in d[:5]]
        if not with_stats:
            table[s - 2, 2] = 0
        rates[s - 2] = d[5].data_ptr()
        fins[s] = d[4]
    d_units = hv.up(np.ascontiguousarray(units).view(np.int32))
    out = hv.zeros(len(units) * 26, np.int32)
    args = (d_units.view(-1, 4), hv.up(zero_at), hv.up(one_at), table)
    if rated:
        hv.rqt_decide_rated_d(*args, rates, 1000, 512, 99, rl, out)
    else:
        hv.rqt_decide_d(*args, 1000, 512, 99, rl, out)
    return hv.down(out, np.int32).view(RQT_RESULT_DT).copy(), {s: hv.down(f, np.int32).reshape(-1, 4).copy() for s, f in fins.items()}


@pytest.mark.gpu
def test_rated_decision_with_the_stand_ins_values_is_the_stand_in_path(hv):
    units, zero_at, one_at, sizes = _random_trees(9, 700)
    for s in sizes.values():
        s["rate"] = R.tu_rate(s["cbf"], s["nonzero"], s["sum_abs"])
    a, fa = _device_trees(hv, units, zero_at, one_at, sizes, False, 54321)
    b, fb = _device_trees(hv, units, zero_at, one_at, sizes, True, 54321)
    assert a.tobytes() == b.tobytes() and all(fa[s].tobytes() == fb[s].tobytes() for s in fa)
    assert (a["depth"] == 1).any() and ((a["depth"] == 0) & (a["tried_zero"] == 1)).any() and (a["tried_zero"] == 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("with_stats", [True, False])
def test_rated_decision_with_arbitrary_rates_is_the_numpy_restatement(hv, with_stats):
    units, zero_at, one_at, sizes = _random_trees(10, 700)
    rng = np.random.default_rng(3)
    for s in sizes.values():
        s["rate"] = rng.integers(0, 1 << 26, len(s["cbf"])).astype(np.int64) * (rng.random(len(s["cbf"])) < 0.9)
    rl = 40000
    got, fin = _device_trees(hv, units, zero_at, one_at, sizes, True, rl, with_stats)
    want_sizes = sizes if with_stats else {s: {k: v for k, v in z.items() if k in ("cbf", "ssd", "rate")} for s, z in sizes.items()}
    want = R.decide_rqt(units, zero_at, one_at, want_sizes, rl)
    assert got.tobytes() == want.tobytes()
    assert (want["depth"] == 1).any() and ((want["depth"] == 0) & (want["tried_zero"] == 1)).any()
    # the final jobs: the chosen tree into the picture (rec_origin 1000, stride 512), the rest at the dump offset
    for i, u in enumerate(units):
        L, j0, j1 = int(u["log2_size"]), int(zero_at[i]), int(one_at[i])
        zero_wins = want["depth"][i] == 0 and want["tried_zero"][i] == 1
        half = 1 << (L - 1)
        assert list(fin[L][j0]) == [j0 * 7, j0 * 11 + 1, j0 * 13 + 2, 1000 + int(u["y0"]) * 512 + int(u["x0"]) if zero_wins else 99]
        for k in range(4):
            at = 99 if zero_wins else 1000 + (int(u["y0"]) + (k >> 1) * half) * 512 + int(u["x0"]) + (k & 1) * half
            assert list(fin[L - 1][j1 + k]) == [(j1 + k) * 7, (j1 + k) * 11 + 1, (j1 + k) * 13 + 2, at]


@pytest.fixture(scope="module")
def pictures(hv):
    """DecisionPicture(416, 240, 8 bit, QP 32, seed 21) with and without residual_rates: three steps each, the third replayed from the graph"""
    from turingcodec_amd.decisions import DecisionPicture
    out = {}
    for rated in (False, True):
        dp = DecisionPicture(hv, 416, 240, 8, 32, seed=21, threads=8, intra=False, residual_rates=rated)
        for _ in range(3):
            _, field, _ = dp.step()
        assert all(dp._graphs.values()) and len(dp._graphs) == 1
        out[rated] = (dp, field)
    return out


@pytest.mark.gpu
def test_picture_step_with_residual_rates(hv, pictures):
    import torch
    dp, field = pictures[True]
    P = dp.rqt_plan
    units, zero_at, one_at = dp.units, hv.down(P["d_zero_at"], np.int32), hv.down(P["d_one_at"], np.int32)
    results = dp.rqt_results.copy()
    # the rates: the restatement on the downloaded levels, from the unit's snapshot, the four depth-1 blocks as one chain
    sizes = {}
    for log2, g in P["sizes"].items():
        levels = hv.down(g["level"], np.int16)
        want, _ = R.walk_jobs(log2, levels, dp.rdoq_states, g["rate_jobs"])
        assert np.array_equal(dp.rqt_rates[log2], want), log2
        assert (want > 0).any()
        sizes[log2] = dict(cbf=hv.down(g["cbf"], np.int32), ssd=hv.down(g["ssd"], np.uint32), rate=dp.rqt_rates[log2])
    assert set(np.unique(np.concatenate([g["rate_jobs"]["count"] for g in P["sizes"].values()]))) == {1, 4}
    # the decisions: the numpy restatement on the downloaded outcomes and rates
    want = R.decide_rqt(units, zero_at, one_at, sizes, P["rl_q16"])
    assert results.tobytes() == want.tobytes()
    assert (results["depth"] == 1).any() and ((results["depth"] == 0) & (results["tried_zero"] == 1)).any()
    # the rates change decisions: at least one unit decides differently from the default picture
    base = pictures[False][0].rqt_results
    differ = (base["depth"] != results["depth"]) | (base["tried_zero"] != results["tried_zero"])
    print("units", len(units), "deciding differently with the reference's residual bits:", int(differ.sum()))
    assert differ.any()
    # the reconstruction is the chosen trees': the transform-tree part once more into a cleared picture, against the candidates' own reconstructions (pieces)
    with torch.cuda.stream(hv.tstream):
        dp.recon.zero_()
    dp.tree_decisions()
    hv.sync()
    assert hv.down(P["d_out"], np.int32).tobytes() == results.tobytes()
    recon = hv.down(dp.recon, dp.dt)
    pieces = {log2: hv.down(g["piece"], dp.dt) for log2, g in P["sizes"].items()}
    for i, u in enumerate(units):
        L, x0, y0 = int(u["log2_size"]), int(u["x0"]), int(u["y0"])
        blocks = [(L, int(zero_at[i]), x0, y0)] if results["depth"][i] == 0 and results["tried_zero"][i] == 1 else \
                 [(L - 1, int(one_at[i]) + k, x0 + (k & 1) * (1 << (L - 1)), y0 + (k >> 1) * (1 << (L - 1))) for k in range(4)]
        for s, j, x, y in blocks:
            n = 1 << s
            o = dp.origin + y * dp.stride + x
            got = recon[o + np.arange(n)[:, None] * dp.stride + np.arange(n)]
            assert np.array_equal(got, pieces[s][j * n * n:(j + 1) * n * n].reshape(n, n)), (i, s, j)


@pytest.mark.gpu
def test_residual_rates_are_refused_off_the_device_route(hv, pictures):
    from turingcodec_amd.decisions import DecisionPicture
    with pytest.raises(ValueError):
        DecisionPicture(hv, 416, 240, 8, 32, seed=21, threads=8, intra=False, search_on_device=False, residual_rates=True)
    with pytest.raises(ValueError):
        pictures[True][0].step_banded(hv)
    with pytest.raises(ValueError):
        pictures[False][0].rqt_rates


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(reflibs.REF_SO), reason="oracle/_ref not built")
def test_default_picture_step_is_unchanged(hv, pictures):
    """the default step (residual_rates=False): the decisions and the reconstruction the reference's tables + Rdoq.cpp give with the stand-in rate, as
    tests/test_decisions.py holds them"""
    import search_tools as st
    dp, field = pictures[False]
    ref = st.Client("ref", 3)
    pred = hv.down(dp.pred, dp.dt).copy()
    exp_rqt, exp_rec = ref.rqt(8, dp.host_planes[0], dp.stride, dp.PAD, pred, dp.W, dp.rdoq_states, dp.quant, dp.lam, 1.0 / dp.lam, dp.units)
    assert dp.rqt_results.tobytes() == exp_rqt.tobytes()
    import torch
    with torch.cuda.stream(hv.tstream):
        dp.recon.zero_()
    dp.tree_decisions()
    hv.sync()
    o = dp.origin
    rows = o + np.arange(dp.H)[:, None] * dp.stride + np.arange(dp.W)
    assert np.array_equal(hv.down(dp.recon, dp.dt)[rows], exp_rec[rows])
