"""The CABAC rate of a prediction unit's candidates and the inter mode decision on the device (havoc_mi355x_pu_rate, havoc_mi355x_pu_decide): what measurePuCost
measures per candidate and what go2 compares (turing/Search.hpp:1656-1706, 1829-1902).

CPU (-m "not gpu"): the plain-Python restatement tests/pu_rate_tools.pu_rate against (a) the reference's own Syntax<prediction_unit> under Measure<void> over coded data
filled as its search fills it (tests/pu_rate_shim.cpp, compiled at test time where the reference sources are) on fresh candidates and (b) the committed outputs of that
shim (tests/golden/pu_rate_golden.npz); the branches the candidates reach, asserted; the numpy decision against search/pu_decision.hpp's decidePu and the reference's
Cost / Lambda arithmetic; the library surface.  GPU (-m gpu): the kernels against the golden file, fresh jobs and the restatements -- every rate, every snapshot byte,
every refusal, every cost, best and winner snapshot -- and their contract (untouched memory, EINVAL, graph replay).
"""
import collections
import os

import numpy as np
import pytest

import pu_rate_tools as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pu_rate_golden.npz")
needs_ref = pytest.mark.skipif(PR.reference_dir() is None, reason="reference sources not present (the shim compiles them at test time)")
SLICE_IDS = list(range(len(PR.SLICES)))
slice_names = ["{}-M{}-z{}-r{}-{}".format("B" if s.slice_b else "P", *s[1:]) for s in PR.SLICES]


@pytest.fixture(scope="module")
def golden():
    from turingcodec_amd.havoc import PU_RATE_JOB_DT
    g = np.load(GOLDEN)
    out = {}
    for i, sl in enumerate(PR.SLICES):
        k = f"s{i}"
        assert tuple(g[k + ".slice"]) == tuple(sl)
        out[i] = dict(states=g[k + ".states"], jobs=g[k + ".jobs"].copy().view(PU_RATE_JOB_DT).reshape(-1), rates=g[k + ".rates"], after=g[k + ".after"])
    out["cost"] = dict(rows=g["cost.rows"], lam=g["cost.lambda"], cost=g["cost.cost"], lam_q16=g["cost.lambda_q16"])
    return out


@pytest.fixture(scope="module")
def restated(golden):
    """the restatement over the golden candidates, computed once: {slice: (rates, snapshots after, refusal reasons, branch counters)}"""
    out = {}
    for i, sl in enumerate(PR.SLICES):
        tags = collections.Counter()
        out[i] = PR.walk_jobs(golden[i]["jobs"], sl, golden[i]["states"], tags) + (tags,)
    return out


def _slice_params(sl):
    from turingcodec_amd.havoc import PuSlice
    return PuSlice(sl.slice_b, sl.max_num_merge_cand, sl.mvd_l1_zero_flag, (sl.num_ref_idx_l0, sl.num_ref_idx_l1))


# ------------------------------------------------------------------------------------------------------------------ CPU
@needs_ref
def test_restatement_matches_the_reference_on_fresh_candidates():
    """candidates the golden file has not seen, every slice: the rate of every candidate and all 16 context bytes it leaves"""
    shim = PR.Shim()
    for i, sl in enumerate(PR.SLICES):
        states, jobs = PR.make_cases(300 + i, sl, n_random=120)
        tags = collections.Counter()
        rates, after, why = PR.walk_jobs(jobs, sl, states, tags)
        want_rates, want_after = shim.walk_jobs(jobs, sl, states)
        assert np.array_equal(rates, want_rates), (sl, np.flatnonzero(rates != want_rates)[:8])
        assert np.array_equal(after, want_after), sl
        assert not [k for k in PR.required_tags(sl) if not tags[k]]
        valid = np.array([w is None for w in why])
        assert (rates[jobs["out_index"][valid]] >= 0).all() and (rates[jobs["out_index"][~valid]] == -1).all()


@needs_ref
def test_cost_arithmetic_is_the_references(golden):
    """rate + (satdY + satdCb + satdCr) * lambda in numpy against the reference's Cost and Lambda types, and Lambda::set(double)"""
    shim = PR.Shim()
    c = golden["cost"]
    for r, d, want, want_q in list(zip(c["rows"], c["lam"], c["cost"], c["lam_q16"]))[:60]:
        assert shim.cost(r[0], r[1:], d) == (int(want), int(want_q))


@pytest.mark.parametrize("i", SLICE_IDS, ids=slice_names)
def test_restatement_matches_golden(golden, restated, i):
    g, (rates, after, why, _) = golden[i], restated[i]
    assert np.array_equal(rates, g["rates"]) and np.array_equal(after, g["after"])
    jobs, before = g["jobs"], g["states"][g["jobs"]["ctx_index"]]
    refused = np.array([w is not None for w in why])
    # a refused candidate: -1 and its input snapshot; the reserved bytes of every candidate pass through; several jobs share a snapshot; out_index is no identity
    assert (g["rates"][jobs["out_index"][refused]] == -1).all() and (g["rates"][jobs["out_index"][~refused]] >= 0).all()
    assert np.array_equal(g["after"][refused], before[refused]) and np.array_equal(g["after"][:, 12:], before[:, 12:])
    assert len(np.unique(jobs["ctx_index"][:63])) < 63 and not np.array_equal(jobs["out_index"], np.arange(len(jobs)))
    assert len(jobs) >= 257 and len(jobs) % 64 != 0


def test_cost_table_matches_golden(golden):
    c = golden["cost"]
    lq = np.array([PR.lambda_q16(d) for d in c["lam"]], np.int64)
    assert np.array_equal(lq, c["lam_q16"])
    for k in range(len(lq)):
        cost, _, _, _ = PR.pu_decide([0], [1], c["rows"][k:k + 1, 0], c["rows"][k:k + 1, 1], c["rows"][k:k + 1, 2], c["rows"][k:k + 1, 3], int(lq[k]))
        assert cost[0] == c["cost"][k]


@pytest.mark.parametrize("i", SLICE_IDS, ids=slice_names)
def test_golden_candidates_reach_every_branch(restated, i):
    tags = restated[i][3]
    missing = [k for k in PR.required_tags(PR.SLICES[i]) if not tags[k]]
    assert not missing, missing


def test_coverage_of_the_slices():
    """what required_tags asks per slice adds up to what the candidates must reach over all slices"""
    S = PR.SLICES
    assert {s.max_num_merge_cand for s in S if s.slice_b} == {1, 2, 3, 4, 5} == {s.max_num_merge_cand for s in S if not s.slice_b}
    assert any(s.slice_b and s.mvd_l1_zero_flag for s in S) and any(s.slice_b and not s.mvd_l1_zero_flag for s in S)
    for l in (3, 4):
        assert any(s.slice_b and s[l] == 0 for s in S) and any(s.slice_b and s[l] > 2 for s in S)
    need = set()
    for s in S:
        need |= set(PR.required_tags(s))
    assert {("merge", M, i, how) for M in range(1, 6) for i in range(M) for how in ("merge", "skip")} <= need
    assert {("pred", p, d) for p in range(3) for d in range(4)} <= need and {("small", 8, 4, 0), ("small", 4, 8, 1)} <= need
    assert {("mvd", c, a, neg) for c in (0, 1) for a in (1, 2, 3, 4) for neg in (False, True)} <= need and ("eg1_bins", 30) in need
    assert {("refused", r) for r in PR.REFUSALS} <= need and "mvd_l1_zero_bi" in need
    assert 32767 in PR.MVD_VALUES and -32768 in PR.MVD_VALUES and PR.eg1_bins(32766) == 30 and PR.eg1_bins(0) == 2


def _made_units_hold(first, count, rates, cost, best, best_cost, lam):
    """units 0-5 of pu_rate_tools.random_units"""
    assert list(best[:6]) == [0, 1, -1, 1, 1, -1] and list(best_cost[[2, 5]]) == [-1, -1]
    f = first
    assert cost[f[0]] == cost[f[0] + 1] == cost[f[0] + 2] and cost[f[1] + 1] == cost[f[1] + 2] < cost[f[1]]
    assert (cost[f[2]:f[2] + 3] == -1).all() and cost[f[3]] == -1
    assert cost[f[4]] == lam + 1 and cost[f[4] + 1] == lam and best_cost[4] == lam


def test_numpy_decision_is_pu_decision_hpp():
    """pu_decide against search/pu_decision.hpp's decidePu (tests/pu_decide_client.cpp, compiled here): the restatement is pinned before it judges the device"""
    client = PR.DecisionClient()
    for seed, n, lam in ((3, 6, 0), (2, 64, PR.lambda_q16(3.5)), (1, 300, PR.lambda_q16(0.07))):
        first, count, rates, sy, scb, scr, after = PR.random_units(seed, n, lam)
        cost, best, best_cost, best_syntax = PR.pu_decide(first, count, rates, sy, scb, scr, lam, after)
        want = client.decide(first, count, rates, sy, scb, scr, lam)
        assert np.array_equal(cost, want[0]) and np.array_equal(best, want[1]) and np.array_equal(best_cost, want[2])
        if lam:
            _made_units_hold(first, count, rates, cost, best, best_cost, lam)
        won = best >= 0
        assert np.array_equal(best_syntax[won], after[first[won] + best[won]]) and not best_syntax[~won].any()
    assert (best[6:] > 0).any() and (cost > 1 << 40).any()


def test_library_surface():
    from turingcodec_amd import havoc
    L, names = havoc._load()
    assert L.havoc_mi355x_pu_rate and L.havoc_mi355x_pu_decide and {"pu_rate", "pu_decide"} <= set(names)
    dt = havoc.PU_RATE_JOB_DT
    assert dt.itemsize == 32 and [dt.fields[k][1] for k in ("ctx_index", "out_index", "mvd", "merge_idx", "pred", "mvp_flag", "ref_idx", "w", "h", "cqt_depth", "flags")] == \
        [0, 4, 8, 16, 17, 18, 20, 22, 23, 24, 25]
    assert (havoc.PU_RATE_MERGE, havoc.PU_RATE_SKIP) == (PR.MERGE, PR.SKIP) == (1, 2) and havoc.PU_SYNTAX_CTX_BYTES == PR.SYNTAX_BYTES == 16
    header = open(os.path.join(ROOT, "include", "havoc_mi355x.h")).read()
    for name in ("havoc_mi355x_pu_rate(", "havoc_mi355x_pu_decide(", "} havoc_mi355x_pu_rate_job;   /* sizeof: 32 */", "} havoc_mi355x_pu_slice;",
                 "HAVOC_PU_SYNTAX_CTX_MERGE_FLAG = 0", "HAVOC_PU_SYNTAX_CTX_MERGE_IDX = 1", "HAVOC_PU_SYNTAX_CTX_INTER_PRED_IDC = 2", "HAVOC_PU_SYNTAX_CTX_REF_IDX = 7",
                 "HAVOC_PU_SYNTAX_CTX_ABS_MVD_GREATER0 = 9", "HAVOC_PU_SYNTAX_CTX_ABS_MVD_GREATER1 = 10", "HAVOC_PU_SYNTAX_CTX_MVP_FLAG = 11", "HAVOC_PU_SYNTAX_CTX_BYTES = 16"):
        assert name in header, name
    assert (PR.MERGE_FLAG, PR.MERGE_IDX, PR.INTER_PRED_IDC, PR.REF_IDX, PR.GREATER0, PR.GREATER1, PR.MVP_FLAG) == (0, 1, 2, 7, 9, 10, 11)


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


def _torch(hv, a, dtype):
    import torch
    with torch.cuda.stream(hv.tstream):
        return torch.from_numpy(np.ascontiguousarray(a, dtype).reshape(-1).copy()).to(hv.device)


@pytest.mark.gpu
@pytest.mark.parametrize("i", SLICE_IDS, ids=slice_names)
def test_device_matches_golden_and_restatement(hv, golden, restated, i):
    """launches of 1, 63, 64, 65 jobs and the golden set (no multiple of 64), refusals among them: every rate, every snapshot byte"""
    g, (rates, after, why, _), sl = golden[i], restated[i], PR.SLICES[i]
    for njobs in (1, 63, 64, 65, len(g["jobs"])):
        jobs = g["jobs"][:njobs]
        got, got_after = hv.pu_rate(g["states"], jobs, _slice_params(sl))
        idx = jobs["out_index"]
        assert np.array_equal(got[idx], g["rates"][idx]), (njobs, np.flatnonzero(got[idx] != g["rates"][idx])[:8])
        assert np.array_equal(got[idx], rates[idx])
        assert np.array_equal(got_after, g["after"][:njobs]) and np.array_equal(got_after, after[:njobs])
        written = np.zeros(len(got), bool)
        written[idx] = True
        assert not got[~written].any()
    assert any(w is not None for w in why)


@pytest.mark.gpu
def test_device_matches_restatement_on_fresh_jobs(hv):
    for i, sl in enumerate(PR.SLICES[:4]):
        states, jobs = PR.make_cases(900 + i, sl, n_random=40)
        rates, after, _ = PR.walk_jobs(jobs, sl, states)
        got, got_after = hv.pu_rate(states, jobs, _slice_params(sl))
        assert np.array_equal(got, rates) and np.array_equal(got_after, after)


@pytest.mark.gpu
def test_device_contract(hv, golden):
    """a NULL output snapshot table gives the same rates; no input is written; guard entries around every output are untouched; both entries replay from a graph,
    the second time over other jobs in the same buffers"""
    import torch
    sl, g = PR.SLICES[2], golden[2]
    n = 130
    jobs = g["jobs"][:n].copy()
    jobs["out_index"] = np.arange(n)
    jobs2 = g["jobs"][200:200 + n].copy()
    jobs2["out_index"] = np.arange(n)
    sp = _slice_params(sl)
    lam = PR.lambda_q16(0.11)
    count = np.full(26, 5, np.int32)
    first = (np.arange(26) * 5).astype(np.int32)
    rng = np.random.default_rng(5)
    satd = rng.integers(0, 4000, (3, n)).astype(np.int32)
    d_states, d_jobs = _torch_u8(hv, g["states"]), _torch_u8(hv, jobs)
    d_first, d_count, d_satd = _torch(hv, first, np.int32), _torch(hv, count, np.int32), [_torch(hv, s, np.int32) for s in satd]
    with torch.cuda.stream(hv.tstream):
        d_rates = torch.full((n + 16,), -77, dtype=torch.int64, device=hv.device)
        d_rates2 = torch.full((n + 16,), -77, dtype=torch.int64, device=hv.device)
        d_after = torch.full((64 + n * 16 + 64,), 201, dtype=torch.uint8, device=hv.device)
        d_cost = torch.full((n + 16,), -78, dtype=torch.int64, device=hv.device)
        d_best = torch.full((26 + 16,), -79, dtype=torch.int32, device=hv.device)
        d_best_cost = torch.full((26 + 16,), -80, dtype=torch.int64, device=hv.device)
        d_best_cost2 = torch.full((26 + 16,), -80, dtype=torch.int64, device=hv.device)
        d_best_syntax = torch.full((64 + 26 * 16 + 64,), 202, dtype=torch.uint8, device=hv.device)

    def run():
        hv.pu_rate_d(d_states, d_jobs, sp, d_rates[8:], d_after[64:])
        hv.pu_decide_d(d_first, d_count, 26, d_rates[8:], *d_satd, lam, d_after[64:], d_cost[8:], d_best[8:], d_best_cost[8:], d_best_syntax[64:])

    def check(jb, k):
        rates, after, _ = PR.walk_jobs(jb, sl, g["states"])
        cost, best, best_cost, best_syntax = PR.pu_decide(first, count, rates, *satd, lam, after)
        got = hv.down(d_rates, np.int64)
        assert np.array_equal(got[8:8 + n], rates) and (got[:8] == -77).all() and (got[8 + n:] == -77).all(), k
        a = hv.down(d_after, np.uint8)
        assert np.array_equal(a[64:64 + 16 * n].reshape(-1, 16), after) and (a[:64] == 201).all() and (a[64 + 16 * n:] == 201).all(), k
        c, b, bc, bs = hv.down(d_cost, np.int64), hv.down(d_best, np.int32), hv.down(d_best_cost, np.int64), hv.down(d_best_syntax, np.uint8)
        assert np.array_equal(c[8:8 + n], cost) and (c[:8] == -78).all() and (c[8 + n:] == -78).all(), k
        assert np.array_equal(b[8:34], best) and (b[:8] == -79).all() and (b[34:] == -79).all(), k
        assert np.array_equal(bc[8:34], best_cost) and (bc[:8] == -80).all() and (bc[34:] == -80).all(), k
        assert np.array_equal(bs[64:64 + 16 * 26].reshape(-1, 16), best_syntax) and (bs[:64] == 202).all() and (bs[64 + 16 * 26:] == 202).all(), k
        return rates, best

    run()
    rates1, best1 = check(jobs, "direct")
    hv.pu_rate_d(d_states, d_jobs, sp, d_rates2[8:], None)
    assert np.array_equal(hv.down(d_rates2, np.int64), hv.down(d_rates, np.int64))
    hv.pu_decide_d(d_first, d_count, 26, d_rates[8:], *d_satd, lam, None, d_cost[8:], d_best[8:], d_best_cost2[8:], None)
    assert np.array_equal(hv.down(d_best_cost2, np.int64), hv.down(d_best_cost, np.int64))
    assert np.array_equal(hv.down(d_states, np.uint8), g["states"].reshape(-1)) and np.array_equal(hv.down(d_jobs, np.uint8), jobs.view(np.uint8).reshape(-1))
    assert np.array_equal(hv.down(d_first, np.int32), first) and np.array_equal(hv.down(d_count, np.int32), count)
    for t, s in zip(d_satd, satd):
        assert np.array_equal(hv.down(t, np.int32), s)
    graph = hv.graph_capture(run)
    for k, jb in enumerate((jobs, jobs2)):
        with torch.cuda.stream(hv.tstream):
            d_jobs.copy_(torch.from_numpy(jb.view(np.uint8).reshape(-1).copy()))
            d_rates.fill_(-77)
            d_after.fill_(201)
            d_cost.fill_(-78)
            d_best.fill_(-79)
            d_best_cost.fill_(-80)
            d_best_syntax.fill_(202)
        hv.graph_launch(graph)
        rates2, best2 = check(jb, k)
    assert not np.array_equal(rates1, rates2) and (rates1 == -1).any() and (best1 > 0).any()
    hv.graph_destroy(graph)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [6, 255, 256, 257, 1500])
def test_decision_is_the_numpy_restatement(hv, n):
    """made ties, refused candidates and empty units first, arbitrary units behind them: every cost, best, best cost and winner snapshot"""
    lam = PR.lambda_q16(0.07)
    first, count, rates, sy, scb, scr, after = PR.random_units(40 + n, n, lam)
    want = PR.pu_decide(first, count, rates, sy, scb, scr, lam, after)
    got = hv.pu_decide(first, count, rates, sy, scb, scr, lam, after)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    _made_units_hold(first, count, rates, got[0], got[1], got[2], lam)


@pytest.mark.gpu
def test_device_einval(hv, golden):
    import torch
    from turingcodec_amd.havoc import HavocError, PuSlice
    g = golden[0]
    jobs = g["jobs"][:8].copy()
    d_states, d_jobs = _torch_u8(hv, g["states"]), _torch_u8(hv, jobs)
    with torch.cuda.stream(hv.tstream):
        d_rates = torch.zeros(1024, dtype=torch.int64, device=hv.device)
        d_out = torch.zeros(8 * 16, dtype=torch.uint8, device=hv.device)
        d_i32 = torch.zeros(64, dtype=torch.int32, device=hv.device)
        d_i64 = torch.zeros(64, dtype=torch.int64, device=hv.device)
        d_i64b = torch.zeros(64, dtype=torch.int64, device=hv.device)
    sp = PuSlice()
    f = hv.L.havoc_mi355x_pu_rate
    import ctypes as C
    p = [d_states.data_ptr(), d_jobs.data_ptr(), 8, C.addressof(sp), d_rates.data_ptr(), d_out.data_ptr()]
    hv._ck(f(hv.h, *p))
    for k in (0, 1, 3, 4):
        q = list(p)
        q[k] = None
        with pytest.raises(HavocError, match="null"):
            hv._ck(f(hv.h, *q))
    q = list(p)
    q[2] = -1
    with pytest.raises(HavocError, match="njobs"):
        hv._ck(f(hv.h, *q))
    q = list(p)
    q[5] = q[0]
    with pytest.raises(HavocError, match="d_syntax_out"):
        hv._ck(f(hv.h, *q))
    for k in (0, 4, 5):
        q = list(p)
        q[k] += 4
        with pytest.raises(HavocError, match="aligned"):
            hv._ck(f(hv.h, *q))
    for bad in (PuSlice(1, 0), PuSlice(1, 6)):
        with pytest.raises(HavocError, match="MaxNumMergeCand"):
            hv.pu_rate_d(d_states, d_jobs, bad, d_rates, d_out)
    for bad in (PuSlice(1, 5, 0, (16, 0)), PuSlice(1, 5, 0, (0, -1))):
        with pytest.raises(HavocError, match="num_ref_idx"):
            hv.pu_rate_d(d_states, d_jobs, bad, d_rates, d_out)
    # pu_decide: first, count, n, rate, satd x 3, lambda, syntax after, cost, best, best cost, best syntax
    good = [d_i32, d_i32, 4, d_i64, d_i32, d_i32, d_i32, 100, d_out, d_i64b, d_i32, d_rates, d_out]
    good[12] = None
    hv.pu_decide_d(*good)
    for k in (0, 1, 3, 4, 5, 6, 9, 10, 11):
        a = list(good)
        a[k] = None
        with pytest.raises(HavocError, match="null"):
            hv.pu_decide_d(*a)
    a = list(good)
    a[2] = -1
    with pytest.raises(HavocError, match="n < 0"):
        hv.pu_decide_d(*a)
    a = list(good)
    a[7] = -1
    with pytest.raises(HavocError, match="lambda"):
        hv.pu_decide_d(*a)
    a = list(good)
    a[8], a[12] = None, d_out
    with pytest.raises(HavocError, match="d_syntax_after"):
        hv.pu_decide_d(*a)
    a = list(good)
    a[12] = d_out
    with pytest.raises(HavocError, match="d_best_syntax"):
        hv.pu_decide_d(*a)
    a = list(good)
    a[9] = d_i64
    with pytest.raises(HavocError, match="d_rate"):
        hv.pu_decide_d(*a)
    a = list(good)
    a[9] = d_i64b[1:].view(torch.uint8)[4:]
    with pytest.raises(HavocError, match="aligned"):
        hv.pu_decide_d(*a)
    # njobs == 0 and n == 0 launch nothing
    hv._ck(f(hv.h, p[0], p[1], 0, p[3], p[4], None))
    a = list(good)
    a[2] = 0
    hv.pu_decide_d(*a)
