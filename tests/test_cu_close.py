"""Closing an inter coding unit on the device (havoc_mi355x_cu_close) and the prediction's distortion it needs (havoc_mi355x_unit_pred_ssd): what
Search<IfCbf<rqt_root_cbf, transform_tree>>::go prices and decides (turing/Search.hpp:2362-2568).

CPU (-m "not gpu"): the plain-Python restatement tests/cu_close_tools.close against (a) the reference's own Syntax<coding_unit> under Measure<void> and its Cost / Lambda
arithmetic (tests/cu_close_shim.cpp, compiled at test time where the reference sources are) on fresh jobs and (b) the committed outputs of that shim
(tests/golden/cu_close_golden.npz); the branches the golden jobs reach, asserted by name, and the four outcomes the reference's own results show; the numpy decision
against search/cu_decision.hpp's closeInterCu; the library surface.  GPU (-m gpu): the kernels against the golden file, the restatement and numpy -- every field, every
snapshot byte, every refusal -- and their contract (untouched inputs, EINVAL, graph replay).
"""
import collections
import os

import numpy as np
import pytest

import cu_close_tools as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cu_close_golden.npz")
needs_ref = pytest.mark.skipif(CC.reference_dir() is None, reason="reference sources not present (the shim compiles them at test time)")
SLICE_IDS = list(range(len(CC.SLICES)))
slice_names = ["{}-M{}-{}".format("B" if s.slice_b else "P", s.max_num_merge_cand, s.reciprocal_lambda) for s in CC.SLICES]
CASE_KEYS = ("cu_syntax", "pu_before", "pu_after", "pu_rate", "choice", "tree_choice", "tree_rate", "pred_ssd", "jobs")


@pytest.fixture(scope="module")
def golden():
    from turingcodec_amd.decisions import RQT_RESULT_DT
    from turingcodec_amd.havoc import CU_CHOICE_DT, CU_CLOSE_JOB_DT, RQT_TREE_RESULT_DT
    g = np.load(GOLDEN)
    dts = dict(choice=RQT_RESULT_DT, tree_choice=RQT_TREE_RESULT_DT, jobs=CU_CLOSE_JOB_DT)
    out = {}
    for i, sl in enumerate(CC.SLICES):
        k = f"s{i}"
        assert tuple(g[k + ".slice"]) == tuple(float(v) for v in sl)
        case = {name: (g[f"{k}.{name}"].copy().view(dts[name]).reshape(-1) if name in dts else g[f"{k}.{name}"]) for name in CASE_KEYS}
        out[i] = dict(case=case, out=g[k + ".out"].copy().view(CU_CHOICE_DT).reshape(-1), cu_after=g[k + ".cu_after"], pu_after_out=g[k + ".pu_after_out"])
    out["cost"] = dict(rows=g["cost.rows"], lam=g["cost.lambda"], ref=g["cost.ref"])
    return out


@pytest.fixture(scope="module")
def restated(golden):
    """the restatement over the golden jobs, computed once: {launch: (records, CU snapshots, PU snapshots, refusal reasons, branch counters)}"""
    out = {}
    for i, sl in enumerate(CC.SLICES):
        tags = collections.Counter()
        out[i] = CC.walk_jobs(golden[i]["case"], sl, tags) + (tags,)
    return out


def _same_records(a, b):
    return [k for k in CC.CHOICE_FIELDS if not np.array_equal(a[k], b[k])]


# ------------------------------------------------------------------------------------------------------------------ CPU
@needs_ref
def test_restatement_matches_the_reference_on_fresh_jobs():
    """jobs the golden file has not seen, every launch: outcome, rate, lambdaDistortion, the costs and every byte of both snapshots"""
    shim = CC.Shim()
    for i, sl in enumerate(CC.SLICES):
        case = CC.make_cases(500 + i, sl, n_random=60)
        tags = collections.Counter()
        out, cu, pu, why = CC.walk_jobs(case, sl, tags)
        want, want_cu, want_pu, _ = CC.walk_jobs(case, sl, closer=shim.close)
        assert not _same_records(out, want), (sl, _same_records(out, want))
        assert np.array_equal(cu, want_cu) and np.array_equal(pu, want_pu), sl
        assert not [k for k in CC.required_tags(sl) if not tags[k]]
        refused = np.array([w is not None for w in why])
        assert (out["rate"][refused] == -1).all() and (out["rate"][~refused] >= 0).all() and refused.any()


@needs_ref
def test_cost_arithmetic_is_the_references(golden):
    """the two costs and the strict comparison against the reference's Cost and Lambda types, and Lambda::set(double)"""
    shim = CC.Shim()
    c = golden["cost"]
    for r, d, want in list(zip(c["rows"], c["lam"], c["ref"]))[:80]:
        assert shim.costs(r[2], r[4:7], r[3], r[7:10], d) == [int(v) for v in want]


@pytest.mark.parametrize("i", SLICE_IDS, ids=slice_names)
def test_restatement_matches_golden(golden, restated, i):
    g, (out, cu, pu, why, _) = golden[i], restated[i]
    assert not _same_records(out, g["out"]), _same_records(out, g["out"])
    assert np.array_equal(cu, g["cu_after"]) and np.array_equal(pu, g["pu_after_out"])
    case = g["case"]
    jobs, before = case["jobs"], case["cu_syntax"][case["jobs"]["ctx_index"]]
    refused = np.array([w is not None for w in why])
    # a refused job: -1 everywhere and its input snapshots; the split_cu_flag and reserved bytes of every job pass through; the snapshots are shared between jobs
    assert (g["out"]["outcome"][refused] == -1).all() and (g["out"]["cost"][refused] == -1).all() and (g["out"]["rate"][~refused] >= 0).all()
    assert np.array_equal(g["cu_after"][refused], before[refused]) and np.array_equal(g["pu_after_out"][refused], case["pu_after"][jobs["pu_after_index"]][refused])
    assert np.array_equal(g["cu_after"][:, :3], before[:, :3]) and np.array_equal(g["cu_after"][:, 12:], before[:, 12:])
    assert len(np.unique(jobs["ctx_index"][:63])) < 63 and not np.array_equal(jobs["unit_index"], np.arange(len(jobs)))
    assert len(jobs) >= 257 and len(jobs) % 64 != 0


def test_cost_table_matches_golden(golden):
    c = golden["cost"]
    for k, (r, d, want) in enumerate(zip(c["rows"], c["lam"], c["ref"])):
        q = CC.lambda_q16(d)
        assert q == want[5]
        got = CC.decide([True], [r[1]], [r[2]], [r[3]], [r[4:7]], [r[7:10]], q)[0]
        assert got[4] == want[1] and got[5] == want[3] and (got[0] != CC.CODED) == bool(want[4])
        assert got[2] == (want[2] if want[4] else want[0])


@pytest.mark.parametrize("i", SLICE_IDS, ids=slice_names)
def test_golden_jobs_reach_every_branch(golden, restated, i):
    """by name; and the four outcomes on the REFERENCE's recorded results alone"""
    tags = restated[i][4]
    missing = [k for k in CC.required_tags(CC.SLICES[i]) if not tags[k]]
    assert not missing, missing
    out = golden[i]["out"]
    both = out["have_residual"] == 1
    assert ((out["outcome"] == CC.CODED) & (out["cost_coded"] < out["cost_no_residual"])).any(), "coded wins"
    assert (both & (out["outcome"] == CC.NO_RESIDUAL)).any(), "no residual wins"
    assert ((out["outcome"] == CC.CODED) & (out["cost_coded"] == out["cost_no_residual"])).any(), "equal cost keeps the residual"
    assert (~both & (out["outcome"] == CC.SKIPPED)).any() and (both & (out["outcome"] == CC.SKIPPED)).any(), "skipped"
    assert (both & (out["cost_coded"] == out["cost_no_residual"] + 1)).any() and (both & (out["cost_coded"] + 1 == out["cost_no_residual"])).any()


def test_coverage_of_the_launches():
    S = CC.SLICES
    assert {1, 5} <= {s.max_num_merge_cand for s in S if s.slice_b} and {1, 5} <= {s.max_num_merge_cand for s in S if not s.slice_b}
    need = set()
    for s in S:
        need |= set(CC.required_tags(s))
    assert {("refused", r) for r in CC.REFUSALS} <= need and {("skip_merge_idx", 5, i) for i in range(5)} <= need and "skip_merge_idx_not_coded" in need
    assert {("part_mode", CC.PART_MODES[pm], "amp_bypass") for pm in (4, 5, 6, 7)} <= need and ("part_mode", "NxN", "min_cb_third_bin") in need


def _decision_rows(seed, n, lam):
    rng = np.random.default_rng(seed)
    have, merged = rng.integers(0, 2, n).astype(bool), rng.integers(0, 2, n).astype(bool)
    rc, rn = rng.integers(0, 900 << 16, n), rng.integers(0, 100 << 16, n)
    ssd, sp = rng.integers(0, 1 << 20, (n, 3)), rng.integers(0, 1 << 20, (n, 3))
    # made rows: 0 equal costs (the residual stays), 1 the unit without residual cheaper by one Q16 unit, 2 dearer by one, 3 an int32 sum that wraps, 4 no residual
    have[:5], merged[:5] = [1, 1, 1, 1, 0], [0, 1, 0, 1, 1]
    ssd[:3], sp[:3] = [10, 20, 30], [[60, 1, 2]] * 3
    rn[:3] = 5 << 16
    rc[:3] = [(5 << 16) + 3 * lam, (5 << 16) + 3 * lam + 1, (5 << 16) + 3 * lam - 1]
    ssd[3] = [0x30000000] * 3
    return have, merged, rc, rn, ssd, sp


def test_numpy_decision_is_cu_decision_hpp():
    """decide against search/cu_decision.hpp's closeInterCu (tests/cu_close_client.cpp, compiled here): the restatement is pinned before it judges the device"""
    client = CC.DecisionClient()
    for seed, n, lam in ((3, 5, 0), (2, 64, CC.lambda_q16(0.0217)), (1, 300, CC.lambda_q16(0.14))):
        rows = _decision_rows(seed, n, lam)
        got, want = CC.decide(*rows, lam), client.decide(*rows, lam)
        assert np.array_equal(got, want), np.flatnonzero((got != want).any(1))[:8]
        if lam:
            assert list(got[:5, 0]) == [CC.CODED, CC.SKIPPED, CC.CODED, got[3, 0], CC.SKIPPED] and got[0, 4] == got[0, 5] and got[1, 4] == got[1, 5] + 1
            assert got[3, 2] < 0 or got[3, 0] != CC.CODED           # the wrapped sum is negative where it is the winner's
            assert got[4, 4] == -1 and got[4, 1] == rows[3][4]
    assert {CC.CODED, CC.NO_RESIDUAL, CC.SKIPPED} == set(got[:, 0])


def test_library_surface():
    from turingcodec_amd import havoc
    L, names = havoc._load()
    assert L.havoc_mi355x_cu_close and L.havoc_mi355x_unit_pred_ssd and {"cu_close", "unit_pred_ssd"} <= set(names)
    dt = havoc.CU_CLOSE_JOB_DT
    assert dt.itemsize == 32 and [dt.fields[k][1] for k in ("ctx_index", "unit_index", "pu_rate_index", "pu_before_index", "pu_after_index", "log2_cb_size", "part_mode",
                                                            "skip_ctx_inc", "merge_idx", "flags")] == [0, 4, 8, 12, 16, 20, 21, 22, 23, 24]
    dt = havoc.CU_CHOICE_DT
    assert dt.itemsize == 48 and [dt.fields[k][1] for k in CC.CHOICE_FIELDS] == [0, 4, 8, 16, 24, 32, 40]
    assert havoc.PRED_SSD_JOB_DT.itemsize == 32 and havoc.CU_SYNTAX_CTX_BYTES == CC.SYNTAX_BYTES == 16
    assert (havoc.CU_CLOSE_MIN_CB, havoc.CU_CLOSE_AMP, havoc.CU_CLOSE_MERGE_2Nx2N) == (CC.MIN_CB, CC.AMP, CC.MERGE_2Nx2N) == (1, 2, 4)
    assert (havoc.CU_OUTCOME_REFUSED, havoc.CU_OUTCOME_CODED, havoc.CU_OUTCOME_NO_RESIDUAL, havoc.CU_OUTCOME_SKIPPED) == (CC.REFUSED, CC.CODED, CC.NO_RESIDUAL, CC.SKIPPED)
    header = open(os.path.join(ROOT, "include", "havoc_mi355x.h")).read()
    for name in ("havoc_mi355x_cu_close(", "havoc_mi355x_unit_pred_ssd(", "} havoc_mi355x_cu_close_job;   /* sizeof: 32 */", "} havoc_mi355x_cu_choice;",
                 "HAVOC_CU_SYNTAX_CTX_SPLIT_CU_FLAG = 0", "HAVOC_CU_SYNTAX_CTX_CU_SKIP_FLAG = 3", "HAVOC_CU_SYNTAX_CTX_PRED_MODE_FLAG = 6", "HAVOC_CU_SYNTAX_CTX_PART_MODE = 7",
                 "HAVOC_CU_SYNTAX_CTX_RQT_ROOT_CBF = 11", "HAVOC_CU_SYNTAX_CTX_BYTES = 16"):
        assert name in header, name
    assert (CC.SPLIT_CU_FLAG, CC.CU_SKIP_FLAG, CC.PRED_MODE_FLAG, CC.PART_MODE, CC.RQT_ROOT_CBF) == (0, 3, 6, 7, 11)


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


def _close(hv, case, sl, njobs=None):
    jobs = case["jobs"] if njobs is None else case["jobs"][:njobs]
    return hv.cu_close(case["cu_syntax"], case["pu_before"], case["pu_after"], case["pu_rate"], case["choice"], case["tree_choice"], case["tree_rate"], case["pred_ssd"],
                       jobs, sl.max_num_merge_cand, CC.lambda_q16(sl.reciprocal_lambda))


@pytest.mark.gpu
@pytest.mark.parametrize("i", SLICE_IDS, ids=slice_names)
def test_device_matches_golden_and_restatement(hv, golden, restated, i):
    """launches of 1, 63, 64, 65 jobs and the golden set (no multiple of 64), refusals among them: every field, every byte of both snapshots"""
    g, (out, cu, pu, why, _), sl = golden[i], restated[i], CC.SLICES[i]
    case = g["case"]
    for njobs in (1, 63, 64, 65, len(case["jobs"])):
        got, got_cu, got_pu = _close(hv, case, sl, njobs)
        assert not _same_records(got, g["out"][:njobs]), (njobs, _same_records(got, g["out"][:njobs]))
        assert not _same_records(got, out[:njobs])
        assert np.array_equal(got_cu, g["cu_after"][:njobs]) and np.array_equal(got_cu, cu[:njobs])
        assert np.array_equal(got_pu, g["pu_after_out"][:njobs]) and np.array_equal(got_pu, pu[:njobs])
        before = case["cu_syntax"][case["jobs"]["ctx_index"][:njobs]]
        assert np.array_equal(got_cu[:, :3], before[:, :3]) and np.array_equal(got_cu[:, 12:], before[:, 12:])
    assert any(w is not None for w in why[:63]) and any(w is not None for w in why)


@pytest.mark.gpu
def test_device_matches_restatement_on_fresh_jobs(hv):
    for i, sl in enumerate(CC.SLICES[:3]):
        case = CC.make_cases(950 + i, sl, n_random=40)
        out, cu, pu, _ = CC.walk_jobs(case, sl)
        got, got_cu, got_pu = _close(hv, case, sl)
        assert not _same_records(got, out) and np.array_equal(got_cu, cu) and np.array_equal(got_pu, pu)


@pytest.mark.gpu
def test_device_contract(hv, golden, restated):
    """no input is written; guard bytes around every output are untouched; the launch replays from a graph, the second time over other jobs in the same buffers"""
    import torch
    from turingcodec_amd.havoc import CU_CHOICE_DT
    i = 0
    sl, case, (out, cu, pu, _, _) = CC.SLICES[i], golden[i]["case"], restated[i]
    n, lam = 130, CC.lambda_q16(sl.reciprocal_lambda)
    names = ("cu_syntax", "pu_before", "pu_after", "pu_rate", "choice", "tree_choice", "tree_rate", "pred_ssd")
    d_in = [_torch_u8(hv, case[k]) for k in names]
    d_jobs = _torch_u8(hv, case["jobs"][:n])
    with torch.cuda.stream(hv.tstream):
        d_out = torch.full((64 + 48 * n + 64,), 203, dtype=torch.uint8, device=hv.device)
        d_cu = torch.full((64 + 16 * n + 64,), 204, dtype=torch.uint8, device=hv.device)
        d_pu = torch.full((64 + 16 * n + 64,), 205, dtype=torch.uint8, device=hv.device)

    def run():
        hv.cu_close_d(*d_in, d_jobs, sl.max_num_merge_cand, lam, d_out[64:], d_cu[64:], d_pu[64:])

    def check(lo, k):
        o, c, p = hv.down(d_out, np.uint8), hv.down(d_cu, np.uint8), hv.down(d_pu, np.uint8)
        assert (o[:64] == 203).all() and (o[64 + 48 * n:] == 203).all() and (c[:64] == 204).all() and (c[64 + 16 * n:] == 204).all(), k
        assert (p[:64] == 205).all() and (p[64 + 16 * n:] == 205).all(), k
        got = o[64:64 + 48 * n].copy().view(CU_CHOICE_DT)
        assert not _same_records(got, out[lo:lo + n]), k
        assert np.array_equal(c[64:64 + 16 * n].reshape(-1, 16), cu[lo:lo + n]) and np.array_equal(p[64:64 + 16 * n].reshape(-1, 16), pu[lo:lo + n]), k
        return o[64:64 + 48 * n].copy()

    run()
    first = check(0, "direct")
    for t, k in zip(d_in, names):
        assert np.array_equal(hv.down(t, np.uint8), np.ascontiguousarray(case[k]).view(np.uint8).reshape(-1)), k
    assert np.array_equal(hv.down(d_jobs, np.uint8), case["jobs"][:n].view(np.uint8).reshape(-1))
    graph = hv.graph_capture(run)
    for k, lo in enumerate((0, 200)):
        with torch.cuda.stream(hv.tstream):
            d_jobs.copy_(torch.from_numpy(case["jobs"][lo:lo + n].view(np.uint8).reshape(-1).copy()))
            d_out.fill_(203)
            d_cu.fill_(204)
            d_pu.fill_(205)
        hv.graph_launch(graph)
        again = check(lo, k)
        assert np.array_equal(again, first) == (lo == 0)
    hv.graph_destroy(graph)


@pytest.mark.gpu
def test_device_einval(hv, golden):
    import torch
    from turingcodec_amd.havoc import HavocError
    case = golden[0]["case"]
    names = ("cu_syntax", "pu_before", "pu_after", "pu_rate", "choice", "tree_choice", "tree_rate", "pred_ssd")
    d_in = [_torch_u8(hv, case[k]) for k in names] + [_torch_u8(hv, case["jobs"][:8])]
    with torch.cuda.stream(hv.tstream):
        outs = [torch.zeros(1024, dtype=torch.uint8, device=hv.device) for _ in range(3)]
    f = hv.L.havoc_mi355x_cu_close
    p = [t.data_ptr() for t in d_in] + [8, 5, 100] + [t.data_ptr() for t in outs]
    hv._ck(f(hv.h, *p))
    for k in list(range(9)) + [12, 13, 14]:
        q = list(p)
        q[k] = None
        with pytest.raises(HavocError, match="null"):
            hv._ck(f(hv.h, *q))
    for k, v, what in ((9, -1, "njobs"), (10, 0, "MaxNumMergeCand"), (10, 6, "MaxNumMergeCand"), (11, -1, "lambda")):
        q = list(p)
        q[k] = v
        with pytest.raises(HavocError, match=what):
            hv._ck(f(hv.h, *q))
    for k_out in (12, 13, 14):
        for k_in in (0, 2, 8):
            q = list(p)
            q[k_out] = q[k_in]
            with pytest.raises(HavocError, match="output"):
                hv._ck(f(hv.h, *q))
    q = list(p)
    q[13] = q[14]
    with pytest.raises(HavocError, match="distinct"):
        hv._ck(f(hv.h, *q))
    for k in (0, 3, 12, 14):
        q = list(p)
        q[k] += 4
        with pytest.raises(HavocError, match="aligned"):
            hv._ck(f(hv.h, *q))
    q = list(p)
    q[9] = 0
    hv._ck(f(hv.h, *q))                # njobs == 0 launches nothing
    # unit_pred_ssd: bit depth, (plane, stride) x 4, jobs, n, out
    g = hv.L.havoc_mi355x_unit_pred_ssd
    a, o = outs[0].data_ptr(), outs[1].data_ptr()
    good = [8, a, 64, a, 32, a, 64, a, 32, d_in[8].data_ptr(), 0, o]
    hv._ck(g(hv.h, *good))
    for k in (1, 3, 5, 7, 9, 11):
        q = list(good)
        q[k] = None
        with pytest.raises(HavocError, match="null"):
            hv._ck(g(hv.h, *q))
    for k, v, what in ((0, 7, "bit_depth"), (0, 17, "bit_depth"), (10, -1, "n < 0"), (2, 0, "stride"), (6, -64, "stride"), (11, a, "d_out")):
        q = list(good)
        q[k] = v
        with pytest.raises(HavocError, match=what):
            hv._ck(g(hv.h, *q))


def _ssd_case(seed, bd, njobs, extreme=False):
    """a source picture of 200 x 136 with a stride of 216 (no multiple of 64) and a prediction plane of its own stride; units of 8 to 64 at offset 0, at a 4-sample
    offset, against the picture's last row and column, and at random multiples of 4"""
    from turingcodec_amd.havoc import PRED_SSD_JOB_DT
    rng = np.random.default_rng(seed)
    W, H, ss, ps = 200, 136, 216, 208
    top = (1 << bd) - 1
    dt = np.uint8 if bd == 8 else np.uint16

    def plane(stride, rows, lo):
        if extreme:
            return np.full(stride * rows, lo, dt)
        return rng.integers(0, top + 1, stride * rows).astype(dt)

    src_y, src_c = plane(ss, H, 0), plane(ss // 2, H, 0)                     # Cb in rows 0..H/2-1, Cr below
    pred_y, pred_c = plane(ps, H, top), plane(ps // 2, H, top)
    jobs = np.zeros(njobs, PRED_SSD_JOB_DT)
    for j in range(njobs):
        log2 = (3, 4, 5, 6)[j % 4] if njobs > 1 else 6
        n = 1 << log2
        x, y = [(0, 0), (4, 4), (W - n, H - n), (W - n, 0), (0, H - n)][j] if j < 5 else (4 * int(rng.integers(0, (W - n) // 4 + 1)), 4 * int(rng.integers(0, (H - n) // 4 + 1)))
        px, py = (x, y) if j % 3 else (4 * int(rng.integers(0, (W - n) // 4 + 1)), 4 * int(rng.integers(0, (H - n) // 4 + 1)))
        jobs["log2_size"][j] = log2
        jobs["src_off"][j] = [y * ss + x, (y // 2) * (ss // 2) + x // 2, (H // 2 + y // 2) * (ss // 2) + x // 2]
        jobs["pred_off"][j] = [py * ps + px, (py // 2) * (ps // 2) + px // 2, (H // 2 + py // 2) * (ps // 2) + px // 2]
    return (src_y, ss, src_c, ss // 2, pred_y, ps, pred_c, ps // 2), jobs


@pytest.mark.gpu
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("njobs", [1, 4, 23])
def test_unit_pred_ssd_is_numpy(hv, bd, njobs):
    """sizes 8 to 64 mixed in one launch, one unit alone, a whole workgroup's four and a count that is no multiple of four"""
    planes, jobs = _ssd_case(70 + njobs, bd, njobs)
    want = CC.unit_ssd(*planes, jobs)
    got = hv.unit_pred_ssd(bd, *planes, jobs)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert (want > 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("bd", [8, 10])
def test_unit_pred_ssd_at_the_extremes(hv, bd):
    """source all 0 against prediction all 2^bd - 1: the largest sums; 64 x 64 at 10 bits is 4096 x 1023^2 > 2^31 and wraps as the reference's int32 does"""
    planes, jobs = _ssd_case(80, bd, 9, extreme=True)
    want = CC.unit_ssd(*planes, jobs)
    got = hv.unit_pred_ssd(bd, *planes, jobs)
    assert np.array_equal(got, want)
    top = (1 << bd) - 1
    k = int(np.flatnonzero(jobs["log2_size"] == 6)[0])
    assert want[k, 0] == CC.i32(4096 * top * top) and (want[k, 0] < 0) == (bd == 10) and want[k, 1] == 1024 * top * top
