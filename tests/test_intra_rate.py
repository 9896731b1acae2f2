"""The CABAC rate of a refined intra candidate on the device (havoc_mi355x_intra_rate), its job records (havoc_mi355x_intra_rate_jobs), the decision that uses it
(havoc_mi355x_intra_decide_rated) and the batch client's route through them (havoc_search_intra_device_rated, decisions.intra_device(rates="cabac")).

CPU (-m "not gpu"): the plain-Python restatement tests/intra_rate_tools.candidate_rate against (a) the reference's own Syntax<IntraPartition> under EstimateRateLuma
(tests/intra_rate_shim.cpp, compiled at test time where the reference sources are) on fresh candidates and (b) the committed outputs of that shim
(tests/golden/intra_rate_golden.npz); the branches the golden candidates reach; the libraries' exports; libhavoc_search.so over the stand-in device; the numpy
decideIntraRd against tu_decision.hpp's.  GPU (-m gpu): the kernel against the golden file and the restatement -- every rate, all 128 + 4 state bytes after every
job -- its contract (untouched memory, refusals, graph replay), the job records and the rated decision against numpy, and the client end to end.
"""
import collections
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import intra_rate_tools as I
import reflibs
import residual_rate_tools as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "intra_rate_golden.npz")
needs_ref = pytest.mark.skipif(I.reference_dir() is None, reason="reference sources not present (the shim compiles them at test time)")
SIZES = [2, 3, 4, 5]
MAX_ORDER = 12      # HAVOC_MI355X_INTRA_MAX_ORDER


@pytest.fixture(scope="module")
def golden():
    from turingcodec_amd.havoc import INTRA_RATE_JOB_DT
    g = np.load(GOLDEN)
    return {log2: dict(levels=g[f"l{log2}.levels"], states=g[f"l{log2}.states"], syntax=g[f"l{log2}.syntax"],
                       jobs=g[f"l{log2}.jobs"].copy().view(INTRA_RATE_JOB_DT).reshape(-1), aux=g[f"l{log2}.aux"].copy().view(I.AUX_DT).reshape(-1),
                       rates=g[f"l{log2}.rates"], after=g[f"l{log2}.after"], after_syntax=g[f"l{log2}.after_syntax"]) for log2 in SIZES}


@pytest.fixture(scope="module")
def restated(golden):
    """the restatement over the golden candidates, computed once: {log2: (rates, states after, syntax states after, branch counters)}"""
    out = {}
    for log2, g in golden.items():
        tags = collections.Counter()
        out[log2] = I.walk_jobs(log2, g["levels"], g["states"], g["syntax"], g["jobs"], tags) + (tags,)
    return out


# ------------------------------------------------------------------------------------------------------------------ CPU
@needs_ref
@pytest.mark.parametrize("log2", SIZES)
def test_restatement_matches_the_reference_on_fresh_candidates(log2):
    """about 300 RDOQ blocks per size the golden file has not seen, plus the hand-made ones (all-zero, DC only, a lone level at the last position of the last
    sub-block, the mode in two places of candModeList): the rate of every candidate and all 128 + 4 state bytes it leaves.  The shim is given the mode, the list and
    the kind of unit, not the job's mpm_idx and flags: those are the restatement's own derivation."""
    oracle, shim = reflibs.Oracle(), I.Shim()
    levels, states, syntax, jobs, aux = I.make_cases(oracle, 77 + log2, log2, 300)
    tags = collections.Counter()
    got, got_after, got_syntax = I.walk_jobs(log2, levels, states, syntax, jobs, tags)
    want, want_after, want_syntax, info = shim.walk_jobs(log2, levels, states, syntax, jobs, aux)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert np.array_equal(got_after, want_after) and np.array_equal(got_syntax, want_syntax)
    assert np.array_equal(info[:, 0], jobs["mpm_idx"])
    # MaxTrafoDepth as Syntax<IntraPartition> set it
    assert np.array_equal(info[:, 2], aux["depth_intra"] + aux["split"])
    twice = np.array([list(a["cand"]).count(int(a["mode"])) > 1 for a in aux])
    assert twice.sum() >= 20 and {0, 1} <= set(jobs["mpm_idx"][twice])
    assert not [k for k in I.required_tags(log2) if not tags[k]]
    assert (want > 0).all() and (want_syntax != syntax[jobs["ctx_index"]]).any(axis=1).sum() > 250
    # an all-zero block pays its prefix and cbf_luma = 0 and moves nothing else
    zero = np.flatnonzero([not levels[int(j["level_off"]):int(j["level_off"]) + (1 << 2 * log2)].any() for j in jobs])
    keep = np.r_[0, 3:128]
    assert len(zero) and np.array_equal(want_after[zero][:, keep], states[jobs["ctx_index"][zero]][:, keep])


def test_flag_rule_is_the_librarys():
    """havoc_search_intra_rate_flags (what a caller of the client asks) against the restatement the shim has been held to"""
    from turingcodec_amd import decisions
    for log2 in (2, 3, 4, 5, 6):
        for split in (0, 1):
            for depth in (0, 1, 2):
                for min_tb in (2, 3):
                    for max_tb in (4, 5):
                        assert decisions.intra_rate_flags(log2, split, depth, min_tb, max_tb) == I.rate_flags(log2, split, depth, min_tb, max_tb)
    # the reference encoder's set-up: 2Nx2N partitions of 8, 16, 32 code split_transform_flag at depth 0; the 4x4 partitions of an NxN unit do not, at depth 1
    assert [decisions.intra_rate_flags(log2, log2 == 2) for log2 in SIZES] == [2, 1, 1, 1]


@pytest.mark.parametrize("log2", SIZES)
def test_restatement_matches_golden(golden, restated, log2):
    g, (rates, after, after_syntax, _) = golden[log2], restated[log2]
    assert len(g["jobs"]) >= 257
    assert np.array_equal(rates, g["rates"]) and np.array_equal(after, g["after"]) and np.array_equal(after_syntax, g["after_syntax"])
    # the job records are what the mode, the list and the kind of unit give
    for j, a in zip(g["jobs"], g["aux"]):
        assert j["mpm_idx"] == I.mpm_index(int(a["mode"]), a["cand"]) and j["flags"] == I.rate_flags(log2, a["split"], a["depth_intra"], a["min_tb"], a["max_tb"])
    # bytes outside cbf_luma and the residual contexts pass through
    other = np.setdiff1d(np.arange(128), np.r_[1:3, R.RESIDUAL_BYTES])
    assert np.array_equal(after[:, other], g["states"][g["jobs"]["ctx_index"]][:, other])
    # two jobs share one snapshot
    assert len(np.unique(g["jobs"]["ctx_index"][:63])) < 63


@pytest.mark.parametrize("log2", SIZES)
def test_golden_candidates_reach_every_branch(restated, log2):
    tags = restated[log2][3]
    missing = [k for k in I.required_tags(log2) if not tags[k]]
    assert not missing, missing


def test_libraries_export_the_entry_points():
    from turingcodec_amd import decisions, havoc
    L, names = havoc._load()
    assert L.havoc_mi355x_intra_rate and L.havoc_mi355x_intra_rate_jobs and L.havoc_mi355x_intra_decide_rated
    assert {"intra_rate", "intra_rate_jobs", "intra_decide_rated"} <= set(names)
    assert havoc.INTRA_RATE_JOB_DT.itemsize == 32 and havoc.INTRA_RATE_JOB_DT.fields["mpm_idx"][1] == 14 and havoc.INTRA_SYNTAX_CTX_BYTES == 4
    S = decisions.lib()
    assert S.havoc_search_intra_device_rated and S.havoc_search_intra_rate_flags
    header = open(os.path.join(ROOT, "include", "havoc_mi355x.h")).read()
    for name in ("havoc_mi355x_intra_rate(", "havoc_mi355x_intra_rate_jobs(", "havoc_mi355x_intra_decide_rated(", "HAVOC_INTRA_SYNTAX_CTX_PREV_INTRA_LUMA_PRED_FLAG",
                 "HAVOC_INTRA_SYNTAX_CTX_SPLIT_TRANSFORM_FLAG"):
        assert name in header, name


def test_search_library_loads_over_the_stand_in_device_and_reports_the_missing_route():
    """tests/mock_device.c has none of the three new device entry points: libhavoc_search.so must still load over it with every symbol bound at once (ctypes:
    RTLD_NOW), and only the rated client says so -- HAVOC_SEARCH_ENOTAVAILABLE, before it looks at an argument.  (A process of its own: the stand-in takes the
    device library's place for everything loaded after it.)"""
    code = ("import ctypes as C, os, sys\n"
            f"sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); sys.path.insert(0, {ROOT!r})\n"
            "import search_runner\n"
            "dev = C.CDLL(search_runner.build_mock(), mode=C.RTLD_GLOBAL)\n"
            f"L = C.CDLL({os.path.join(ROOT, 'turingcodec_amd', 'libhavoc_search.so')!r}, mode=os.RTLD_NOW)\n"
            "assert not hasattr(dev, 'havoc_mi355x_intra_rate')\n"
            "assert L.havoc_search_intra_device and L.havoc_search_intra_chain\n"
            "L.havoc_search_intra_device_rated.restype = C.c_int\n"
            "print(L.havoc_search_intra_device_rated(*([None] * 11), C.c_double(1), C.c_double(1), C.c_double(1), 1, None))\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    from turingcodec_amd import decisions
    assert int(out.stdout.strip().splitlines()[-1]) == decisions.SEARCH_ENOTAVAILABLE == -200


def _random_partitions(seed, n, full=False):
    """n partitions with 1..12 candidates each: order, count, slot (slots handed out in a shuffled order, as the device's atomic counter may), outcomes per slot"""
    rng = np.random.default_rng(seed)
    count = rng.integers(1, MAX_ORDER + 1, n).astype(np.int32)
    count[0] = 1
    count[-1] = MAX_ORDER if n > 1 or full else count[-1]
    order = np.zeros((n, MAX_ORDER), np.int32)
    for i in range(n):
        order[i, :count[i]] = rng.permutation(35)[:count[i]]
    slot = np.zeros(n, np.int32)
    perm = rng.permutation(n)
    slot[perm] = np.concatenate([[0], np.cumsum(count[perm])[:-1]])
    m = int(count.sum())
    cbf = (rng.integers(0, 40, m) * (rng.random(m) < 0.7)).astype(np.int32)
    nonzero = np.where(cbf != 0, rng.integers(1, 30, m), 0).astype(np.int32)
    stats = np.stack([nonzero, nonzero * rng.integers(1, 4, m)], 1).astype(np.int32)
    ssd = rng.integers(0, 60000, m).astype(np.uint32)
    return order, count, slot, cbf, ssd, stats


def test_numpy_decide_intra_rated_is_tu_decision_hpp():
    """decide_intra_rated against search/tu_decision.hpp's decideIntraRd with a rate functor (tests/intra_rated_client.cpp, compiled here): the restatement is
    pinned before it judges the device.  Ties: the first of equal costs wins.  A challenger whose distortion alone is not below the champion's cost is not measured
    by the reference (Search.hpp:242-246): with that short cut the champion and its cost are the same."""
    client = I.DecisionClient()
    order, count, slot, cbf, ssd, stats = _random_partitions(5, 600)
    rng = np.random.default_rng(6)
    rates = rng.integers(0, 1 << 24, len(ssd)).astype(np.int64)
    rl = 4321
    # ties: in every fourth partition with more than two candidates, the last candidate gets the cost of the first -- and two of them share the minimum
    for i in np.flatnonzero(count > 2)[::4]:
        a, b = int(slot[i]), int(slot[i]) + int(count[i]) - 1
        ssd[b], rates[b] = ssd[a], rates[a]
    for i in np.flatnonzero(count > 2)[::8]:
        a, b = int(slot[i]), int(slot[i]) + int(count[i]) - 1
        ssd[[a, b]], rates[[a, b]] = 0, 0
    got = I.decide_intra_rated(order, count, slot, cbf, ssd, rates, rl)
    for like_ref in (False, True):
        want = client.decide(order, count, slot, ssd, rates, rl, like_ref)
        assert np.array_equal(got["mode"], want[:, 0]) and np.array_equal(got["index"], want[:, 1]) and np.array_equal(got["cost"], want[:, 3])
        assert np.array_equal(want[:, 2], count)
        assert (want[:, 4] > 0).any() == like_ref
    tied = np.flatnonzero(count > 2)[::8]
    assert (got["index"][tied] == 0).all() and (got["index"] > 0).any()


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


def _torch_i64(hv, a):
    import torch
    with torch.cuda.stream(hv.tstream):
        return torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(hv.device)


@pytest.mark.gpu
@pytest.mark.parametrize("log2", SIZES)
def test_device_matches_golden_and_restatement(hv, golden, restated, log2):
    """launches of 1, 63, 64, 65 jobs and the golden set (a workgroup walks 64 jobs: where the transposed copy of the states can go wrong); several jobs share a
    snapshot in every launch"""
    g, (rates, after, after_syntax, _) = golden[log2], restated[log2]
    for njobs in (1, 63, 64, 65, len(g["jobs"])):
        jobs = g["jobs"][:njobs]
        got, got_after, got_syntax = hv.intra_rate(log2, g["levels"], g["states"], g["syntax"], jobs)
        assert len(got) == njobs
        assert np.array_equal(got, g["rates"][:njobs]), (njobs, np.flatnonzero(got != g["rates"][:njobs])[:8])
        assert np.array_equal(got, rates[:njobs])
        assert np.array_equal(got_after, g["after"][:njobs]) and np.array_equal(got_after, after[:njobs])
        assert np.array_equal(got_syntax, g["after_syntax"][:njobs]) and np.array_equal(got_syntax, after_syntax[:njobs])
    assert len(np.unique(g["jobs"]["ctx_index"][:63])) < 63 and len(np.unique(g["jobs"]["ctx_index"][:63])) > 3


@pytest.mark.gpu
def test_device_contract(hv, golden):
    """NULL outputs give the same rates; neither input table is written; guard bytes around every output are untouched; a graph replays with new levels in place"""
    import torch
    log2 = 3
    g = golden[log2]
    jobs = g["jobs"][:130].copy()
    pad = 64
    jobs["level_off"] += pad
    jobs["rate_index"] += 5
    nr, nl = 130 + 5, 130 * 64 + pad
    levels = np.full(nl + pad, 12345, np.int16)
    levels[pad:nl] = g["levels"][:nl - pad]
    d_levels, d_states, d_syntax, d_jobs = hv.up(levels), _torch_u8(hv, g["states"]), _torch_u8(hv, g["syntax"]), _torch_u8(hv, jobs)
    with torch.cuda.stream(hv.tstream):
        d_rates = torch.full((nr + 7,), -77, dtype=torch.int64, device=hv.device)
        d_rates2 = torch.full((nr + 7,), -77, dtype=torch.int64, device=hv.device)
        d_after = torch.full((64 + 130 * 128 + 64,), 201, dtype=torch.uint8, device=hv.device)
        d_after_syntax = torch.full((64 + 130 * 4 + 64,), 202, dtype=torch.uint8, device=hv.device)
    hv.intra_rate_d(log2, d_levels, d_states, d_syntax, d_jobs, d_rates, d_after[64:], d_after_syntax[64:])
    hv.intra_rate_d(log2, d_levels, d_states, d_syntax, d_jobs, d_rates2, None, None)
    rates, rates2 = hv.down(d_rates, np.int64), hv.down(d_rates2, np.int64)
    assert np.array_equal(rates[5:nr], g["rates"][:130]) and np.array_equal(rates2, rates)
    assert (rates[:5] == -77).all() and (rates[nr:] == -77).all()
    assert np.array_equal(hv.down(d_levels, np.int16), levels)
    assert np.array_equal(hv.down(d_states, np.uint8), g["states"].reshape(-1)) and np.array_equal(hv.down(d_syntax, np.uint8), g["syntax"].reshape(-1))
    assert np.array_equal(hv.down(d_jobs, np.uint8), jobs.view(np.uint8).reshape(-1))
    after, after_syntax = hv.down(d_after, np.uint8), hv.down(d_after_syntax, np.uint8)
    assert np.array_equal(after[64:64 + 130 * 128].reshape(-1, 128), g["after"][:130]) and (after[:64] == 201).all() and (after[64 + 130 * 128:] == 201).all()
    assert np.array_equal(after_syntax[64:64 + 130 * 4].reshape(-1, 4), g["after_syntax"][:130])
    assert (after_syntax[:64] == 202).all() and (after_syntax[64 + 130 * 4:] == 202).all()
    # the same launch from a captured graph, replayed twice, the second time with other levels in the same buffer
    graph = hv.graph_capture(lambda: hv.intra_rate_d(log2, d_levels, d_states, d_syntax, d_jobs, d_rates, d_after[64:], d_after_syntax[64:]))
    other = levels.copy()
    other[pad:nl] = g["levels"][127 * 64:257 * 64]
    want2 = I.walk_jobs(log2, other, g["states"], g["syntax"], jobs)
    for k, (lv, want) in enumerate(((levels, (rates[:nr], g["after"][:130], g["after_syntax"][:130])), (other, want2))):
        with torch.cuda.stream(hv.tstream):
            d_levels.copy_(torch.from_numpy(lv))
            d_rates.fill_(-77)
            d_after.fill_(201)
            d_after_syntax.fill_(202)
        hv.graph_launch(graph)
        got = hv.down(d_rates, np.int64)
        assert np.array_equal(got[5:nr], want[0][5:nr]) and (got[:5] == -77).all() and (got[nr:] == -77).all(), k
        assert np.array_equal(hv.down(d_after, np.uint8)[64:64 + 130 * 128].reshape(-1, 128), want[1])
        assert np.array_equal(hv.down(d_after_syntax, np.uint8)[64:64 + 130 * 4].reshape(-1, 4), want[2])
    assert not np.array_equal(want2[0][5:nr], rates[5:nr])
    hv.graph_destroy(graph)


@pytest.mark.gpu
def test_device_refusals(hv, golden):
    import torch
    from turingcodec_amd.havoc import HavocError
    g = golden[4]
    jobs = g["jobs"][:8].copy()
    d_levels, d_states, d_syntax, d_jobs = hv.up(g["levels"]), _torch_u8(hv, g["states"]), _torch_u8(hv, g["syntax"]), _torch_u8(hv, jobs)
    with torch.cuda.stream(hv.tstream):
        d_rates = torch.zeros(64, dtype=torch.int64, device=hv.device)
    for log2 in (1, 6):
        with pytest.raises(HavocError, match="log2TrafoSize"):
            hv.intra_rate_d(log2, d_levels, d_states, d_syntax, d_jobs, d_rates)
    for args in ((None, d_states, d_syntax, d_jobs, d_rates), (d_levels, None, d_syntax, d_jobs, d_rates), (d_levels, d_states, None, d_jobs, d_rates),
                 (d_levels, d_states, d_syntax, d_jobs, None)):
        with pytest.raises(HavocError, match="null"):
            hv.intra_rate_d(4, *args)
    p = [t.data_ptr() for t in (d_levels, d_states, d_syntax, d_jobs, d_rates)]
    with pytest.raises(HavocError, match="null"):
        hv._ck(hv.L.havoc_mi355x_intra_rate(hv.h, 4, p[0], p[1], p[2], None, 1, p[4], None, None))
    with pytest.raises(HavocError, match="njobs"):
        hv._ck(hv.L.havoc_mi355x_intra_rate(hv.h, 4, p[0], p[1], p[2], p[3], -1, p[4], None, None))
    with pytest.raises(HavocError, match="aligned"):
        hv._ck(hv.L.havoc_mi355x_intra_rate(hv.h, 4, p[0] + 2, p[1], p[2], p[3], 8, p[4], None, None))
    with pytest.raises(HavocError, match="aligned"):
        hv._ck(hv.L.havoc_mi355x_intra_rate(hv.h, 4, p[0], p[1], p[2], p[3], 8, p[4] + 4, None, None))
    with pytest.raises(HavocError, match="d_states_out"):
        hv.intra_rate_d(4, d_levels, d_states, d_syntax, d_jobs, d_rates, d_states, None)
    with pytest.raises(HavocError, match="d_syntax_states_out"):
        hv.intra_rate_d(4, d_levels, d_states, d_syntax, d_jobs, d_rates, None, d_syntax)
    # jobs the entry point excludes: nothing of them is walked, their rate is -1, their snapshots pass through; the good jobs beside them are priced
    bad = g["jobs"][:8].copy()
    bad["level_off"][[1, 2, 3]] = 1 << 30      # (would fault if read)
    bad["mpm_idx"][1], bad["scan_idx"][2], bad["scan_idx"][3] = 4, 3, 1      # (scan 1 with 16x16 blocks)
    rates, after, after_syntax = hv.intra_rate(4, g["levels"], g["states"], g["syntax"], bad)
    want = I.walk_jobs(4, g["levels"], g["states"], g["syntax"], bad)
    assert np.array_equal(rates, want[0]) and np.array_equal(after, want[1]) and np.array_equal(after_syntax, want[2])
    assert (rates[1:4] == -1).all() and rates[0] > 0 and (rates[4:] > 0).all()
    assert np.array_equal(after[1:4], g["states"][bad["ctx_index"][1:4]]) and np.array_equal(after_syntax[1:4], g["syntax"][bad["ctx_index"][1:4]])
    # split_transform_flag said to be coded for a 4x4 block
    g2 = golden[2]
    bad = g2["jobs"][:3].copy()
    bad["flags"][1] |= 1
    bad["level_off"][1] = 1 << 30
    rates, after, after_syntax = hv.intra_rate(2, g2["levels"], g2["states"], g2["syntax"], bad)
    assert rates[1] == -1 and np.array_equal(rates[[0, 2]], g2["rates"][[0, 2]]) and np.array_equal(after_syntax[1], g2["syntax"][bad["ctx_index"][1]])
    assert np.array_equal(after[1], g2["states"][bad["ctx_index"][1]])


def _numpy_rate_jobs(mpm, order, count, slot, rdoq_jobs, flags):
    """the records havoc_mi355x_intra_rate_jobs writes, from the same tables"""
    from turingcodec_amd.havoc import INTRA_RATE_JOB_DT
    out = np.zeros(len(rdoq_jobs), INTRA_RATE_JOB_DT)
    for i in range(len(count)):
        for k in range(int(count[i])):
            c = int(slot[i]) + k
            j, r = out[c], rdoq_jobs[c]
            j["level_off"], j["ctx_index"], j["rate_index"], j["scan_idx"], j["sdh"] = r["dst_off"], r["ctx_index"], c, r["scan_idx"], r["sdh"]
            j["mpm_idx"], j["flags"] = I.mpm_index(int(order[i, k]), mpm[i]["cand_mode_list"]), flags
    return out


@pytest.mark.gpu
def test_intra_rate_jobs_is_the_numpy_build(hv):
    from turingcodec_amd.decisions import INTRA_CTX_DT
    from turingcodec_amd.havoc import INTRA_RATE_JOB_DT, RDOQ_JOB_DT, HavocError
    n = 300
    order, count, slot, _, _, _ = _random_partitions(12, n)
    assert count[0] == 1 and count[-1] == MAX_ORDER
    rng = np.random.default_rng(13)
    mpm = np.zeros(n, INTRA_CTX_DT)
    mpm["cand_mode_list"] = np.argsort(rng.random((n, 35)), axis=1)[:, :3]
    for i in range(0, n, 3):                          # a candidate of the partition is in the list ...
        mpm["cand_mode_list"][i, i % 3] = order[i, rng.integers(0, count[i])]
    mpm["cand_mode_list"][-1, 1] = mpm["cand_mode_list"][-1, 2] = order[-1, 5]      # ... and one is there twice: the first place counts
    m = int(count.sum())
    rj = np.zeros(m, RDOQ_JOB_DT)
    rj["dst_off"], rj["ctx_index"] = rng.permutation(m) * 64, rng.integers(0, 50, m)
    rj["scan_idx"], rj["sdh"] = rng.integers(0, 3, m), rng.integers(0, 2, m)
    d = [hv.up(np.ascontiguousarray(mpm).view(np.int32)), hv.up(order), hv.up(count), hv.up(slot), _torch_u8(hv, rj)]
    for flags in (0, 3):
        d_out = _torch_u8(hv, np.full(m * 32 + 64, 203, np.uint8))
        hv.intra_rate_jobs_d(*d, n, flags, d_out[32:])
        got = hv.down(d_out, np.uint8)
        assert (got[:32] == 203).all() and (got[32 + m * 32:] == 203).all()
        want = _numpy_rate_jobs(mpm, order, count, slot, rj, flags)
        assert got[32:32 + m * 32].tobytes() == want.tobytes()
    assert want["mpm_idx"][int(slot[-1]) + 5] == 1 and set(np.unique(want["mpm_idx"])) == {0, 1, 2, 3}
    assert np.array_equal(hv.down(d[4], np.uint8), rj.view(np.uint8).reshape(-1))
    assert INTRA_RATE_JOB_DT.itemsize == 32
    with pytest.raises(HavocError, match="flags"):
        hv.intra_rate_jobs_d(*d, n, 4, d_out)
    with pytest.raises(HavocError, match="null"):
        hv.intra_rate_jobs_d(d[0], None, d[2], d[3], d[4], n, 0, d_out)


def _device_decide(hv, mpm, order, count, slot, cbf, ssd, stats, rates, log2, rl):
    """havoc_mi355x_intra_decide (rates None) / _rated -> (INTRA_RD_RESULT_DT records, final jobs int32 [n, 4])"""
    from turingcodec_amd.decisions import INTRA_RD_RESULT_DT
    n, m = len(count), len(cbf)
    tj = np.stack([np.arange(m) * 7, np.arange(m) * 11 + 1, np.arange(m) * 13 + 2, np.full(m, -5)], 1).astype(np.int32)
    d = [hv.up(np.ascontiguousarray(mpm).view(np.int32)), hv.up(order), hv.up(count), hv.up(slot), hv.up(cbf), hv.up(ssd)]
    d_stats = hv.up(stats) if stats is not None else None
    d_tj, d_out, d_fin = hv.up(tj), hv.zeros(n * 10, np.int32), hv.zeros(n * 4, np.int32)
    if rates is None:
        hv._ck(hv.L.havoc_mi355x_intra_decide(hv.h, *[t.data_ptr() for t in d], d_stats.data_ptr(), d_tj.data_ptr(), n, log2, rl, d_out.data_ptr(), d_fin.data_ptr()))
    else:
        hv.intra_decide_rated_d(*d, d_stats, _torch_i64(hv, rates), d_tj, n, log2, rl, d_out, d_fin)
    return hv.down(d_out, np.int32).view(INTRA_RD_RESULT_DT).copy(), hv.down(d_fin, np.int32).reshape(-1, 4).copy(), tj


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_rated_decision_with_arbitrary_rates_is_the_numpy_restatement(hv, n):
    from turingcodec_amd.decisions import INTRA_CTX_DT
    order, count, slot, cbf, ssd, stats = _random_partitions(20 + n, n, full=True)
    rng = np.random.default_rng(n)
    rates = rng.integers(0, 1 << 26, len(cbf)).astype(np.int64)
    for i in np.flatnonzero(count > 2)[::3]:          # ties: the first wins
        a, b = int(slot[i]), int(slot[i]) + int(count[i]) - 1
        ssd[[a, b]], rates[[a, b]] = 0, 0
    mpm = np.zeros(n, INTRA_CTX_DT)
    rl, log2 = 40000, 3
    for with_stats in (True, False):
        got, fin, tj = _device_decide(hv, mpm, order, count, slot, cbf, ssd, stats if with_stats else None, rates, log2, rl)
        want = I.decide_intra_rated(order, count, slot, cbf, ssd, rates, rl, stats if with_stats else None)
        assert got.tobytes() == want.tobytes()
        for i in range(n):                            # the final job: the champion's, reconstructing into block i
            assert list(fin[i]) == list(tj[int(slot[i]) + int(want["index"][i])][:3]) + [i << (2 * log2)]


@pytest.mark.gpu
def test_rated_decision_with_the_stand_ins_numbers_is_the_stand_in_path(hv):
    from turingcodec_amd.decisions import INTRA_CTX_DT
    n = 700
    order, count, slot, cbf, ssd, stats = _random_partitions(31, n)
    rng = np.random.default_rng(32)
    mpm = np.zeros(n, INTRA_CTX_DT)
    for i in range(n):
        mpm["cand_mode_list"][i] = rng.permutation(order[i, :count[i]].tolist() + [int(v) for v in rng.integers(0, 35, 3)])[:3]
    mpm["rate_a_minus_c"], mpm["rate_b_minus_c"] = -rng.integers(300000, 420000, n), -rng.integers(100000, 200000, n)
    rates = I.stand_in_rates(mpm, order, count, slot, cbf, stats)
    a, fa, _ = _device_decide(hv, mpm, order, count, slot, cbf, ssd, stats, None, 4, 54321)
    b, fb, _ = _device_decide(hv, mpm, order, count, slot, cbf, ssd, stats, rates, 4, 54321)
    assert a.tobytes() == b.tobytes() and fa.tobytes() == fb.tobytes()
    assert (a["index"] > 0).any() and (a["index"] == 0).any() and (rates < 0).any()


# ---- the client end to end: a small region with partitions of all four sizes ---------------------------------------------------------------------------
REGION_SEED = 3
BD, QP, PAD = 8, 32, 96


@pytest.fixture(scope="module")
def region(hv):
    """128 x 64 samples: 64 x 64 of the synthetic clip the benchmark encodes, a flat 32 x 64 block and a noisy one; the intra partitions workload.intra_partitions
    lays over two CTUs (all four sizes), one CABAC snapshot (128 + 4 bytes) per CTU"""
    from turingcodec_amd import decisions, workload
    rng = np.random.default_rng(REGION_SEED)
    W, H = 128, 64
    plane = np.zeros((H, W), np.uint8)
    plane[:, :64] = workload.synth_frames(64, 64, 1, REGION_SEED, BD)[0][0]
    plane[:, 64:96] = 117
    plane[:, 96:] = rng.integers(0, 256, (H, 32))
    src2d = workload.pad_plane(plane, PAD)
    lam = workload.picture_lambda(QP)
    r = dict(W=W, H=H, stride=src2d.shape[1], host_src=np.ascontiguousarray(src2d.ravel()), lam=lam, rsl=float(1.0 / np.sqrt(lam)), quant=decisions.rqt_quant(QP, BD),
             states=rng.integers(0, 126, (2, 128)).astype(np.uint8), syntax=rng.integers(0, 126, (2, 4)).astype(np.uint8), parts={})
    r["d_src"], r["d_states"], r["d_syntax"] = hv.up(r["host_src"]), _torch_u8(hv, r["states"]), _torch_u8(hv, r["syntax"])
    for log2, (jobs, nb, ictx, ctu) in workload.intra_partitions(src2d, W, H, PAD, REGION_SEED + 31).items():
        r["parts"][log2] = dict(jobs=jobs, nb=nb, ictx=ictx, ctu=ctu, d_jobs=hv.up(jobs), d_nb=hv.up(nb), d_ictx=hv.up(np.ascontiguousarray(ictx).view(np.int32)),
                                d_ctu=hv.up(np.ascontiguousarray(ctu, np.int32)), d_rec=hv.zeros(len(jobs) << (2 * log2), np.uint8))
    return r


def _q16(v):
    return int(v * 65536 + 0.5)      # search/decision.hpp: Lambda::set


def _candidates(hv, r, log2):
    """the client's chain up to the candidates' outcomes, launch by launch through the C ABI: -> the tables and outcomes on the host"""
    from turingcodec_amd.havoc import RDOQ_JOB_DT, rdoq_lambda
    g = r["parts"][log2]
    n, nn, tr = len(g["jobs"]), 1 << log2, 1 if log2 == 2 else 0
    qs, qshift, inv, dshift = [int(v) for v in r["quant"][log2 - 2]]
    lq, sf = rdoq_lambda(r["lam"], inv)
    d_cost, d_order, d_count, d_slot, d_total = hv.zeros(n * 35, np.int32), hv.zeros(n * MAX_ORDER, np.int32), hv.zeros(n, np.int32), hv.zeros(n, np.int32), hv.zeros(2, np.int32)
    hv.intra_satd35_d(BD, log2, r["d_src"], r["stride"], g["d_nb"], g["d_jobs"], d_cost)
    hv._ck(hv.L.havoc_mi355x_intra_order(hv.h, d_cost.data_ptr(), g["d_ictx"].data_ptr(), n, _q16(r["rsl"]), d_order.data_ptr(), d_count.data_ptr(), d_slot.data_ptr(),
                                         d_total.data_ptr()))
    total = hv.down(d_total, np.int32)
    assert total[1] == 0
    m = int(total[0])
    d_ij, d_tj, d_rj, d_sj, d_owner = hv.zeros(m * 8, np.int32), hv.zeros(m * 4, np.int32), _torch_u8(hv, np.zeros(m, RDOQ_JOB_DT)), hv.zeros(2 * m, np.int32), hv.zeros(m, np.int32)
    hv._ck(hv.L.havoc_mi355x_intra_expand(hv.h, g["d_jobs"].data_ptr(), d_order.data_ptr(), d_count.data_ptr(), d_slot.data_ptr(), g["d_ctu"].data_ptr(), n, log2, qs, qshift,
                                          inv, lq, sf, 1, d_ij.data_ptr(), d_tj.data_ptr(), d_rj.data_ptr(), d_sj.data_ptr(), d_owner.data_ptr()))
    d_pred, d_piece = hv.zeros(m * nn * nn, np.uint8), hv.zeros(m * nn * nn, np.uint8)
    d_coef, d_level, d_cbf, d_ssd, d_stats = hv.zeros(m * nn * nn, np.int16), hv.zeros(m * nn * nn, np.int16), hv.zeros(m, np.int32), hv.zeros(m, np.int32), hv.zeros(2 * m, np.int32)
    hv.intra_d(BD, log2, d_pred, nn, g["d_nb"], d_ij.view(-1, 8))
    hv.tu_forward_d(BD, tr, log2, d_coef, r["d_src"], r["stride"], d_pred, nn, d_tj.view(-1, 4))
    hv.rdoq_d(BD, log2, d_level, d_coef, r["d_states"], d_rj, d_cbf, hv.rdoq_workspace(m))
    hv.tu_reconstruct_d(BD, tr, log2, inv, dshift, d_piece, nn, d_pred, nn, r["d_src"], r["stride"], d_level, d_tj.view(-1, 4), d_ssd)
    hv.level_stats_d(d_level, d_sj, m, d_stats)
    return dict(n=n, m=m, order=hv.down(d_order, np.int32).reshape(n, MAX_ORDER), count=hv.down(d_count, np.int32), slot=hv.down(d_slot, np.int32),
                rdoq_jobs=hv.down(d_rj, np.uint8).view(RDOQ_JOB_DT).copy(), levels=hv.down(d_level, np.int16), cbf=hv.down(d_cbf, np.int32),
                ssd=hv.down(d_ssd, np.int32).view(np.uint32), stats=hv.down(d_stats, np.int32).reshape(-1, 2), piece=hv.down(d_piece, np.uint8),
                d=(d_order, d_count, d_slot, d_rj))


@pytest.mark.gpu
def test_client_with_cabac_rates_end_to_end(hv, region):
    """decisions.intra_device(rates="cabac"): champions, costs and reconstructions are the numpy decision over the device's own cbf / ssd and the RESTATED rates of the
    device's own levels; the rates change champions; the default route gives what it gave (the stand-in decision over the same outcomes)"""
    from turingcodec_amd import decisions
    from turingcodec_amd.havoc import INTRA_RATE_JOB_DT
    r = region
    assert sorted(r["parts"]) == SIZES
    groups = [dict(log2=log2, n=len(g["jobs"]), d_nb=g["d_nb"].data_ptr(), d_jobs=g["d_jobs"].data_ptr(), d_ictx=g["d_ictx"].data_ptr(), d_ctu=g["d_ctu"].data_ptr(),
                   d_rec=g["d_rec"].data_ptr()) for log2, g in sorted(r["parts"].items(), reverse=True)]
    args = (hv.h, 1, BD, r["d_src"].data_ptr(), r["stride"], groups, r["d_states"].data_ptr(), r["quant"], r["rsl"], r["lam"], 1.0 / r["lam"])
    plain, st_plain = decisions.intra_device(*args)
    plain_rec = {log2: hv.down(g["d_rec"], np.uint8).copy() for log2, g in r["parts"].items()}
    rated, st_rated = decisions.intra_device(*args, rates="cabac", d_syntax_states=r["d_syntax"].data_ptr())
    assert st_rated.launches == st_plain.launches + 4 and st_rated.candidates == st_plain.candidates
    with pytest.raises(ValueError):
        decisions.intra_device(*args, rates="cabac")
    with pytest.raises(ValueError):
        decisions.intra_device(*args, d_syntax_states=r["d_syntax"].data_ptr())
    rl, differ = _q16(1.0 / r["lam"]), 0
    for log2, g in r["parts"].items():
        c = _candidates(hv, r, log2)
        n, nn2 = c["n"], 1 << 2 * log2
        flags = decisions.intra_rate_flags(log2, log2 == 2)
        jobs = _numpy_rate_jobs(g["ictx"], c["order"], c["count"], c["slot"], c["rdoq_jobs"], flags)
        # the device's records for these tables
        d_jobs = _torch_u8(hv, np.zeros(c["m"], INTRA_RATE_JOB_DT))
        hv.intra_rate_jobs_d(g["d_ictx"], *c["d"], n, flags, d_jobs)
        assert hv.down(d_jobs, np.uint8).tobytes() == jobs.tobytes()
        rates, _, _ = I.walk_jobs(log2, c["levels"], r["states"], r["syntax"], jobs)
        assert (rates > 0).all()
        want = I.decide_intra_rated(c["order"], c["count"], c["slot"], c["cbf"], c["ssd"], rates, rl)
        assert rated[log2].tobytes() == want.tobytes(), log2
        rec = hv.down(g["d_rec"], np.uint8)
        for i in range(n):
            s = int(c["slot"][i]) + int(want["index"][i])
            assert np.array_equal(rec[i * nn2:(i + 1) * nn2], c["piece"][s * nn2:(s + 1) * nn2]), (log2, i)
        # the default route: the stand-in decision over the same outcomes, as before
        base = I.decide_intra_rated(c["order"], c["count"], c["slot"], c["cbf"], c["ssd"], I.stand_in_rates(g["ictx"], c["order"], c["count"], c["slot"], c["cbf"], c["stats"]),
                                    rl, c["stats"])
        assert plain[log2].tobytes() == base.tobytes(), log2
        for i in range(n):
            s = int(c["slot"][i]) + int(base["index"][i])
            assert np.array_equal(plain_rec[log2][i * nn2:(i + 1) * nn2], c["piece"][s * nn2:(s + 1) * nn2]), (log2, i)
        differ += int((want["mode"] != base["mode"]).sum())
    print("partitions", sum(len(g["jobs"]) for g in r["parts"].values()), "whose champion differs with the reference's bits:", differ)
    assert differ >= 1
