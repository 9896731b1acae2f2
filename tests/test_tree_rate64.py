"""The CABAC rate of a 64x64 inter unit's one transform tree on the device: havoc_mi355x_tree_rate at (log2CbSize 6, depth 1) -- the split is inferred above
MaxTbLog2SizeY, so no split_transform_flag bin; cbf_cb, cbf_cr, then per child cbf_cb / cbf_cr, cbf_luma, Y 32x32, Cb and Cr 16x16.

CPU (-m "not gpu"): the plain-Python restatement (tests/tree_rate_tools.tree_rate, which takes L = 6 as it is) against (a) the reference's own Syntax<transform_tree>
through tests/tree_rate_shim.cpp on fresh trees and (b) the committed outputs of that shim (tests/golden/tree_rate64_golden.npz); the made cases, by name.
GPU (-m gpu): the kernel against the golden file and the restatement in every rate, mask and state byte; the refusal of a job that claims a coded split flag; (6, 0).
"""
import collections
import os

import numpy as np
import pytest

import reflibs
import residual_rate_tools as R
import tree_rate_tools as TR
import unit_tree_tools as UT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tree_rate64_golden.npz")
needs_ref = pytest.mark.skipif(TR.reference_dir() is None, reason="reference sources not present (the shim compiles them at test time)")
L, DEPTH = UT.L64, UT.DEPTH64


@pytest.fixture(scope="module")
def golden():
    from turingcodec_amd.havoc import TREE_RATE_JOB_DT
    g = np.load(GOLDEN)
    return dict(luma=g["luma"], chroma=g["chroma"], states=g["states"], syntax=g["syntax"], jobs=g["jobs"].copy().view(TREE_RATE_JOB_DT).reshape(-1),
                aux=g["aux"].copy().view(TR.AUX_DT).reshape(-1), rates=g["rates"], masks=g["masks"], after=g["after"], after_syntax=g["after_syntax"], calls=g["calls"])


@pytest.fixture(scope="module")
def restated(golden):
    """the restatement over the golden trees, computed once: (rates, masks, states after, syntax states after, calls)"""
    g, calls = golden, []
    return TR.walk_jobs(L, DEPTH, g["luma"], g["chroma"], g["states"], g["syntax"], g["jobs"], collections.Counter(), calls) + (calls,)


def _made_cases_reached(masks, jobs, rates, after, after_syntax, states, syntax):
    tags = UT.reached(masks, jobs)
    for name in UT.REQUIRED_CASES:
        assert tags[name] > 0, name
    # the all-zero tree: rate 0, nothing moved; a coded tree costs something
    zero = masks == 0
    assert (rates[zero] == 0).all() and (rates[~zero] > 0).all()
    assert np.array_equal(after[zero], states[jobs["ctx_index"][zero]]) and np.array_equal(after_syntax[zero], syntax[jobs["ctx_index"][zero]])
    return tags


# ------------------------------------------------------------------------------------------------------------------ CPU
@needs_ref
def test_restatement_matches_the_reference_on_fresh_trees():
    """40 trees the golden file has not seen, through the shim as it stands (log2Cb 6, depth 1, MaxTrafoDepth 1, MinTb 2, MaxTb 5): every rate, the mask, all 128 + 4
    state bytes, the sequence of residual_coding calls; the made cases by name"""
    oracle, shim = reflibs.Oracle(), TR.Shim()
    luma, chroma, states, syntax, jobs, aux = UT.make_cases64(oracle, 961, 40)
    assert [tuple(int(v) for v in a) for a in aux] == [UT.ENCODER] * len(aux)
    calls = []
    got = TR.walk_jobs(L, DEPTH, luma, chroma, states, syntax, jobs, collections.Counter(), calls)
    want = shim.walk_jobs(L, DEPTH, luma, chroma, states, syntax, jobs, aux)
    assert np.array_equal(got[0], want[0]), np.flatnonzero(got[0] != want[0])[:8]
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert calls == want[4]
    for j in range(len(jobs)):
        assert want[4][j] == (UT.expected_calls64(int(want[1][j])) if want[1][j] else []), j
    _made_cases_reached(want[1], jobs, want[0], want[2], want[3], states, syntax)
    # no split_transform_flag bin: the syntax snapshot passes through every tree
    assert np.array_equal(want[3], syntax[jobs["ctx_index"]])


def test_restatement_matches_golden(golden, restated):
    g, (rates, masks, after, after_syntax, calls) = golden, restated
    assert len(g["jobs"]) > 192 and os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "tree_rate_golden.npz"))
    assert np.array_equal(rates, g["rates"]) and np.array_equal(masks, g["masks"])
    assert np.array_equal(after, g["after"]) and np.array_equal(after_syntax, g["after_syntax"])
    for j, (job, a) in enumerate(zip(g["jobs"], g["aux"])):
        assert tuple(int(v) for v in a) == UT.ENCODER and job["flags"] == TR.rate_flags(L, *UT.ENCODER) == 0
        want = [tuple(int(v) for v in c) for c in g["calls"][j] if c[2] >= 0]
        assert calls[j] == want and want == (UT.expected_calls64(int(g["masks"][j])) if g["masks"][j] else []), j
    # bytes outside the cbf and residual contexts pass through; the whole syntax snapshot too (no flag bin)
    other = np.setdiff1d(np.arange(128), np.r_[1:7, R.RESIDUAL_BYTES])
    assert np.array_equal(after[:, other], g["states"][g["jobs"]["ctx_index"]][:, other])
    assert np.array_equal(g["after_syntax"], g["syntax"][g["jobs"]["ctx_index"]])
    # several jobs share one snapshot
    assert 3 < len(np.unique(g["jobs"]["ctx_index"][:63])) < 63


def test_golden_trees_reach_the_made_cases(golden):
    g = golden
    tags = _made_cases_reached(g["masks"], g["jobs"], g["rates"], g["after"], g["after_syntax"], g["states"], g["syntax"])
    print({k: tags[k] for k in UT.REQUIRED_CASES})


def test_case_names():
    assert UT.case_names(0, 1) == ["zero_tree"]
    assert UT.case_names(0x005, 0) == ["sdh_off", "luma_only"]
    assert UT.case_names(0x030, 1) == ["sdh_on", "chroma_only", "cb_with_zero_child"]
    assert UT.case_names(0x200, 1) == ["sdh_on", "chroma_only", "cr_without_cb"]
    assert UT.case_names(0xfff, 0) == ["sdh_off", "all_twelve"]
    assert "cb_with_zero_child" not in UT.case_names(0x0f1, 0)


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def hv():
    from turingcodec_amd.havoc import Havoc
    h = Havoc(stream="new")
    yield h
    h.close()


@pytest.mark.gpu
def test_device_matches_golden_and_restatement(hv, golden, restated):
    """launches of 1, 63, 64, 65 jobs and the golden set (a workgroup walks 64 jobs); several jobs share a snapshot in every launch"""
    g, (rates, masks, after, after_syntax, _) = golden, restated
    for njobs in (1, 63, 64, 65, len(g["jobs"])):
        jobs = g["jobs"][:njobs]
        got, got_masks, got_after, got_syntax = hv.tree_rate(L, DEPTH, g["luma"], g["chroma"], g["states"], g["syntax"], jobs)
        assert len(got) == njobs
        assert np.array_equal(got, g["rates"][:njobs]), (njobs, np.flatnonzero(got != g["rates"][:njobs])[:8])
        assert np.array_equal(got, rates[:njobs])
        assert np.array_equal(got_masks, g["masks"][:njobs]) and np.array_equal(got_masks, masks[:njobs])
        assert np.array_equal(got_after, g["after"][:njobs]) and np.array_equal(got_after, after[:njobs])
        assert np.array_equal(got_syntax, g["after_syntax"][:njobs]) and np.array_equal(got_syntax, after_syntax[:njobs])


@pytest.mark.gpu
def test_device_refuses_a_coded_split_flag_and_depth_zero(hv, golden):
    """a 64x64 job with HAVOC_TREE_RATE_SPLIT_FLAG_CODED names a bin the syntax cannot code: refused like an unknown bit beside good jobs -- nothing of it is read,
    rate -1, mask 0, snapshots passed through; (6, 0) is no launch at all"""
    import torch
    from turingcodec_amd.havoc import HavocError
    g = golden
    bad = g["jobs"][:8].copy()
    bad["luma_off"][[1, 5]] = bad["cb_off"][[1, 5]] = bad["cr_off"][[1, 5]] = 1 << 30      # (would fault if read)
    bad["flags"][1], bad["flags"][5] = TR.SPLIT_CODED, 2
    rates, masks, after, after_syntax = hv.tree_rate(L, DEPTH, g["luma"], g["chroma"], g["states"], g["syntax"], bad)
    keep = [0, 2, 3, 4, 6, 7]
    assert (rates[[1, 5]] == -1).all() and (masks[[1, 5]] == 0).all()
    assert np.array_equal(rates[keep], g["rates"][keep]) and np.array_equal(masks[keep], g["masks"][keep]) and (rates[keep] > 0).any()
    assert np.array_equal(after[[1, 5]], g["states"][bad["ctx_index"][[1, 5]]]) and np.array_equal(after_syntax[[1, 5]], g["syntax"][bad["ctx_index"][[1, 5]]])
    assert np.array_equal(after[keep], g["after"][keep]) and np.array_equal(after_syntax[keep], g["after_syntax"][keep])
    with torch.cuda.stream(hv.tstream):
        d = torch.zeros(64, dtype=torch.int64, device=hv.device)
    with pytest.raises(HavocError, match="log2CbSize"):
        hv.tree_rate_d(6, 0, d, d, d, d, d, d, d)
    with pytest.raises(HavocError, match="log2CbSize"):
        hv.tree_rate_d(7, 1, d, d, d, d, d, d, d)
