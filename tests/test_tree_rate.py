"""The CABAC rate of an inter unit's whole transform tree on the device (havoc_mi355x_tree_rate): split_transform_flag, cbf_cb, cbf_cr, cbf_luma and the Y, Cb and Cr
residual_coding of both depths, one CABAC state running through them.

CPU (-m "not gpu"): the plain-Python restatement tests/tree_rate_tools.tree_rate against (a) the reference's own Syntax<transform_tree> / Syntax<transform_unit> under
EstimateRate<void> over coded data its own CodedData functions fill (tests/tree_rate_shim.cpp, compiled at test time where the reference sources are) on fresh trees
and (b) the committed outputs of that shim (tests/golden/tree_rate_golden.npz); the residual_coding calls the syntax reaches, which pin the job layout; the branches
the trees reach; the library surface.  GPU (-m gpu): the kernel against the golden file and the restatement -- every rate, every mask, all 128 + 4 state bytes after
every job -- and its contract (untouched memory, refusals, graph replay).
"""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

import reflibs
import residual_rate_tools as R
import tree_rate_tools as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tree_rate_golden.npz")
needs_ref = pytest.mark.skipif(TR.reference_dir() is None, reason="reference sources not present (the shim compiles them at test time)")
UNITS = TR.UNITS
unit_ids = [f"L{L}-depth{d}" for L, d in UNITS]


@pytest.fixture(scope="module")
def golden():
    from turingcodec_amd.havoc import TREE_RATE_JOB_DT
    g = np.load(GOLDEN)
    out = {}
    for L, d in UNITS:
        k = f"l{L}d{d}"
        out[L, d] = dict(luma=g[k + ".luma"], chroma=g[k + ".chroma"], states=g[k + ".states"], syntax=g[k + ".syntax"],
                         jobs=g[k + ".jobs"].copy().view(TREE_RATE_JOB_DT).reshape(-1), aux=g[k + ".aux"].copy().view(TR.AUX_DT).reshape(-1),
                         rates=g[k + ".rates"], masks=g[k + ".masks"], after=g[k + ".after"], after_syntax=g[k + ".after_syntax"], calls=g[k + ".calls"])
    return out


@pytest.fixture(scope="module")
def restated(golden):
    """the restatement over the golden trees, computed once: {(L, depth): (rates, masks, states after, syntax states after, branch counters, calls)}"""
    out = {}
    for (L, d), g in golden.items():
        tags, calls = collections.Counter(), []
        out[L, d] = TR.walk_jobs(L, d, g["luma"], g["chroma"], g["states"], g["syntax"], g["jobs"], tags, calls) + (tags, calls)
    return out


def _expected_calls(L, depth, mask):
    """the residual_coding calls of a coded tree in the syntax's order, from the header's description of the job layout alone: (x0, y0, log2, cIdx, cbf)"""
    if depth == 0:
        c = max(L - 1, 2)
        return [(0, 0, L, 0, mask & 1), (0, 0, c, 1, mask >> 4 & 1), (0, 0, c, 2, mask >> 8 & 1)]
    out, half = [], 1 << (L - 1)
    for k in range(4):
        x0, y0 = (k & 1) * half, (k >> 1) * half
        out.append((x0, y0, L - 1, 0, mask >> k & 1))
        if L > 3:
            out += [(x0, y0, L - 2, 1, mask >> (4 + k) & 1), (x0, y0, L - 2, 2, mask >> (8 + k) & 1)]
        elif k == 3:      # an 8x8 unit: its one 4x4 Cb and Cr block, after child 3 only, at the parent's origin
            out += [(0, 0, 2, 1, mask >> 4 & 1), (0, 0, 2, 2, mask >> 8 & 1)]
    return out


# ------------------------------------------------------------------------------------------------------------------ CPU
@needs_ref
@pytest.mark.parametrize("L,depth", UNITS, ids=unit_ids)
def test_restatement_matches_the_reference_on_fresh_trees(L, depth):
    """120 trees per unit size and depth the golden file has not seen: the rate and mask of every tree, all 128 + 4 state bytes it leaves, and the sequence of
    residual_coding calls.  The shim is given MaxTrafoDepth and the transform size limits, not the job's flags: those are the restatement's own derivation."""
    oracle, shim = reflibs.Oracle(), TR.Shim()
    luma, chroma, states, syntax, jobs, aux = TR.make_cases(oracle, 90 + 10 * L + depth, L, depth, 120)
    tags, calls = collections.Counter(), []
    got = TR.walk_jobs(L, depth, luma, chroma, states, syntax, jobs, tags, calls)
    want = shim.walk_jobs(L, depth, luma, chroma, states, syntax, jobs, aux)
    assert np.array_equal(got[0], want[0]), np.flatnonzero(got[0] != want[0])[:8]
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert calls == want[4]
    for j in range(len(jobs)):
        assert want[4][j] == (_expected_calls(L, depth, int(want[1][j])) if want[1][j] else []), j
    assert not [k for k in TR.required_tags(L, depth) if not tags[k]]
    # an all-zero tree: rate 0, no byte moved; a coded tree costs something
    zero = want[1] == 0
    assert zero.any() and (want[0][zero] == 0).all() and (want[0][~zero] > 0).all()
    assert np.array_equal(want[2][zero], states[jobs["ctx_index"][zero]]) and np.array_equal(want[3][zero], syntax[jobs["ctx_index"][zero]])


@pytest.mark.parametrize("L,depth", UNITS, ids=unit_ids)
def test_restatement_matches_golden(golden, restated, L, depth):
    g, (rates, masks, after, after_syntax, _, calls) = golden[L, depth], restated[L, depth]
    assert len(g["jobs"]) >= 257
    assert np.array_equal(rates, g["rates"]) and np.array_equal(masks, g["masks"])
    assert np.array_equal(after, g["after"]) and np.array_equal(after_syntax, g["after_syntax"])
    for j, (job, a) in enumerate(zip(g["jobs"], g["aux"])):
        assert job["flags"] == TR.rate_flags(L, int(a["max_trafo_depth"]), int(a["min_tb"]), int(a["max_tb"]))
        want = [tuple(int(v) for v in c) for c in g["calls"][j] if c[2] >= 0]
        assert calls[j] == want and want == (_expected_calls(L, depth, int(g["masks"][j])) if g["masks"][j] else []), j
    # bytes outside the cbf and residual contexts pass through; prev_intra_luma_pred_flag's byte of the syntax snapshot too
    other = np.setdiff1d(np.arange(128), np.r_[1:7, R.RESIDUAL_BYTES])
    assert np.array_equal(after[:, other], g["states"][g["jobs"]["ctx_index"]][:, other])
    assert np.array_equal(after_syntax[:, 0], g["syntax"][g["jobs"]["ctx_index"]][:, 0])
    zero = g["masks"] == 0
    assert zero.any() and (g["rates"][zero] == 0).all() and np.array_equal(g["after"][zero], g["states"][g["jobs"]["ctx_index"][zero]])
    assert np.array_equal(g["after_syntax"][zero], g["syntax"][g["jobs"]["ctx_index"][zero]])
    # several jobs share one snapshot
    assert len(np.unique(g["jobs"]["ctx_index"][:63])) < 63


@pytest.mark.parametrize("L,depth", UNITS, ids=unit_ids)
def test_golden_trees_reach_every_branch(restated, L, depth):
    tags = restated[L, depth][4]
    missing = [k for k in TR.required_tags(L, depth) if not tags[k]]
    assert not missing, missing



def _made_cases_hold(rec, tree):
    """units 0-5 of tree_rate_tools.random_trees: ties leave depth 1; a depth-1 tree coded in chroma only is no uncoded tree; an uncoded tree never tries depth 0;
    the factor 4 on chroma flips the choice both ways"""
    assert list(rec["depth"][:2]) == [1, 1] and list(rec["tried_zero"][:2]) == [1, 1] and (rec["cost_zero"][:2] == rec["cost_one"][:2]).all()
    assert rec["tried_zero"][2] == 1 and rec["depth"][2] == 0 and tree["mask_one"][2] == 0x080 and not rec["one"]["cbf"][2].any()
    assert rec["tried_zero"][3] == 0 and rec["depth"][3] == 0 and rec["cost_zero"][3] == 0 and tree["mask_zero"][3] == 0
    assert rec["depth"][4] == 1 and rec["depth"][5] == 0 and (rec["tried_zero"][4:6] == 1).all()
    for i, want in ((4, 0), (5, 1)):      # ... what luma alone, and chroma weighted once, would have chosen
        y1, y0 = int(rec["one"]["ssd"][i].sum()), int(rec["zero"]["ssd"][i])
        assert (0 if y0 < y1 else 1) == want and (0 if y0 + tree["chroma_ssd_zero"][i] < y1 + tree["chroma_ssd_one"][i] else 1) == want


def test_numpy_decide_tree_is_tu_decision_hpp():
    """decide_tree against search/tu_decision.hpp's decideRqt with the chroma functor and a rate per depth (tests/tree_decide_client.cpp, compiled here): the
    restatement is pinned before it judges the device"""
    client = TR.DecisionClient()
    T = TR.random_trees(5, 600)
    units, zero_at, one_at, sizes, csizes, chroma_at, tree_rate, tree_cbf = T
    for rl in (1, 40000, 1234567):
        rec, tree = TR.decide_tree(*T, rl)
        want = client.decide(TR.client_rows(*T), rl)
        assert np.array_equal(rec["depth"], want[:, 0]) and np.array_equal(rec["tried_zero"], want[:, 1])
        assert np.array_equal(rec["cost_zero"], want[:, 2]) and np.array_equal(rec["cost_one"], want[:, 3])
        assert np.array_equal(want[:, 4], rec["tried_zero"])      # depth 0 is evaluated only when it is tried
        _made_cases_hold(rec, tree)
    assert (rec["depth"] == 1).any() and ((rec["depth"] == 0) & (rec["tried_zero"] == 1)).any() and (rec["tried_zero"] == 0).any()
    chroma_only = (tree_cbf[1::2] != 0) & ((tree_cbf[1::2] & 0xf) == 0)
    assert chroma_only.sum() > 20 and (rec["tried_zero"][chroma_only] == 1).all()
    # SSDs near 2^31: the sum wraps in int32 as the reference's does
    big = TR.random_trees(6, 40)
    for z in big[3].values():
        z["ssd"][:] = np.random.default_rng(1).integers(1 << 29, 1 << 32, len(z["ssd"]), dtype=np.uint64).astype(np.uint32)
    rec, _ = TR.decide_tree(*big, 3)
    want = client.decide(TR.client_rows(*big), 3)
    assert np.array_equal(rec["cost_zero"], want[:, 2]) and np.array_equal(rec["cost_one"], want[:, 3]) and (rec["cost_one"] < 0).any()


def test_library_surface():
    from turingcodec_amd import havoc
    L, names = havoc._load()
    assert L.havoc_mi355x_tree_rate and L.havoc_mi355x_rqt_decide_tree and {"tree_rate", "rqt_decide_tree"} <= set(names)
    assert havoc.RQT_CHROMA_AT_DT.itemsize == 16 and havoc.RQT_TREE_RESULT_DT.itemsize == 16
    assert havoc.TREE_RATE_JOB_DT.itemsize == 32 and havoc.TREE_RATE_JOB_DT.fields["out_index"][1] == 16 and havoc.TREE_RATE_JOB_DT.fields["flags"][1] == 21
    assert havoc.TREE_RATE_SPLIT_FLAG_CODED == TR.SPLIT_CODED == 1
    header = open(os.path.join(ROOT, "include", "havoc_mi355x.h")).read()
    for name in ("havoc_mi355x_tree_rate(", "} havoc_mi355x_tree_rate_job;   /* sizeof: 32 */", "HAVOC_TREE_RATE_SPLIT_FLAG_CODED", "rqt_root_cbf itself is NOT priced",
                 "havoc_mi355x_rqt_decide_tree(", "havoc_mi355x_rqt_chroma_at", "havoc_mi355x_rqt_tree_choice"):
        assert name in header, name


def test_search_library_still_loads_over_the_stand_in_device():
    """tests/mock_device.c has no tree_rate: libhavoc_search.so does not need it and must still load over the stand-in with every symbol bound at once (a process
    of its own: the stand-in takes the device library's place for everything loaded after it)"""
    code = ("import ctypes as C, os, sys\n"
            f"sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); sys.path.insert(0, {ROOT!r})\n"
            "import search_runner\n"
            "dev = C.CDLL(search_runner.build_mock(), mode=C.RTLD_GLOBAL)\n"
            f"L = C.CDLL({os.path.join(ROOT, 'turingcodec_amd', 'libhavoc_search.so')!r}, mode=os.RTLD_NOW)\n"
            "assert not hasattr(dev, 'havoc_mi355x_tree_rate')\n"
            "assert L.havoc_search_intra_device and L.havoc_search_intra_chain\n"
            "print('loaded')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1] == "loaded", out.stderr[-2000:]


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
@pytest.mark.parametrize("L,depth", UNITS, ids=unit_ids)
def test_device_matches_golden_and_restatement(hv, golden, restated, L, depth):
    """launches of 1, 63, 64, 65 jobs and the golden set (a workgroup walks 64 jobs: where the transposed copy of the states can go wrong); several jobs share a
    snapshot in every launch"""
    g, (rates, masks, after, after_syntax, _, _) = golden[L, depth], restated[L, depth]
    for njobs in (1, 63, 64, 65, len(g["jobs"])):
        jobs = g["jobs"][:njobs]
        got, got_masks, got_after, got_syntax = hv.tree_rate(L, depth, g["luma"], g["chroma"], g["states"], g["syntax"], jobs)
        assert len(got) == njobs
        assert np.array_equal(got, g["rates"][:njobs]), (njobs, np.flatnonzero(got != g["rates"][:njobs])[:8])
        assert np.array_equal(got, rates[:njobs])
        assert np.array_equal(got_masks, g["masks"][:njobs]) and np.array_equal(got_masks, masks[:njobs])
        assert np.array_equal(got_after, g["after"][:njobs]) and np.array_equal(got_after, after[:njobs])
        assert np.array_equal(got_syntax, g["after_syntax"][:njobs]) and np.array_equal(got_syntax, after_syntax[:njobs])
    assert 3 < len(np.unique(g["jobs"]["ctx_index"][:63])) < 63


@pytest.mark.gpu
def test_device_contract(hv, golden):
    """NULL outputs give the same rates and masks; no input table is written; guard bytes around every output are untouched; a graph replays with new levels in
    place"""
    import torch
    L, depth, n = 4, 1, 130
    g = golden[L, depth]
    sy, sc = TR.sizes(L, depth)
    jobs = g["jobs"][:n].copy()
    pad = 64
    jobs["luma_off"] += pad
    jobs["cb_off"] += pad
    jobs["cr_off"] += pad
    jobs["out_index"] += 5
    nr = n + 5
    luma, chroma = np.full(pad + n * sy + pad, 12345, np.int16), np.full(pad + 2 * n * sc + pad, 12345, np.int16)
    luma[pad:pad + n * sy], chroma[pad:pad + 2 * n * sc] = g["luma"][:n * sy], g["chroma"][:2 * n * sc]
    d_luma, d_chroma, d_states, d_syntax, d_jobs = hv.up(luma), hv.up(chroma), _torch_u8(hv, g["states"]), _torch_u8(hv, g["syntax"]), _torch_u8(hv, jobs)
    with torch.cuda.stream(hv.tstream):
        d_rates = torch.full((nr + 7,), -77, dtype=torch.int64, device=hv.device)
        d_rates2 = torch.full((nr + 7,), -77, dtype=torch.int64, device=hv.device)
        d_masks = torch.full((nr + 7,), -78, dtype=torch.int32, device=hv.device)
        d_masks2 = torch.full((nr + 7,), -78, dtype=torch.int32, device=hv.device)
        d_after = torch.full((64 + n * 128 + 64,), 201, dtype=torch.uint8, device=hv.device)
        d_after_syntax = torch.full((64 + n * 4 + 64,), 202, dtype=torch.uint8, device=hv.device)
    hv.tree_rate_d(L, depth, d_luma, d_chroma, d_states, d_syntax, d_jobs, d_rates, d_masks, d_after[64:], d_after_syntax[64:])
    hv.tree_rate_d(L, depth, d_luma, d_chroma, d_states, d_syntax, d_jobs, d_rates2, d_masks2, None, None)
    rates, rates2, masks, masks2 = hv.down(d_rates, np.int64), hv.down(d_rates2, np.int64), hv.down(d_masks, np.int32), hv.down(d_masks2, np.int32)
    assert np.array_equal(rates[5:nr], g["rates"][:n]) and np.array_equal(rates2, rates)
    assert np.array_equal(masks[5:nr].view(np.uint32), g["masks"][:n]) and np.array_equal(masks2, masks)
    assert (rates[:5] == -77).all() and (rates[nr:] == -77).all() and (masks[:5] == -78).all() and (masks[nr:] == -78).all()
    assert np.array_equal(hv.down(d_luma, np.int16), luma) and np.array_equal(hv.down(d_chroma, np.int16), chroma)
    assert np.array_equal(hv.down(d_states, np.uint8), g["states"].reshape(-1)) and np.array_equal(hv.down(d_syntax, np.uint8), g["syntax"].reshape(-1))
    assert np.array_equal(hv.down(d_jobs, np.uint8), jobs.view(np.uint8).reshape(-1))
    after, after_syntax = hv.down(d_after, np.uint8), hv.down(d_after_syntax, np.uint8)
    assert np.array_equal(after[64:64 + n * 128].reshape(-1, 128), g["after"][:n]) and (after[:64] == 201).all() and (after[64 + n * 128:] == 201).all()
    assert np.array_equal(after_syntax[64:64 + n * 4].reshape(-1, 4), g["after_syntax"][:n])
    assert (after_syntax[:64] == 202).all() and (after_syntax[64 + n * 4:] == 202).all()
    # the same launch from a captured graph, replayed twice, the second time with other levels in the same buffers
    graph = hv.graph_capture(lambda: hv.tree_rate_d(L, depth, d_luma, d_chroma, d_states, d_syntax, d_jobs, d_rates, d_masks, d_after[64:], d_after_syntax[64:]))
    luma2, chroma2 = luma.copy(), chroma.copy()
    luma2[pad:pad + n * sy], chroma2[pad:pad + 2 * n * sc] = g["luma"][127 * sy:257 * sy], g["chroma"][2 * 127 * sc:2 * 257 * sc]
    want2 = TR.walk_jobs(L, depth, luma2, chroma2, g["states"], g["syntax"], jobs)
    first = (rates[:nr], masks[:nr].view(np.uint32), g["after"][:n], g["after_syntax"][:n])
    for k, (lv, cv, want) in enumerate(((luma, chroma, first), (luma2, chroma2, want2))):
        with torch.cuda.stream(hv.tstream):
            d_luma.copy_(torch.from_numpy(lv))
            d_chroma.copy_(torch.from_numpy(cv))
            d_rates.fill_(-77)
            d_masks.fill_(-78)
            d_after.fill_(201)
            d_after_syntax.fill_(202)
        hv.graph_launch(graph)
        got, got_masks = hv.down(d_rates, np.int64), hv.down(d_masks, np.int32)
        assert np.array_equal(got[5:nr], want[0][5:nr]) and (got[:5] == -77).all() and (got[nr:] == -77).all(), k
        assert np.array_equal(got_masks[5:nr].view(np.uint32), want[1][5:nr]) and (got_masks[:5] == -78).all() and (got_masks[nr:] == -78).all(), k
        assert np.array_equal(hv.down(d_after, np.uint8)[64:64 + n * 128].reshape(-1, 128), want[2])
        assert np.array_equal(hv.down(d_after_syntax, np.uint8)[64:64 + n * 4].reshape(-1, 4), want[3])
    assert not np.array_equal(want2[0][5:nr], rates[5:nr])
    hv.graph_destroy(graph)


@pytest.mark.gpu
def test_device_refusals(hv, golden):
    import torch
    from turingcodec_amd.havoc import HavocError
    L, depth = 4, 0
    g = golden[L, depth]
    jobs = g["jobs"][:8].copy()
    d_luma, d_chroma, d_states, d_syntax, d_jobs = hv.up(g["luma"]), hv.up(g["chroma"]), _torch_u8(hv, g["states"]), _torch_u8(hv, g["syntax"]), _torch_u8(hv, jobs)
    with torch.cuda.stream(hv.tstream):
        d_rates = torch.zeros(64, dtype=torch.int64, device=hv.device)
        d_masks = torch.zeros(64, dtype=torch.int32, device=hv.device)
    good = (d_luma, d_chroma, d_states, d_syntax, d_jobs, d_rates, d_masks)
    for bad_l in (2, 6):
        with pytest.raises(HavocError, match="log2CbSize"):
            hv.tree_rate_d(bad_l, 0, *good)
    for bad_d in (-1, 2):
        with pytest.raises(HavocError, match="depth"):
            hv.tree_rate_d(4, bad_d, *good)
    for k in (0, 1, 2, 3, 5, 6):
        args = list(good)
        args[k] = None
        with pytest.raises(HavocError, match="null"):
            hv.tree_rate_d(4, 0, *args)
    p = [t.data_ptr() for t in good]
    with pytest.raises(HavocError, match="null"):
        hv._ck(hv.L.havoc_mi355x_tree_rate(hv.h, 4, 0, p[0], p[1], p[2], p[3], None, 1, p[5], p[6], None, None))
    with pytest.raises(HavocError, match="njobs"):
        hv._ck(hv.L.havoc_mi355x_tree_rate(hv.h, 4, 0, p[0], p[1], p[2], p[3], p[4], -1, p[5], p[6], None, None))
    for k, off in ((0, 2), (1, 4), (5, 4), (6, 2)):
        q = list(p)
        q[k] += off
        with pytest.raises(HavocError, match="aligned"):
            hv._ck(hv.L.havoc_mi355x_tree_rate(hv.h, 4, 0, q[0], q[1], q[2], q[3], q[4], 8, q[5], q[6], None, None))
    with pytest.raises(HavocError, match="d_states_out"):
        hv.tree_rate_d(4, 0, *good, d_states, None)
    with pytest.raises(HavocError, match="d_syntax_states_out"):
        hv.tree_rate_d(4, 0, *good, None, d_syntax)
    # a job the entry point excludes beside good ones: nothing of it is read, its rate is -1, its mask 0, its snapshots pass through; the others are priced
    bad = g["jobs"][:8].copy()
    bad["luma_off"][[1, 5]] = bad["cb_off"][[1, 5]] = bad["cr_off"][[1, 5]] = 1 << 30      # (would fault if read)
    bad["flags"][1], bad["flags"][5] = 2, 0x81
    rates, masks, after, after_syntax = hv.tree_rate(L, depth, g["luma"], g["chroma"], g["states"], g["syntax"], bad)
    want = TR.walk_jobs(L, depth, g["luma"], g["chroma"], g["states"], g["syntax"], bad)
    for a, b in zip((rates, masks, after, after_syntax), want):
        assert np.array_equal(a, b)
    keep = [0, 2, 3, 4, 6, 7]
    assert (rates[[1, 5]] == -1).all() and (masks[[1, 5]] == 0).all() and np.array_equal(rates[keep], g["rates"][keep]) and (rates[keep] > 0).any()
    assert np.array_equal(after[[1, 5]], g["states"][bad["ctx_index"][[1, 5]]]) and np.array_equal(after_syntax[[1, 5]], g["syntax"][bad["ctx_index"][[1, 5]]])


def _device_tree_decision(hv, units, zero_at, one_at, sizes, csizes, chroma_at, tree_rate, tree_cbf, rl):
    """havoc_mi355x_rqt_decide_tree over made outcomes -> (RQT_RESULT_DT, RQT_TREE_RESULT_DT records, {log2: luma final jobs}, {log2: chroma final jobs})"""
    import torch
    from turingcodec_amd.decisions import RQT_RESULT_DT
    from turingcodec_amd.havoc import RQT_TREE_RESULT_DT
    tables, keep, fins = [np.zeros((4, 5), np.uint64), np.zeros((4, 5), np.uint64)], [], [{}, {}]
    for which, group in enumerate((sizes, csizes)):
        for s, z in group.items():
            m = len(z["cbf"])
            if not m:
                continue
            jobs = np.stack([np.arange(m) * 7, np.arange(m) * 11 + 1, np.arange(m) * 13 + 2, np.full(m, -5)], 1).astype(np.int32)
            d = [hv.up(z["cbf"]), hv.up(z["ssd"]), None, hv.up(jobs), hv.zeros(4 * m, np.int32)]
            keep.append(d)
            tables[which][s - 2] = [t.data_ptr() if t is not None else 0 for t in d]
            fins[which][s] = d[4]
    d_units = hv.up(np.ascontiguousarray(units).view(np.int32))
    with torch.cuda.stream(hv.tstream):
        d_rate = torch.from_numpy(np.ascontiguousarray(tree_rate, np.int64)).to(hv.device)
    out, tree_out = hv.zeros(len(units) * 26, np.int32), hv.zeros(len(units) * 4, np.int32)
    hv.rqt_decide_tree_d(d_units.view(-1, 4), hv.up(zero_at), hv.up(one_at), tables[0], tables[1], hv.up(np.ascontiguousarray(chroma_at).view(np.int32)), d_rate,
                         hv.up(tree_cbf), 1000, 512, 99, 5000, 9000, 256, 77, rl, out, tree_out)
    return (hv.down(out, np.int32).view(RQT_RESULT_DT).copy(), hv.down(tree_out, np.int32).view(RQT_TREE_RESULT_DT).copy(),
            {s: hv.down(f, np.int32).reshape(-1, 4).copy() for s, f in fins[0].items()}, {s: hv.down(f, np.int32).reshape(-1, 4).copy() for s, f in fins[1].items()})


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_tree_decision_is_the_numpy_restatement(hv, n):
    """arbitrary rates, masks and SSDs (a workgroup decides 256 units), the made cases among them; the final job records of every luma and chroma candidate: the
    chosen tree into the picture (luma origin 1000, stride 512; Cb 5000, Cr 9000, stride 256), the rest at the dump offsets (99, 77)"""
    T = TR.random_trees(20 + n, n)
    units, zero_at, one_at, sizes, csizes, chroma_at, tree_rate, tree_cbf = T
    rl = 40000
    got, got_tree, fin, cfin = _device_tree_decision(hv, *T, rl)
    want, want_tree = TR.decide_tree(*T, rl)
    assert got.tobytes() == want.tobytes() and got_tree.tobytes() == want_tree.tobytes()
    if n >= 6:
        _made_cases_hold(got, got_tree)
        assert (want["depth"] == 1).any() and ((want["depth"] == 0) & (want["tried_zero"] == 1)).any() and (want["tried_zero"] == 0).any()

    def job(j, at):
        return [j * 7, j * 11 + 1, j * 13 + 2, at]

    for i, u in enumerate(units):
        L, j0, j1, a, x0, y0 = int(u["log2_size"]), int(zero_at[i]), int(one_at[i]), chroma_at[i], int(u["x0"]), int(u["y0"])
        zero_wins = want["depth"][i] == 0 and want["tried_zero"][i] == 1
        half = 1 << (L - 1)
        assert list(fin[L][j0]) == job(j0, 1000 + y0 * 512 + x0 if zero_wins else 99)
        for k in range(4):
            assert list(fin[L - 1][j1 + k]) == job(j1 + k, 99 if zero_wins else 1000 + (y0 + (k >> 1) * half) * 512 + x0 + (k & 1) * half)
        c = (y0 // 2) * 256 + x0 // 2
        zero_chroma = zero_wins or L == 3      # an 8x8 unit's one chroma block per component belongs to both trees
        cz = cfin[max(L - 1, 2)]
        assert list(cz[a["cb_zero"]]) == job(int(a["cb_zero"]), 5000 + c if zero_chroma else 77)
        assert list(cz[a["cr_zero"]]) == job(int(a["cr_zero"]), 9000 + c if zero_chroma else 77)
        if L > 3:
            q = half // 2
            for k in range(4):
                sub = c + (k >> 1) * q * 256 + (k & 1) * q
                assert list(cfin[L - 2][a["cb_one"] + k]) == job(int(a["cb_one"]) + k, 77 if zero_wins else 5000 + sub)
                assert list(cfin[L - 2][a["cr_one"] + k]) == job(int(a["cr_one"]) + k, 77 if zero_wins else 9000 + sub)
    # every final record was written exactly by its own unit
    for f in list(fin.values()) + list(cfin.values()):
        assert (f[:, 3] != 0).all() or n == 1


@pytest.mark.gpu
def test_tree_decision_refusals(hv):
    from turingcodec_amd.havoc import HavocError
    T = TR.random_trees(3, 8)
    for bad in (dict(rl=-1), dict(stride=0), dict(cdump=-1)):
        with pytest.raises(HavocError):
            units, zero_at, one_at, sizes, csizes, chroma_at, tree_rate, tree_cbf = T
            z = np.zeros((4, 5), np.uint64)
            d = hv.zeros(64, np.int32)
            hv.rqt_decide_tree_d(d.view(-1, 4)[:8], d, d, z, z, d, d, d, 1000, 512, 99, 5000, 9000, bad.get("stride", 256), bad.get("cdump", 77), bad.get("rl", 5), d, d)
    with pytest.raises(HavocError, match="null"):
        z = np.zeros((4, 5), np.uint64)
        d = hv.zeros(64, np.int32)
        hv.rqt_decide_tree_d(d.view(-1, 4)[:8], d, d, z, z, None, d, d, 1000, 512, 99, 5000, 9000, 256, 77, 5, d, d)
    with pytest.raises(HavocError, match="chroma size table"):
        z, c = np.zeros((4, 5), np.uint64), np.zeros((4, 5), np.uint64)
        d = hv.zeros(64, np.int32)
        c[0, 0] = d.data_ptr()
        hv.rqt_decide_tree_d(d.view(-1, 4)[:8], d, d, z, c, d, d, d, 1000, 512, 99, 5000, 9000, 256, 77, 5, d, d)


# ---- the picture level: DecisionPicture(tree_rates=True) -----------------------------------------------------------------------------------------------
PICTURE = (56, 56)      # the smallest picture whose rqt_units hold 32x32, 16x16 and 8x8 units: a remainder of 16 and of 8 beyond a whole 32, both ways


@pytest.fixture(scope="module")
def pictures(hv):
    """DecisionPicture(56, 56, 8 bit, QP 32, seed 21) by default, with residual_rates and with tree_rates: three steps each, the third replayed from the graph"""
    from turingcodec_amd.decisions import DecisionPicture
    out = {}
    for name, options in (("default", {}), ("residual", dict(residual_rates=True)), ("tree", dict(tree_rates=True))):
        dp = DecisionPicture(hv, *PICTURE, 8, 32, seed=21, threads=8, intra=False, **options)
        for _ in range(3):
            dp.step()
        assert all(dp._graphs.values()) and len(dp._graphs) == 1
        out[name] = dp
    return out


def _block(plane, origin, stride, x, y, n):
    return plane[origin + y * stride + x + np.arange(n)[:, None] * stride + np.arange(n)]


@pytest.mark.gpu
def test_picture_step_with_tree_rates(hv, pictures):
    import torch
    dp = pictures["tree"]
    P = dp.rqt_plan
    units, zero_at, one_at, chroma_at = dp.units, hv.down(P["d_zero_at"], np.int32), hv.down(P["d_one_at"], np.int32), P["chroma_at"]
    assert {3, 4, 5} == set(int(v) for v in units["log2_size"])
    results, tree_results = dp.rqt_results.copy(), dp.rqt_tree_results.copy()
    # the rates and masks: the restatement on the device's own levels of three planes, every tree from its unit's snapshots
    levels = {s: hv.down(g["level"], np.int16) for s, g in P["sizes"].items()}
    clevels = {s: hv.down(g["level"], np.int16) for s, g in P["csizes"].items()}
    tree_rate, tree_cbf = np.zeros(2 * len(units), np.int64), np.zeros(2 * len(units), np.uint32)
    device_cbf = hv.down(P["tree_cbf"], np.int32).view(np.uint32)
    assert set(P["tree_jobs"]) == set(UNITS)
    for (L, depth), t in P["tree_jobs"].items():
        jobs = t["jobs"]
        r, m, _, _ = TR.walk_jobs(L, depth, levels[t["luma"]], clevels[t["chroma"]], dp.rdoq_states, dp.syntax_states, jobs)
        at = jobs["out_index"]
        assert np.array_equal(dp.rqt_rates[L, depth], r[at]) and np.array_equal(device_cbf[at], m[at]), (L, depth)
        assert np.array_equal(at, 2 * np.flatnonzero(units["log2_size"] == L) + depth) and (jobs["flags"] == 1).all()
        tree_rate[at], tree_cbf[at] = r[at], m[at]
    assert (tree_rate > 0).any()
    # the decisions: the numpy restatement on the device's own cbf / ssd of all three planes and the restated rates
    sizes = {s: dict(cbf=hv.down(g["cbf"], np.int32), ssd=hv.down(g["ssd"], np.uint32)) for s, g in P["sizes"].items()}
    csizes = {s: dict(cbf=hv.down(g["cbf"], np.int32), ssd=hv.down(g["ssd"], np.uint32)) for s, g in P["csizes"].items()}
    want, want_tree = TR.decide_tree(units, zero_at, one_at, sizes, csizes, chroma_at, tree_rate, tree_cbf, P["rl_q16"])
    assert results.tobytes() == want.tobytes() and tree_results.tobytes() == want_tree.tobytes()
    # a candidate's cbf is its mask bit
    for i, u in enumerate(units):
        L, a = int(u["log2_size"]), chroma_at[i]
        assert [int(v != 0) for v in sizes[L - 1]["cbf"][one_at[i]:one_at[i] + 4]] == [int(tree_cbf[2 * i + 1]) >> k & 1 for k in range(4)]
        assert int(csizes[max(L - 1, 2)]["cbf"][a["cb_zero"]] != 0) == int(tree_cbf[2 * i]) >> 4 & 1
    # recon and crecon hold, per unit, the pieces of the chosen depth: the tree part once more into cleared planes
    with torch.cuda.stream(hv.tstream):
        dp.recon.zero_()
        dp.crecon.zero_()
    dp.tree_decisions()
    hv.sync()
    assert hv.down(P["d_out"], np.int32).tobytes() == results.tobytes()
    recon, crecon = hv.down(dp.recon, dp.dt), hv.down(dp.crecon, dp.dt)
    pieces = {s: hv.down(g["piece"], dp.dt) for s, g in P["sizes"].items()}
    cpieces = {s: hv.down(g["piece"], dp.dt) for s, g in P["csizes"].items()}
    for i, u in enumerate(units):
        L, x0, y0, a = int(u["log2_size"]), int(u["x0"]), int(u["y0"]), chroma_at[i]
        zero_wins = results["depth"][i] == 0 and results["tried_zero"][i] == 1
        half = 1 << (L - 1)
        blocks = [(L, int(zero_at[i]), x0, y0)] if zero_wins else [(L - 1, int(one_at[i]) + k, x0 + (k & 1) * half, y0 + (k >> 1) * half) for k in range(4)]
        for s, j, x, y in blocks:
            n = 1 << s
            assert np.array_equal(_block(recon, dp.origin, dp.stride, x, y, n), pieces[s][j * n * n:(j + 1) * n * n].reshape(n, n)), (i, s, j)
        for comp, zero_key, one_key in ((0, "cb_zero", "cb_one"), (1, "cr_zero", "cr_one")):
            origin = comp * dp.cpe + dp.corigin
            if zero_wins or L == 3:
                cblocks = [(max(L - 1, 2), int(a[zero_key]), x0 // 2, y0 // 2)]
            else:
                cblocks = [(L - 2, int(a[one_key]) + k, x0 // 2 + (k & 1) * (half // 2), y0 // 2 + (k >> 1) * (half // 2)) for k in range(4)]
            for s, j, x, y in cblocks:
                n = 1 << s
                assert np.array_equal(_block(crecon, origin, dp.cstride, x, y, n), cpieces[s][j * n * n:(j + 1) * n * n].reshape(n, n)), (i, comp, s, j)
    # how the whole-tree comparison moves the decisions (printed, not asserted: the made inputs of the kernel and decision tests hold the branch coverage)
    other = pictures["residual"].rqt_results
    differ = (other["depth"] != results["depth"]) | (other["tried_zero"] != results["tried_zero"])
    print("units", len(units), "deciding differently from residual_rates=True:", int(differ.sum()), "| untried:", int((results["tried_zero"] == 0).sum()),
          "depth 0:", int(((results["depth"] == 0) & (results["tried_zero"] == 1)).sum()), "depth 1:", int((results["depth"] == 1).sum()),
          "| depth-1 trees coded in chroma only:", int(((tree_results["mask_one"] != 0) & ((tree_results["mask_one"] & 0xf) == 0)).sum()))


@pytest.mark.gpu
def test_default_picture_is_unchanged_beside_the_tree_route(hv, pictures):
    """the same picture without the option: the default route's launches are what they were -- its decisions carry no tree record, and its chroma, coded at depth 0
    always, is bit for bit the tree route's depth-0 chroma candidates (same prediction, same snapshots, same chain)"""
    dp, tr = pictures["default"], pictures["tree"]
    assert not dp.tree_rates and not hasattr(dp, "syntax_states") and "csizes" not in dp.rqt_plan
    with pytest.raises(ValueError):
        dp.rqt_tree_results
    assert np.array_equal(hv.down(dp.pred, dp.dt), hv.down(tr.pred, tr.dt)) and np.array_equal(hv.down(dp.cpred, dp.dt), hv.down(tr.cpred, tr.dt))
    crecon = hv.down(dp.crecon, dp.dt)
    P = tr.rqt_plan
    cpieces = {s: hv.down(g["piece"], tr.dt) for s, g in P["csizes"].items()}
    for i, u in enumerate(tr.units):
        L, a = int(u["log2_size"]), P["chroma_at"][i]
        s = max(L - 1, 2)
        n = 1 << (L - 1)
        if n < 4:
            continue
        for comp, key in ((0, "cb_zero"), (1, "cr_zero")):
            j = int(a[key])
            assert np.array_equal(_block(crecon, comp * dp.cpe + dp.corigin, dp.cstride, int(u["x0"]) // 2, int(u["y0"]) // 2, n),
                                  cpieces[s][j * n * n:(j + 1) * n * n].reshape(n, n)), (i, comp)
    # the luma candidates of both routes are the same blocks
    for s, g in dp.rqt_plan["sizes"].items():
        assert np.array_equal(hv.down(g["level"], np.int16), hv.down(P["sizes"][s]["level"], np.int16))


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(reflibs.REF_SO), reason="oracle/_ref not built")
def test_default_picture_step_is_the_reference_tables(hv, pictures):
    """the default step on this picture: the decisions and the reconstruction the reference's tables + Rdoq.cpp give with the stand-in rate, as
    tests/test_decisions.py holds them at its sizes"""
    import torch
    import search_tools as st
    dp = pictures["default"]
    ref = st.Client("ref", 3)
    pred = hv.down(dp.pred, dp.dt).copy()
    exp_rqt, exp_rec = ref.rqt(8, dp.host_planes[0], dp.stride, dp.PAD, pred, dp.W, dp.rdoq_states, dp.quant, dp.lam, 1.0 / dp.lam, dp.units)
    assert dp.rqt_results.tobytes() == exp_rqt.tobytes()
    with torch.cuda.stream(hv.tstream):
        dp.recon.zero_()
    dp.tree_decisions()
    hv.sync()
    rows = dp.origin + np.arange(dp.H)[:, None] * dp.stride + np.arange(dp.W)
    assert np.array_equal(hv.down(dp.recon, dp.dt)[rows], exp_rec[rows])


@pytest.mark.gpu
def test_tree_rates_are_refused_where_they_are_not_built(hv, pictures):
    from turingcodec_amd.decisions import DecisionPicture
    for options in (dict(search_on_device=False), dict(residual_rates=True), dict(sao=True)):
        with pytest.raises(ValueError):
            DecisionPicture(hv, *PICTURE, 8, 32, seed=21, threads=8, intra=False, tree_rates=True, **options)
    with pytest.raises(ValueError):
        pictures["tree"].step_banded(hv)
