"""DecisionPicture(motion=...) and DecisionPicture(col=...): a decided picture hands the next picture both things a reference picture is -- the deblocked, padded planes
(finish=True) and its motion as the collocated store (havoc_mi355x_cqt_motion_store, directly behind the commit inside the replayed graph) -- and the next picture
derives its units' temporal candidates from that store on the device (havoc_mi355x_temporal_candidates, inside ITS replayed graph), with no host round trip.  -m gpu.

Picture A (POC 8, list 0 -> POC 0, list 1 -> POC 16) runs with unit_trees, cqt, commit, finish and motion; picture B (POC 4, list 0 -> POC 0, list 1 -> POC 8 = A) runs the
default step with col = A's store, after A's step is synchronised.  Two sizes: 136 x 72 and 416 x 240; 8-bit, QP 32, three steps each, the third from the graph.
With these picture order counts A's vectors span 8 pictures (list 0: +8, list 1: -8) and B's targets lie 4 pictures away (list 0: +4, list 1: -4): EVERY candidate
that exists is scaled, by +-1/2, and none has the same distance, is clipped, long-term or refused.
"""
import collections

import numpy as np
import pytest

import cqt_motion_tools as M

pytestmark = pytest.mark.gpu

PICTURES = {"136x72": (136, 72), "416x240": (416, 240)}
BASE = dict(tree_rates=True, pu_modes=True, cu_close=True, cqt=True, unit_trees=True, commit=True, finish=True)
QP, MOTION = 32, (8, 0, 16)
COL = dict(col_poc=8, cur_poc=4, target_poc=(0, 8), all_backwards=0)


@pytest.fixture(scope="module")
def hv():
    from turingcodec_amd.havoc import Havoc
    h = Havoc(stream="new")
    yield h
    h.close()


def _steps(dp):
    for _ in range(3):
        out = dp.step()
    assert all(dp._graphs.values()) and len(dp._graphs) == 1
    return out


@pytest.fixture(scope="module", params=list(PICTURES))
def pictures(hv, request):
    """A with and without motion; then -- A's steps are synchronised, its store stands -- B without col and with col for both collocated_from_l0 values"""
    from turingcodec_amd.decisions import DecisionPicture
    w, h = PICTURES[request.param]
    out = {}
    for name, options in (("a_on", dict(BASE, motion=MOTION)), ("a_off", BASE)):
        dp = DecisionPicture(hv, w, h, 8, QP, seed=21, threads=8, intra=False, **options)
        out[name] = (dp, _steps(dp))
    store = out["a_on"][0].cqt_store
    for name, options in (("b_off", {}), ("b_l0", dict(col=dict(COL, store=store, collocated_from_l0=1))), ("b_l1", dict(col=dict(COL, store=store, collocated_from_l0=0)))):
        dp = DecisionPicture(hv, w, h, 8, QP, seed=22, threads=8, intra=False, **options)
        out[name] = (dp, _steps(dp))
    return out


def _same(a, b):
    assert set(a) == set(b)
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) if isinstance(a[k], np.ndarray) else a[k] == b[k]
               for k in a)


def _legacy_outputs(dp):
    """recon, the picture's part of crecon (its lower padding holds the legacy plan's dump block, different from run to run), cells, the loop filter's edge data"""
    c2, c = dp.PAD // 2, dp.hv.down(dp.crecon, dp.dt)
    chroma = np.stack([c[k * dp.cpe:k * dp.cpe + dp.cn].reshape(-1, dp.cstride)[c2:c2 + dp.H // 2, c2:c2 + dp.W // 2] for k in (0, 1)])
    return dict(recon=dp.hv.down(dp.recon, dp.dt), chroma=chroma, cells=np.ascontiguousarray(dp.cells).view(np.uint8), data=dp.hv.down(dp.d_data, np.int8),
                bs=dp.hv.down(dp.d_bs, np.uint8))


def test_store_is_the_restatement_over_the_committed_cells(pictures):
    a = pictures["a_on"][0]
    cqt = a.hv.cqt_cells_download(a.cqt_cells, a.W, a.H, 3)
    assert (cqt["unit"] >= 0).all()
    got, tags = a.cqt_motion_results(), collections.Counter()
    want = M.motion_store(cqt, a.W, a.H, 3, MOTION[1], MOTION[2], tags)
    assert got.dtype == M.COL_CELL_DT and got.shape == M.store_shape(a.W, a.H) and got.tobytes() == want.tobytes()
    assert a.cqt_motion_results() is got
    print("entries", got.size, dict(tags))
    assert got["pred_flag"].any(axis=-1).all() and got["mv"].any()         # every CTU is decided: every entry has motion, and not all of it is zero


def test_a_is_otherwise_unchanged(pictures):
    """motion leaves the finished planes, the committed cells, recon, crecon, cells and every record of the options byte-identical; one graph"""
    (on, r_on), (off, r_off) = pictures["a_on"], pictures["a_off"]
    assert not hasattr(off, "cqt_store")
    assert _same(_legacy_outputs(on), _legacy_outputs(off)) and _legacy_outputs(on)["recon"].any()
    assert _same(on.cqt_finish_results(), off.cqt_finish_results())
    assert on.hv.down(on.cqt_cells, np.uint8).tobytes() == off.hv.down(off.cqt_cells, np.uint8).tobytes()
    assert _same(on.pu_decisions, off.pu_decisions) and _same(on.unit_tree_decisions(), off.unit_tree_decisions())
    assert _same(on.cu_decisions, off.cu_decisions) and _same(on.cqt_decisions, off.cqt_decisions)
    assert np.array_equal(r_on[0], r_off[0]) and np.array_equal(r_on[1], r_off[1])
    assert len(on._graphs) == 1 and len(off._graphs) == 1


@pytest.mark.parametrize("which,from_l0", [("b_l0", 1), ("b_l1", 0)])
def test_candidates_are_the_host_form_over_a_store(pictures, which, from_l0):
    """B's records equal search/amvp.hpp's deriveTemporalCandidate (the client) and the restatement over A's downloaded store and B's own unit table"""
    a, b = pictures["a_on"][0], pictures[which][0]
    store = a.cqt_motion_results()
    params = M.make_params(b.W, b.H, 6, COL["col_poc"], COL["cur_poc"], COL["target_poc"], COL["all_backwards"], from_l0)
    got, tags = b.temporal_candidates(), collections.Counter()
    assert got.dtype == M.CAND_DT and got.shape == (len(b.pus), 2) and b.temporal_candidates() is got
    assert got.tobytes() == M.Client().temporal_candidates(params, store, b.pus).tobytes()
    assert got.tobytes() == M.temporal_candidates(params, store, b.pus, tags).tobytes()
    print(which, "records", got.size, "available", int(got["available"].sum()), dict(tags))
    # at least one candidate is available and at least one is scaled; and no other outcome than the module docstring says
    assert got["available"].any() and tags["scaled"] > 0
    for k in ("same_distance", "td_clipped", "tb_clipped", "factor_clipped", "vector_clipped", "long_term", "col_poc_equals_ref_poc", "pu_outside_picture", "none"):
        assert tags[k] == 0, k
    assert got["available"].all() and set(np.unique(got["source"])) <= {M.BOTTOM_RIGHT, M.CENTRE}
    assert tags["both_from_l0" if from_l0 else "both_from_l1"] > 0 and tags["both_from_l1" if from_l0 else "both_from_l0"] == 0


def test_b_is_otherwise_unchanged(pictures):
    """col leaves the search results, recon, crecon, cells and the edge data byte-identical; one graph"""
    (off, r_off) = pictures["b_off"]
    assert not hasattr(off, "_d_temporal")
    for which in ("b_l0", "b_l1"):
        on, r_on = pictures[which]
        assert _same(_legacy_outputs(on), _legacy_outputs(off)) and _legacy_outputs(on)["recon"].any(), which
        assert np.array_equal(r_on[0], r_off[0]) and np.array_equal(r_on[1], r_off[1]), which
        assert on.rqt_results.tobytes() == off.rqt_results.tobytes(), which
        assert len(on._graphs) == 1 and len(off._graphs) == 1


def test_refusals(hv, pictures):
    from turingcodec_amd.decisions import DecisionPicture
    a, a_off, b, b_off = (pictures[k][0] for k in ("a_on", "a_off", "b_l0", "b_off"))
    make = lambda **o: DecisionPicture(hv, a.W, a.H, 8, QP, seed=21, threads=8, intra=False, **o)
    with pytest.raises(ValueError, match="motion"):
        make(motion=MOTION)
    with pytest.raises(ValueError, match="motion"):
        make(motion=MOTION, **dict(BASE, commit=False, finish=False))
    with pytest.raises(ValueError, match="commit"):      # wherever commit is refused
        make(motion=MOTION, commit=True, tree_rates=True, pu_modes=True, cu_close=True, cqt=True)
    with pytest.raises(ValueError, match="col"):
        make(col=dict(COL, store=a.cqt_store, collocated_from_l0=1), search_on_device=False)
    with pytest.raises(ValueError, match="col"):
        make(col=dict(COL, store=a.cqt_store))           # a key is missing
    with pytest.raises(ValueError, match="motion"):
        a_off.cqt_motion_results()
    with pytest.raises(ValueError, match="col"):
        b_off.temporal_candidates()
    with pytest.raises(ValueError, match="temporal"):
        b.step_banded(hv)
    with pytest.raises(ValueError):
        a.step_banded(hv)
