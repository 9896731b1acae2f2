"""DecisionPicture(merge_lists=max_cand): the merge candidate lists of the committed picture's final coding units (havoc_mi355x_cqt_merge_lists), derived inside the one
replayed graph from the committed cells and this picture's temporal candidates.  -m gpu.

Picture A (POC 8, list 0 -> POC 0, list 1 -> POC 16) runs with commit, finish and motion, as in tests/test_cqt_motion_picture.py; picture B (POC 4, list 0 -> POC 0,
list 1 -> POC 8 = A) runs with the full base options, motion=(4, 0, 8), col = A's store and merge_lists=5 -- with temporal_mvp off and on, and without col (no
temporal candidate).  B's records must be the restatement of tests/merge_list_tools over B's DOWNLOADED cells and temporal candidates; every other output of B must be
what B without merge_lists leaves.  136 x 72 and 416 x 240, 8-bit, QP 32, three steps each, the third from the graph.
"""
import collections

import numpy as np
import pytest

import merge_list_tools as M
import search_temporal_tools as T

pytestmark = pytest.mark.gpu

BASE = dict(tree_rates=True, pu_modes=True, cu_close=True, cqt=True, unit_trees=True, commit=True, finish=True)
QP, MOTION_A, MOTION_B = 32, (8, 0, 16), (4, 0, 8)
COL = dict(col_poc=8, cur_poc=4, target_poc=(0, 8), all_backwards=0, collocated_from_l0=1)
VARIANTS = {"off": dict(col=True), "on": dict(col=True, merge_lists=5), "off_mvp": dict(col=True, temporal_mvp=True), "on_mvp": dict(col=True, temporal_mvp=True, merge_lists=5),
            "off_no_col": dict(), "on_no_col": dict(merge_lists=5)}


@pytest.fixture(scope="module")
def hv():
    h = M.private_havoc()       # (a stream of the context's own, not one of torch's pool: see there)
    yield h
    h.close()


def _snapshot(dp, out):
    """everything a step leaves that does not belong to merge_lists"""
    hv = dp.hv
    c2, c = dp.PAD // 2, hv.down(dp.crecon, dp.dt)
    chroma = np.stack([c[k * dp.cpe:k * dp.cpe + dp.cn].reshape(-1, dp.cstride)[c2:c2 + dp.H // 2, c2:c2 + dp.W // 2] for k in (0, 1)])
    s = dict(res=out[0].copy(), field=out[1].copy(), bi=dp.bi_results.copy(), recon=hv.down(dp.recon, dp.dt), chroma=chroma, cells=np.ascontiguousarray(dp.cells).view(np.uint8),
             data=hv.down(dp.d_data, np.int8), bs=hv.down(dp.d_bs, np.uint8), rqt=np.frombuffer(dp.rqt_results.tobytes(), np.uint8),
             cqt_cells=hv.down(dp.cqt_cells, np.uint8), store=dp.cqt_motion_results().copy())
    s.update({"finish_" + k: np.ascontiguousarray(v) for k, v in dp.cqt_finish_results().items()})
    if dp.col is not None:
        s["cands"] = dp.temporal_candidates().copy()
    return s


def _same(a, b):
    assert set(a) == set(b)
    return [k for k in a if np.ascontiguousarray(a[k]).view(np.uint8).tobytes() != np.ascontiguousarray(b[k]).view(np.uint8).tobytes()]


@pytest.fixture(scope="module", params=list(T.PICTURES))
def pictures(hv, request):
    from turingcodec_amd.decisions import DecisionPicture
    w, h = T.PICTURES[request.param]
    a = DecisionPicture(hv, w, h, 8, QP, seed=21, threads=8, intra=False, **dict(BASE, motion=MOTION_A))
    for _ in range(3):
        a.step()
    out = {"a": a}
    for name, o in VARIANTS.items():
        o = dict(o)
        if o.pop("col", False):
            o["col"] = dict(COL, store=a.cqt_store)
        dp = DecisionPicture(hv, w, h, 8, QP, seed=22, threads=8, intra=False, **dict(BASE, motion=MOTION_B, **o))
        shots, merges = [], []
        for _ in range(3):
            shots.append(_snapshot(dp, dp.step()))
            merges.append(dp.cqt_merge_results().copy() if dp.merge_lists is not None else None)
        assert all(dp._graphs.values()) and len(dp._graphs) == 1, name          # one graph, replayed by the third step
        out[name] = (dp, shots, merges)
    return out


@pytest.mark.parametrize("name", ["on", "on_mvp", "on_no_col"])
def test_records_are_the_restatement_over_the_downloaded_cells(pictures, hv, name):
    dp, shots, merges = pictures[name]
    from turingcodec_amd import havoc
    assert merges[0].dtype == havoc.MERGE_LIST_DT == M.MERGE_LIST_DT and merges[0].shape == (len(dp.pus),)
    assert merges[1].tobytes() == merges[0].tobytes() and merges[2].tobytes() == merges[0].tobytes()       # plain, captured, replayed
    cells = hv.cqt_cells_download(dp.cqt_cells, dp.W, dp.H, dp.CQT_MIN_CB_LOG2)
    params = M.make_params(dp.W, dp.H, dp.CQT_CTB_LOG2, 5, MOTION_B[1:])
    pus = np.ascontiguousarray(dp.pus)
    assert pus.dtype == M.PU_DT
    temporal = shots[-1]["cands"] if dp.col is not None else None
    tags = collections.Counter()
    want = M.merge_lists(params, cells, pus, temporal, tags)
    got = merges[-1]
    assert got.tobytes() == want.tobytes()
    # every final unit's n_cand is 5, every other record is zero; the final units are the decided quadtrees' leaves: they tile the decided CTUs
    final = got["n_cand"] == 5
    assert final.any() and not got["n_cand"][~final].any() and not got[~final]["cand"].view(np.uint8).any() and (got["match"][~final] == -1).all() and not got["reserved"].any()
    area = int((pus["w"][final].astype(np.int64) * pus["h"][final]).sum())
    assert area == int((cells["unit"] >= 0).sum()) * 64
    has_temporal = tags["col_l0_only"] + tags["col_l1_only"] + tags["col_both"]
    if dp.col is None:
        assert tags["col_no_table"] == final.sum() and not has_temporal
    else:
        assert has_temporal > 0
    per_index = [int((got["match"][final] == k).sum()) for k in range(5)]
    print(dp.W, dp.H, name, "final units", int(final.sum()), "of", len(pus), "with match >= 0 per index", per_index, "none", int((got["match"][final] < 0).sum()),
          "with a temporal candidate", has_temporal, "n_real histogram", np.bincount(got["n_real"][final], minlength=6).tolist())


def test_lists_without_col_hold_no_temporal_candidate(pictures):
    """the same cells (the searches do not depend on col without temporal_mvp): a list made with the table differs from the one made without only where the unit has
    a temporal candidate"""
    (on, s_on, m_on), (no, s_no, m_no) = pictures["on"], pictures["on_no_col"]
    assert s_on[-1]["cqt_cells"].tobytes() == s_no[-1]["cqt_cells"].tobytes()
    cands = s_on[-1]["cands"]
    differ = np.array([a.tobytes() != b.tobytes() for a, b in zip(m_on[-1], m_no[-1])])
    assert differ.any() and cands["available"].any(axis=1)[differ].all()


@pytest.mark.parametrize("on,off", [("on", "off"), ("on_mvp", "off_mvp"), ("on_no_col", "off_no_col")])
def test_every_other_output_is_untouched(pictures, on, off):
    (dp_on, s_on, _), (dp_off, s_off, _) = pictures[on], pictures[off]
    assert dp_off.merge_lists is None and not hasattr(dp_off, "cqt_merge") and dp_on.merge_lists == 5
    for a, b in zip(s_on, s_off):
        assert _same(a, b) == []
    assert len(dp_on._graphs) == 1 and len(dp_off._graphs) == 1


def test_refusals(pictures, hv):
    from turingcodec_amd.decisions import DecisionPicture
    a = pictures["a"]
    make = lambda **o: DecisionPicture(hv, a.W, a.H, 8, QP, seed=22, threads=8, intra=False, **o)
    with pytest.raises(ValueError, match="merge_lists"):
        make(**dict(BASE, merge_lists=5))                                   # no motion=: no picture order counts
    with pytest.raises(ValueError, match="merge_lists"):
        make(merge_lists=5, motion=MOTION_B)                                # no commit
    with pytest.raises(ValueError, match="merge_lists"):
        make(**dict(BASE, motion=MOTION_B, merge_lists=6))
    with pytest.raises(ValueError, match="merge_lists"):
        make(**dict(BASE, motion=MOTION_B, merge_lists=0))
    with pytest.raises(ValueError, match="merge_lists.*target_poc"):
        make(**dict(BASE, motion=MOTION_B, merge_lists=5, col=dict(COL, store=a.cqt_store, target_poc=(0, 16))))
    with pytest.raises(ValueError, match="commit"):
        make(**dict(BASE, unit_trees=False, motion=MOTION_B, merge_lists=5))     # refused where commit is refused
    with pytest.raises(ValueError, match="cqt_merge_results"):
        pictures["off"][0].cqt_merge_results()
    with pytest.raises(ValueError):
        pictures["on"][0].step_banded(hv)
