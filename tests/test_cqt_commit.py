"""Acting on the decided coding quadtree (havoc_mi355x_cqt_commit): of the searched units the final coding units of every decided CTU into one picture of three planes,
and one record per MinCb cell.

CPU (-m "not gpu"): search/cqt_decision.hpp's commitCqt (tests/cqt_commit_client.cpp, compiled at test time) against the numpy restatement tests/cqt_commit_tools.
commit_picture, byte for byte, on synthetic cases; the branches those cases reach, asserted by name; the library surface.  GPU (-m gpu): the kernel against the
restatement -- every destination byte, the padding and the undecided CTUs still holding the sentinel, every cell -- its contract (inputs untouched, graph replay) and
its EINVAL cases.
"""
import collections
import os

import numpy as np
import pytest

import cqt_commit_tools as M
import cqt_tools as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(M.CASES)


@pytest.fixture(scope="module")
def cases():
    """{name: (case, the restatement's result, its branch counters)}, computed once"""
    out = {}
    for name in NAMES:
        case, tags = M.make_case(**M.CASES[name]), collections.Counter()
        out[name] = (case, M.commit_picture(case, tags), tags)
    return out


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_cases_reach_every_branch(cases):
    """by name; and the named cases hold what their names say"""
    tags = collections.Counter()
    for name in NAMES:
        tags.update(cases[name][2])
    missing = [k for k in M.REQUIRED_TAGS + ("refused", "not_its_node") if not tags[k]]
    assert not missing, missing
    for name in ("136x72_8bit", "136x72_10bit"):        # each sample size takes every way a unit is committed
        assert all(cases[name][2][k] for k in M.COMMITTED), (name, cases[name][2])
    for name in ("40x24_8bit", "40x24_10bit"):
        assert all(cases[name][2][k] for k in ("coded_depth0", "coded_depth1", "coded_8_shared_chroma", "no_residual", "skipped", "not_final")), (name, cases[name][2])
    case, want, tags = cases["136x72_ctu_undecided"]
    assert tags["ctu_undecided"] > 0 and (want["cells"]["unit"][:8, 8:16] == -1).all() and (want["cells"]["unit"][:8, :8] >= 0).all()
    assert cases["40x24_final_refused"][2]["refused"] == 2 and not any(cases[name][2]["refused"] for name in NAMES if name != "40x24_final_refused")
    case, want, tags = cases["136x72_none_decided"]
    assert tags["ctu_undecided"] + tags["no_such_node"] == len(case["units"]) and tags["ctu_undecided"] > 0 and not any(tags[k] for k in M.COMMITTED)
    fresh = M.sentinels(case)
    assert want["rec_y"].tobytes() == fresh["rec_y"].tobytes() and want["rec_c"].tobytes() == fresh["rec_c"].tobytes()
    assert (want["cells"].view(np.uint8) == 0xff).all()


def test_restatement_tiles_the_decided_ctus(cases):
    """the committed units cover every cell of a decided CTU exactly once (no sample is written twice: why the kernel needs no atomics), the cells of a unit form its
    square, and no sentinel is left inside a decided CTU while the padding keeps it"""
    for name in NAMES:
        case, want, tags = cases[name]
        ctb, mcb, W, H = case["ctb_log2"], case["min_cb_log2"], case["width"], case["height"]
        cx = -(-W >> ctb)
        cells = want["cells"]
        for (j, i), cell in np.ndenumerate(cells):
            c = ((j << mcb) >> ctb) * cx + ((i << mcb) >> ctb)
            assert (cell["unit"] >= 0) == (case["ctus"][c]["decided"] == 1) or (tags["refused"] and cell["unit"] == -1), (name, j, i)
        for p in np.unique(cells["unit"][cells["unit"] >= 0]):
            u = case["units"][p]
            inside = np.zeros(cells.shape, bool)
            s = 1 << (u["log2_size"] - mcb)
            inside[u["y0"] >> mcb:(u["y0"] >> mcb) + s, u["x0"] >> mcb:(u["x0"] >> mcb) + s] = True
            assert ((cells["unit"] == p) == inside).all(), (name, p)
        assert sum(tags[k] for k in ("coded_depth0", "coded_depth1", "coded_64", "no_residual", "skipped")) == len(np.unique(cells["unit"][cells["unit"] >= 0]))
        y = want["rec_y"][:case["rec_y_size"]].reshape(-1, case["rec_stride"])
        sentinel = M.sentinels(case)["rec_y"][0]
        pad = case["rec_origin"] % case["rec_stride"]
        assert (y[:pad] == sentinel).all() and (y[pad + H:] == sentinel).all() and (y[:, :pad] == sentinel).all() and (y[:, pad + W:] == sentinel).all(), name


@pytest.mark.parametrize("name", NAMES)
def test_commit_cqt_hpp_is_the_restatement(cases, name):
    """commitCqt, CTU by CTU: every destination byte and every cell"""
    case, want, tags = cases[name]
    got, done = M.Client().commit_picture(case)
    assert M.same(got, want) is None, M.same(got, want)
    assert done == sum(tags[k] for k in ("coded_depth0", "coded_depth1", "coded_64", "no_residual", "skipped"))


def test_library_surface():
    from turingcodec_amd import havoc
    L, names = havoc._load()
    assert L.havoc_mi355x_cqt_commit and "cqt_commit" in names and "havoc_mi355x_cqt_commit" in havoc.exported_symbols()
    assert havoc.CQT_CELL_DT.itemsize == 24 and havoc.CQT_CELL_DT == M.CELL_DT
    assert [M.CELL_DT.fields[k][1] for k in M.CELL_DT.names] == [0, 4, 8, 16, 17, 18, 19, 20]
    import ctypes
    assert ctypes.sizeof(havoc.CqtCommitArgs) == 288 and havoc.CqtCommitArgs.d_units.offset == 24 and havoc.CqtCommitArgs.d_cells.offset == 280
    header = open(os.path.join(ROOT, "include", "havoc_mi355x.h")).read()
    for text in ("havoc_mi355x_cqt_commit(", "} havoc_mi355x_cqt_cell;   /* sizeof: 24 */", "} havoc_mi355x_cqt_commit_args;"):
        assert text in header, text


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def hv():
    from turingcodec_amd.havoc import Havoc
    h = Havoc(stream="new")
    yield h
    h.close()


def _up(hv, a):
    import torch
    with torch.cuda.stream(hv.tstream):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(hv.device)


INPUTS = ("units", "node_cu", "ctus", "nodes", "cu", "rqt", "tree", "zero_at", "one_at", "chroma_at", "pred_y", "pred_c", "pred_off", "best", "unit_cand")


def _device(hv, case, drop_unused=False):
    """the case on the device -> (the input tensors by name, the destination tensors pre-filled with the sentinel, a function that makes the call)"""
    t = {k: _up(hv, case[k]) for k in INPUTS}
    t["cand_mv"] = None if case["cand_mv"] is None else _up(hv, case["cand_mv"])
    used = {case["ctb_log2"] - d - (1 if k else 0) for d in range(case["ctb_log2"] - case["min_cb_log2"] + 1) for k in (0, 1)}
    luma = [_up(hv, a) if not drop_unused or s in used else None for s, a in zip((2, 3, 4, 5), case["luma"])]
    chroma = [_up(hv, a) for a in case["chroma"]]
    fresh = M.sentinels(case)
    dst = {k: _up(hv, fresh[k]) for k in ("rec_y", "rec_c", "cells")}

    def run():
        hv.cqt_commit_d(case["bit_depth"], case["width"], case["height"], case["ctb_log2"], case["min_cb_log2"], t["units"].view(hv.torch.int32), t["node_cu"], t["ctus"],
                        t["nodes"], t["cu"], t["rqt"], t["tree"], t["zero_at"], t["one_at"], t["chroma_at"], luma, chroma, t["pred_y"], case["pred_stride"], t["pred_c"],
                        case["pred_stride_c"], t["pred_off"], t["best"], t["unit_cand"], t["cand_mv"], dst["rec_y"], case["rec_origin"], case["rec_stride"], dst["rec_c"],
                        case["cb_origin"], case["cr_origin"], case["c_stride"], dst["cells"])

    return t, dst, run


def _download(hv, case, dst):
    hc, wc = case["height"] >> case["min_cb_log2"], case["width"] >> case["min_cb_log2"]
    return dict(rec_y=hv.down(dst["rec_y"], np.uint8).view(case["dt"]), rec_c=hv.down(dst["rec_c"], np.uint8).view(case["dt"]),
                cells=hv.down(dst["cells"], np.uint8).view(M.CELL_DT).reshape(hc, wc))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_device_matches_restatement(hv, cases, name):
    """every destination byte -- the padding border and undecided CTUs still the sentinel -- and every cell, those of undecided CTUs all-ones; no input is written"""
    case, want, _ = cases[name]
    t, dst, run = _device(hv, case, drop_unused=name.startswith("40x24"))
    run()
    got = _download(hv, case, dst)
    assert M.same(got, want) is None, M.same(got, want)
    for k in INPUTS:
        assert hv.down(t[k], np.uint8).tobytes() == np.ascontiguousarray(case[k]).tobytes(), k


@pytest.mark.gpu
def test_device_replays_from_a_graph(hv, cases):
    """the fill and the launch are captured: a replay over dirtied destinations gives the same bytes, twice"""
    import torch
    case, want, _ = cases["136x72_ctu_undecided"]
    t, dst, run = _device(hv, case)
    run()
    assert M.same(_download(hv, case, dst), want) is None
    graph = hv.graph_capture(run)
    fresh = M.sentinels(case)
    for k in range(2):
        with torch.cuda.stream(hv.tstream):
            for key in dst:
                dst[key].copy_(torch.from_numpy(np.ascontiguousarray(fresh[key]).view(np.uint8).reshape(-1).copy()))
        hv.graph_launch(graph)
        assert M.same(_download(hv, case, dst), want) is None, k
    hv.graph_destroy(graph)


@pytest.mark.gpu
def test_device_einval(hv, cases):
    import ctypes
    from turingcodec_amd import havoc
    case, _, _ = cases["40x24_8bit"]
    t, dst, run = _device(hv, case)
    run()
    f = hv.L.havoc_mi355x_cqt_commit

    def args(**change):
        a = havoc.CqtCommitArgs()
        a.bit_depth, a.width, a.height, a.ctb_log2, a.min_cb_log2, a.n = 8, 40, 24, 4, 3, len(case["units"])
        for k, v in (("d_units", "units"), ("d_node_cu", "node_cu"), ("d_ctu", "ctus"), ("d_node", "nodes"), ("d_cu", "cu"), ("d_choice", "rqt"), ("d_tree_choice", "tree"),
                     ("d_zero_at", "zero_at"), ("d_one_at", "one_at"), ("d_chroma_at", "chroma_at"), ("d_pred_y", "pred_y"), ("d_pred_c", "pred_c"),
                     ("d_pred_off", "pred_off"), ("d_best", "best"), ("d_unit_cand", "unit_cand"), ("d_cand_mv", "cand_mv")):
            setattr(a, k, t[v].data_ptr())
        a.d_rec_y, a.d_rec_c, a.d_cells = dst["rec_y"].data_ptr(), dst["rec_c"].data_ptr(), dst["cells"].data_ptr()
        a.pred_stride, a.pred_stride_c, a.rec_stride, a.c_stride = case["pred_stride"], case["pred_stride_c"], case["rec_stride"], case["c_stride"]
        a.rec_origin, a.cb_origin, a.cr_origin = case["rec_origin"], case["cb_origin"], case["cr_origin"]
        for k, v in change.items():
            setattr(a, k, v)
        return a

    def call(a):        # (a is kept alive over the call)
        hv._ck(f(hv.h, ctypes.addressof(a)))

    call(args(n=0))     # the arguments as made here are accepted; without units only the fill runs
    assert (hv.down(dst["cells"], np.uint8) == 0xff).all()
    # none of the calls below reaches the device: args() leaves the piece pointers null, and every call is refused before a unit is read
    with pytest.raises(havoc.HavocError, match="null"):
        hv._ck(f(hv.h, None))
    required = ["d_units", "d_node_cu", "d_ctu", "d_node", "d_cu", "d_choice", "d_tree_choice", "d_zero_at", "d_one_at", "d_chroma_at", "d_pred_y", "d_pred_c", "d_pred_off",
                "d_best", "d_unit_cand", "d_rec_y", "d_rec_c", "d_cells"]
    for k in required:
        with pytest.raises(havoc.HavocError, match="null"):
            call(args(**{k: None}))
    for k, v, what in (("bit_depth", 7, "bit_depth"), ("bit_depth", 17, "bit_depth"), ("width", 0, "width"), ("width", 44, "width"), ("height", -8, "height"),
                       ("height", 20, "height"), ("ctb_log2", 3, "ctb_log2"), ("ctb_log2", 7, "ctb_log2"), ("min_cb_log2", 2, "min_cb_log2"), ("min_cb_log2", 5, "min_cb_log2"),
                       ("n", -1, "n < 0"), ("pred_stride", 0, "stride"), ("pred_stride_c", -1, "stride"), ("rec_stride", 0, "stride"), ("c_stride", -4, "stride"),
                       ("rec_origin", -1, "origin"), ("cb_origin", -1, "origin"), ("cr_origin", -1, "origin")):
        with pytest.raises(havoc.HavocError, match=what):
            call(args(**{k: v}))
    for out in ("d_rec_y", "d_rec_c", "d_cells"):
        for k in ("d_units", "d_node", "d_cu", "d_pred_y", "d_pred_c", "d_cand_mv"):
            with pytest.raises(havoc.HavocError, match="destination"):
                call(args(**{out: getattr(args(), k)}))
    a = args()
    a.luma_pieces[1] = dst["rec_y"].data_ptr()
    with pytest.raises(havoc.HavocError, match="destination"):
        call(a)
    for a_, b_ in (("d_rec_c", "d_rec_y"), ("d_cells", "d_rec_y"), ("d_cells", "d_rec_c")):
        with pytest.raises(havoc.HavocError, match="distinct"):
            call(args(**{a_: getattr(args(), b_)}))
    for k in ("d_cells", "d_cand_mv", "d_node", "d_units"):
        with pytest.raises(havoc.HavocError, match="aligned"):
            call(args(**{k: getattr(args(), k) + 4}))
