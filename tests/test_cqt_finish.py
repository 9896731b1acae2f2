"""The committed quadtree's cells as the loop filter's block structure (havoc_mi355x_cqt_block_cells): one 4x4 havoc_mi355x_cell per cell of the picture from the
record per MinCb cell havoc_mi355x_cqt_commit writes.

CPU (-m "not gpu"): search/cqt_decision.hpp's cqtBlockCells (tests/cqt_finish_client.cpp, compiled at test time) against the numpy restatement tests/cqt_finish_tools.
block_cells, byte for byte; the REFERENCE PIN -- the restated cells through the pinned per-cell derivation (oracle_derive_bs) equal the reference's own processCu /
processTu / processRc + sameMotion over unit lists made from the same committed cells unit by unit; the branches the cases reach, by name.  GPU (-m gpu): the kernel
against the restatement with dense and wider rows, graph replay, EINVAL, and derive_bs on the device's own map.
"""
import collections
import os

import numpy as np
import pytest

import cqt_finish_tools as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(F.CASES)


@pytest.fixture(scope="module")
def cases():
    """{name: (case, the restatement's cells, its branch counters)}, computed once"""
    out = {}
    for name in NAMES:
        case, tags = F.make_case(name), collections.Counter()
        out[name] = (case, F.restate(case, tags), tags)
    return out


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_cases_reach_every_branch(cases):
    """every required tag at least 5 times over the cases together (counted per 4x4 cell; min8_right / min8_bottom have one cell per unit); the named cases hold what
    their names say"""
    tags = collections.Counter()
    for name in NAMES:
        tags.update(cases[name][2])
    short = {k: tags[k] for k in F.REQUIRED_TAGS if tags[k] < 5}
    assert not short, (short, tags)
    case, want, t = cases["136x72_ctu_undecided"]
    assert t["undecided"] == 256 and (want["flags"][:16, 16:32] == F.CELL_NO_FILTER).all() and not (want["flags"][:16, :16] & F.CELL_NO_FILTER).any()
    case, want, t = cases["136x72_none_decided"]
    assert t["undecided"] == want.size and (case["cqt"].view(np.uint8) == 0xff).all()
    assert (want["flags"] == F.CELL_NO_FILTER).all() and (want["dpb_index"] == -1).all() and not want["mv"].any() and (want["tu_log2"] == 2).all()
    for name in NAMES:
        case, want, _ = cases[name]
        assert (want["qp_y"] == case["qp"]).all() and not want["reserved"].any() and not (want["flags"] & F.CELL_INTRA).any(), name
    assert cases["64x64_mincb16"][1]["tu_log2"].min() >= 3      # MinCb 16: no 8x8 unit, no 4x4 transform block


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("extra", [0, 3])
def test_cqt_block_cells_hpp_is_the_restatement(cases, name, extra):
    """cqtBlockCells: every cell byte for byte, dense rows and rows three cells wider -- whose other bytes keep the sentinel"""
    case, want, _ = cases[name]
    stride = case["W"] // 4 + extra
    got = F.Client().block_cells(case, stride)
    assert got.tobytes() == F.rows_of(want, stride).tobytes()


@pytest.mark.parametrize("name", F.FULLY_DECIDED)
def test_reference_derivation_over_the_units_gives_the_same_strengths(oracle, reference_c, cases, name):
    """the pin: what the 4x4 map means to derive_bs is what the reference derives from the decided units themselves.  (The reference has no notion of an undecided
    CTU: those cases are held against the stated rule only.)  On the units' own edges strengths 0 and 1 both occur"""
    case, want, _ = cases[name]
    W, H = case["W"], case["H"]
    lists = F.unit_lists(case["cqt"], W, H, case["min_cb_log2"], case["qp"], case["dpb0"], case["dpb1"])
    ref = reference_c.derive_bs(W, H, *lists)
    got = oracle.derive_bs(want, W, H)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    edges = F.unit_edge_strengths(case["cqt"], W, H, case["min_cb_log2"], ref[1])
    print(name, "units", len(lists[0]), "transform blocks", len(lists[2]), "unit-edge strengths 0 / 1 / 2:", np.bincount(edges, minlength=3))
    assert (edges == 0).any() and (edges == 1).any() and not (edges == 2).any()


def test_library_surface():
    from turingcodec_amd import havoc
    L, names = havoc._load()
    assert L.havoc_mi355x_cqt_block_cells and "cqt_block_cells" in names and "havoc_mi355x_cqt_block_cells" in havoc.exported_symbols()
    assert havoc.CELL_DT == F.CELL_DT and havoc.CQT_CELL_DT == F.CQT_CELL_DT
    assert (havoc.CELL_INTRA, havoc.CELL_CODED, havoc.CELL_NO_FILTER, havoc.CELL_PU_LEFT, havoc.CELL_PU_TOP) == (1, 2, 4, 8, 16)
    header = open(os.path.join(ROOT, "include", "havoc_mi355x.h")).read()
    assert "int havoc_mi355x_cqt_block_cells(havoc_mi355x_ctx *ctx, int width, int height, int min_cb_log2, int qp, int dpb_index0, int dpb_index1," in header
    assert "Argument order: ctx, width, height, min_cb_log2, qp, dpb_index0, dpb_index1, d_cqt_cells (in), d_cells (out), cells_stride." in header


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


def _run(hv, case, d_cqt, d_cells, stride):
    hv.cqt_block_cells_d(case["W"], case["H"], case["min_cb_log2"], case["qp"], case["dpb0"], case["dpb1"], d_cqt, d_cells, stride)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("extra", [0, 3])
def test_device_matches_restatement(hv, cases, name, extra):
    """every cell byte for byte; with wider rows the bytes between the rows keep their sentinel; the input is not written; the numpy-level binding gives the map"""
    case, want, _ = cases[name]
    stride = case["W"] // 4 + extra
    fresh = np.full((case["H"] // 4, stride * 16), F.SENTINEL, np.uint8)
    d_cqt, d_cells = _up(hv, case["cqt"]), _up(hv, fresh)
    _run(hv, case, d_cqt, d_cells, stride)
    assert hv.down(d_cells, np.uint8).tobytes() == F.rows_of(want, stride).tobytes()
    assert hv.down(d_cqt, np.uint8).tobytes() == np.ascontiguousarray(case["cqt"]).tobytes()
    if not extra:
        got = hv.cqt_block_cells(case["cqt"], case["W"], case["H"], case["min_cb_log2"], case["qp"], case["dpb0"], case["dpb1"])
        assert got.dtype == F.CELL_DT and got.shape == want.shape and got.tobytes() == want.tobytes()


@pytest.mark.gpu
def test_device_replays_from_a_graph(hv, cases):
    """one launch, captured: two replays, each over a dirtied destination and CHANGED committed cells of the same geometry"""
    import torch
    case, want, _ = cases["136x72_ctu_undecided"]
    stride = case["W"] // 4 + 3
    fresh = np.full((case["H"] // 4, stride * 16), F.SENTINEL, np.uint8)
    d_cqt, d_cells = _up(hv, case["cqt"]), _up(hv, fresh)
    run = lambda: _run(hv, case, d_cqt, d_cells, stride)
    run()
    assert hv.down(d_cells, np.uint8).tobytes() == F.rows_of(want, stride).tobytes()
    graph = hv.graph_capture(run)
    for other in ("136x72", "136x72_none_decided"):     # the same geometry, other cells (qp and dpb indices are the captured call's)
        changed = dict(case, cqt=cases[other][0]["cqt"])
        with torch.cuda.stream(hv.tstream):
            d_cells.copy_(torch.from_numpy(fresh.reshape(-1).copy()))
            d_cqt.copy_(torch.from_numpy(np.ascontiguousarray(changed["cqt"]).view(np.uint8).reshape(-1).copy()))
        hv.graph_launch(graph)
        assert hv.down(d_cells, np.uint8).tobytes() == F.rows_of(F.restate(changed), stride).tobytes(), other
    hv.graph_destroy(graph)


@pytest.mark.gpu
def test_device_einval(hv, cases):
    from turingcodec_amd import havoc
    case, want, _ = cases["40x24_ctb16"]
    d_cqt, d_cells = _up(hv, case["cqt"]), _up(hv, np.zeros(want.size * 16 + 16, np.uint8))
    f = hv.L.havoc_mi355x_cqt_block_cells
    good = dict(width=40, height=24, min_cb_log2=3, qp=27, dpb0=3, dpb1=3, cqt=d_cqt.data_ptr(), cells=d_cells.data_ptr(), stride=10)

    def call(**change):
        a = dict(good, **change)
        hv._ck(f(hv.h, a["width"], a["height"], a["min_cb_log2"], a["qp"], a["dpb0"], a["dpb1"], a["cqt"], a["cells"], a["stride"]))

    call()              # the arguments as made here are accepted
    assert hv.down(d_cells, np.uint8)[:want.size * 16].tobytes() == want.tobytes()
    # none of the calls below reaches the device
    for k in ("cqt", "cells"):
        with pytest.raises(havoc.HavocError, match="null"):
            call(**{k: None})
    for k, v, what in (("min_cb_log2", 2, "min_cb_log2"), ("min_cb_log2", 7, "min_cb_log2"), ("width", 0, "width"), ("width", -8, "width"), ("width", 44, "width"),
                       ("height", 0, "height"), ("height", 20, "height"), ("qp", -1, "qp"), ("qp", 52, "qp"), ("dpb0", -1, "dpb"), ("dpb0", 128, "dpb"),
                       ("dpb1", -1, "dpb"), ("dpb1", 128, "dpb"), ("stride", 9, "cells_stride"), ("stride", 0, "cells_stride"), ("stride", -10, "cells_stride")):
        with pytest.raises(havoc.HavocError, match=what):
            call(**{k: v})
    with pytest.raises(havoc.HavocError, match="width"):
        call(min_cb_log2=4)         # 40 and 24 are no multiples of 16
    with pytest.raises(havoc.HavocError, match="destination"):
        call(cells=good["cqt"])
    with pytest.raises(havoc.HavocError, match="aligned"):
        call(cqt=good["cqt"] + 4)
    with pytest.raises(havoc.HavocError, match="aligned"):
        call(cells=good["cells"] + 8)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_derive_bs_on_the_device_map_is_the_oracle_on_the_restatement(hv, oracle, cases, name):
    """the two launches chained on the device, the map never leaving it"""
    import torch
    case, want, _ = cases[name]
    W, H = case["W"], case["H"]
    n = ((W + 63) // 64 * 8 + 1) * ((H + 63) // 64 * 8 + 1)
    d_cqt, d_cells = _up(hv, case["cqt"]), _up(hv, np.zeros(want.size * 16, np.uint8))
    with torch.cuda.stream(hv.tstream):
        data, bs = torch.zeros(n, dtype=torch.int8, device=hv.device), torch.zeros(n, dtype=torch.uint8, device=hv.device)
    _run(hv, case, d_cqt, d_cells, W // 4)
    hv.derive_bs_d(d_cells, W // 4, W, H, data, bs)
    ref = oracle.derive_bs(want, W, H)
    assert np.array_equal(hv.down(data, np.int8), ref[0]) and np.array_equal(hv.down(bs, np.uint8), ref[1])
