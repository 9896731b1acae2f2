"""The committed quadtree's motion as the next picture's collocated store (havoc_mi355x_cqt_motion_store) and the temporal candidate of a picture's prediction units
from such a store (havoc_mi355x_temporal_candidates).

CPU (-m "not gpu"): search/cqt_decision.hpp's cqtMotionStore and search/amvp.hpp's deriveTemporalCandidate (tests/cqt_motion_client.cpp, compiled at test time) against
the numpy restatements of tests/cqt_motion_tools, byte for byte; the REFERENCE PIN of the store -- a real StateCollocatedMotion filled through the reference's own
fillRectangle once per committed unit (tests/cqt_motion_shim.cpp) holds the restated entries, and so does the committed golden file, which travels where the reference
does not; the branches the cases reach, by name.  (The candidate's rule is pinned where it is stated: tests/test_trace_pin.py holds deriveTemporalCandidate against
112 280 derivations of the traced reference encoder.)  GPU (-m gpu): both kernels against the restatements over sentinel-filled destinations, graph replay, EINVAL,
n == 0.
"""
import collections
import os

import numpy as np
import pytest

import cqt_motion_tools as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_ref = pytest.mark.skipif(M.reference_dir() is None, reason="reference sources not present (the shim compiles them at test time)")
STORES, CANDS = list(M.STORE_CASES), list(M.CAND_CASES)


@pytest.fixture(scope="module")
def stores():
    """{name: (case, the restated store, its branch counters)}, computed once"""
    out = {}
    for name in STORES:
        case, tags = M.make_store_case(name), collections.Counter()
        out[name] = (case, M.restate_store(case, tags), tags)
    return out


@pytest.fixture(scope="module")
def cands():
    """{name: (case, the restated records, their branch counters)}, computed once"""
    out = {}
    for name in CANDS:
        case, tags = M.make_cand_case(name), collections.Counter()
        out[name] = (case, M.temporal_candidates(case["params"], case["store"], case["pus"], tags), tags)
    return out


@pytest.fixture(scope="module")
def client():
    return M.Client()


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_store_cases_reach_every_branch(stores):
    """a condition on the inputs: every tag of STORE_TAGS occurs; the named cases hold what their names say"""
    tags = collections.Counter()
    for name in STORES:
        tags.update(stores[name][2])
    missing = [k for k in M.STORE_TAGS if not tags[k] > 0]
    assert not missing, (missing, tags)
    case, want, t = stores["136x72"]
    assert want.shape == (5, 9) and t["right_partial_column"] == 5 and t["bottom_partial_row"] == 9 and not t["undecided"]
    case, want, t = stores["136x72_ctu_undecided"]
    assert t["undecided"] == 16 and not want[:4, 4:8].view(np.uint8).any() and want["pred_flag"][:4, :4].any(axis=-1).all()
    case, want, t = stores["64x64_one_unit"]
    assert t["unit64_sixteen_entries"] == 1 and t["pred2"] == 16 and len({e.tobytes() for e in want.reshape(-1)}) == 1
    case, want, t = stores["64x64_mincb16"]
    assert not t["unit8_with_entry"] and not t["unit8_without_entry"]       # MinCb 16: a committed cell is an entry's whole area
    for name in STORES:
        want = stores[name][1]
        assert not want["long_term"].any() and not want["reserved"].any(), name


def test_candidate_cases_reach_every_branch(cands):
    """a condition on the inputs: every tag of CAND_TAGS occurs -- every choice of cell and list, every clip, both edges, every unit size"""
    tags = collections.Counter()
    for name in CANDS:
        tags.update(cands[name][2])
    missing = [k for k in M.CAND_TAGS if not tags[k] > 0]
    assert not missing, (missing, tags)
    for name in CANDS:
        case, want, _ = cands[name]
        outside = want[-6:]
        assert not outside.view(np.uint8).any(), name                   # the six units that are not inside the picture: no candidate, every byte zero
        none = want["available"] == 0
        assert not want["mv"][none].any() and (want["source"][none] == M.NONE).all() and (want["source"][~none] != M.NONE).all(), name
        assert set(np.unique(want["available"])) == {0, 1}, name


@pytest.mark.parametrize("name", STORES)
def test_cqt_motion_store_hpp_is_the_restatement(stores, client, name):
    """cqtMotionStore: every entry byte for byte, dense rows, nothing behind the last entry"""
    case, want, _ = stores[name]
    assert client.motion_store(case).tobytes() == M.flat(want).tobytes()


@pytest.fixture(scope="module")
def shim():
    return M.Shim()         # (compiled once; asked for by tests behind needs_ref only)


@needs_ref
@pytest.mark.parametrize("name", STORES)
def test_reference_store_holds_the_same_entries(stores, shim, name):
    """the pin: StateCollocatedMotion after one fillRectangle per committed unit, the units in two different orders"""
    case, want, _ = stores[name]
    view = M.shim_view(want, case["ref_poc0"], case["ref_poc1"], 3, 5)
    for order in (None, np.random.default_rng(7)):
        assert np.array_equal(shim.entries(case, 3, 5, order), view)


@pytest.mark.parametrize("name", STORES)
def test_store_matches_golden(stores, name):
    """the reference's entries as recorded (tests/golden/make_cqt_motion_golden.py): the pin where the reference sources are absent"""
    case, want, _ = stores[name]
    golden = np.load(M.golden_path())
    assert sorted(golden.files) == sorted(STORES)
    assert np.array_equal(golden[name], M.shim_view(want, case["ref_poc0"], case["ref_poc1"], *M.GOLDEN_DPB))


@pytest.mark.parametrize("name", CANDS)
def test_derive_temporal_candidate_hpp_is_the_restatement(cands, client, name):
    """deriveTemporalCandidate through the client: every record byte for byte -- col_poc == ref_poc included, this project's own rule (no motion)"""
    case, want, _ = cands[name]
    got = client.temporal_candidates(case["params"], case["store"], case["pus"])
    assert got.tobytes() == want.tobytes()


def test_library_surface():
    from turingcodec_amd import havoc, workload
    L, names = havoc._load()
    for n in ("cqt_motion_store", "temporal_candidates"):
        assert getattr(L, "havoc_mi355x_" + n) and n in names and "havoc_mi355x_" + n in havoc.exported_symbols()
    assert havoc.COL_CELL_DT == M.COL_CELL_DT and havoc.TEMPORAL_PARAMS_DT == M.PARAMS_DT and havoc.TEMPORAL_CAND_DT == M.CAND_DT and workload.PICTURE_PU_DT == M.PU_DT
    assert (havoc.TEMPORAL_NONE, havoc.TEMPORAL_BOTTOM_RIGHT, havoc.TEMPORAL_CENTRE) == (M.NONE, M.BOTTOM_RIGHT, M.CENTRE)
    header = open(os.path.join(ROOT, "include", "havoc_mi355x.h")).read()
    assert "int havoc_mi355x_cqt_motion_store(havoc_mi355x_ctx *ctx, int width, int height, int min_cb_log2, int poc, int ref_poc0, int ref_poc1," in header
    assert "int havoc_mi355x_temporal_candidates(havoc_mi355x_ctx *ctx, const havoc_mi355x_temporal_params *params, const havoc_mi355x_col_cell *d_store," in header
    assert "} havoc_mi355x_col_cell;" in header and "} havoc_mi355x_temporal_params;" in header and "} havoc_mi355x_temporal_cand;" in header


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


def _store_call(hv, case, d_cqt, d_store):
    hv.cqt_motion_store_d(case["W"], case["H"], case["min_cb_log2"], case["poc"], case["ref_poc0"], case["ref_poc1"], d_cqt, d_store)


@pytest.mark.gpu
@pytest.mark.parametrize("name", STORES)
def test_device_store_matches_restatement(hv, stores, name):
    """every entry byte for byte; the store has no bytes between its rows and none behind its last entry: the sentinel stands there; the input is not written"""
    case, want, _ = stores[name]
    expect = M.flat(want)
    d_cqt, d_store = _up(hv, case["cqt"]), _up(hv, np.full(expect.size, M.SENTINEL, np.uint8))
    _store_call(hv, case, d_cqt, d_store)
    assert hv.down(d_store, np.uint8).tobytes() == expect.tobytes()
    assert hv.down(d_cqt, np.uint8).tobytes() == np.ascontiguousarray(case["cqt"]).tobytes()


def _wide(store, extra):
    """the store with `extra` sentinel records at the end of every row -> uint8 [rows, (cols + extra) * 24]"""
    out = np.full((store.shape[0], (store.shape[1] + extra) * M.COL_CELL_DT.itemsize), M.SENTINEL, np.uint8)
    out[:, :store.shape[1] * M.COL_CELL_DT.itemsize] = np.ascontiguousarray(store).view(np.uint8).reshape(store.shape[0], -1)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", CANDS)
@pytest.mark.parametrize("extra", [0, 2])
def test_device_candidates_match_restatement(hv, cands, name, extra):
    """every record byte for byte, dense store rows and rows two records wider (whose other bytes are the sentinel: reading one would show); d_out keeps its sentinel
    beyond 2 n records; the inputs are not written"""
    case, want, _ = cands[name]
    n = len(case["pus"])
    wide = _wide(case["store"], extra)
    fresh = np.full((2 * n + 3) * 8, M.SENTINEL, np.uint8)
    d_store, d_pus, d_out = _up(hv, wide), _up(hv, case["pus"]), _up(hv, fresh)
    hv.temporal_candidates_d(case["params"], d_store, case["store"].shape[1] + extra, d_pus, n, d_out)
    got = hv.down(d_out, np.uint8)
    assert got[:2 * n * 8].tobytes() == want.tobytes() and (got[2 * n * 8:] == M.SENTINEL).all()
    assert hv.down(d_store, np.uint8).tobytes() == wide.tobytes() and hv.down(d_pus, np.uint8).tobytes() == case["pus"].tobytes()


@pytest.mark.gpu
def test_device_replays_from_a_graph(hv, stores, cands):
    """both calls captured into one graph, the candidates reading the store the first call writes: two replays, each over dirtied destinations and CHANGED committed
    cells of the same geometry"""
    import torch
    case = stores["136x72_ctu_undecided"][0]
    cc = cands["136x72_from_l0"][0]
    n = len(cc["pus"])
    sh, sw = M.store_shape(case["W"], case["H"])
    dirty_store, dirty_out = np.full(sh * sw * 24 + 48, M.SENTINEL, np.uint8), np.full((2 * n + 3) * 8, M.SENTINEL, np.uint8)
    d_cqt, d_store, d_pus, d_out = _up(hv, case["cqt"]), _up(hv, dirty_store), _up(hv, cc["pus"]), _up(hv, dirty_out)

    def run():
        _store_call(hv, case, d_cqt, d_store)
        hv.temporal_candidates_d(cc["params"], d_store, sw, d_pus, n, d_out)

    def check(cqt, what):
        store = M.motion_store(cqt, case["W"], case["H"], case["min_cb_log2"], case["ref_poc0"], case["ref_poc1"])
        assert hv.down(d_store, np.uint8).tobytes() == M.flat(store).tobytes(), what
        got = hv.down(d_out, np.uint8)
        assert got[:2 * n * 8].tobytes() == M.temporal_candidates(cc["params"], store, cc["pus"]).tobytes() and (got[2 * n * 8:] == M.SENTINEL).all(), what

    run()
    check(case["cqt"], "plain")
    graph = hv.graph_capture(run)
    for other in ("136x72", "136x72_ctu_undecided"):
        cqt = stores[other][0]["cqt"]
        with torch.cuda.stream(hv.tstream):
            d_store.copy_(torch.from_numpy(dirty_store.copy()))
            d_out.copy_(torch.from_numpy(dirty_out.copy()))
            d_cqt.copy_(torch.from_numpy(np.ascontiguousarray(cqt).view(np.uint8).reshape(-1).copy()))
        hv.graph_launch(graph)
        check(cqt, other)
    hv.graph_destroy(graph)


@pytest.mark.gpu
def test_device_store_einval(hv, stores):
    from turingcodec_amd import havoc
    case, want, _ = stores["136x72"]
    d_cqt, d_store = _up(hv, case["cqt"]), _up(hv, np.zeros(want.size * 24 + 16, np.uint8))
    f = hv.L.havoc_mi355x_cqt_motion_store
    good = dict(width=136, height=72, min_cb_log2=3, poc=8, ref0=0, ref1=16, cqt=d_cqt.data_ptr(), store=d_store.data_ptr())

    def call(**change):
        a = dict(good, **change)
        hv._ck(f(hv.h, a["width"], a["height"], a["min_cb_log2"], a["poc"], a["ref0"], a["ref1"], a["cqt"], a["store"]))

    call()              # the arguments as made here are accepted
    assert hv.down(d_store, np.uint8)[:want.size * 24].tobytes() == want.tobytes()
    call(ref0=8 - 32767, ref1=8 + 32768)        # the ends of DiffPicOrderCnt's range are inside it
    # none of the calls below reaches the device
    for k in ("cqt", "store"):
        with pytest.raises(havoc.HavocError, match="null"):
            call(**{k: None})
    for k, v, what in (("min_cb_log2", 2, "min_cb_log2"), ("min_cb_log2", 7, "min_cb_log2"), ("width", 0, "width"), ("width", -8, "width"), ("width", 132, "width"),
                       ("height", 0, "height"), ("height", 68, "height"), ("ref0", 8, "ref_poc"), ("ref1", 8, "ref_poc"), ("ref0", 8 - 32768, "poc difference"),
                       ("ref1", 8 + 32769, "poc difference"), ("poc", 2 ** 31 - 1, "poc difference"), ("ref1", -2 ** 31, "poc difference")):
        with pytest.raises(havoc.HavocError, match=what):
            call(**{k: v})
    with pytest.raises(havoc.HavocError, match="width"):
        call(min_cb_log2=4)         # 136 and 72 are no multiples of 16
    with pytest.raises(havoc.HavocError, match="destination"):
        call(store=good["cqt"])
    with pytest.raises(havoc.HavocError, match="aligned"):
        call(cqt=good["cqt"] + 4)
    with pytest.raises(havoc.HavocError, match="aligned"):
        call(store=good["store"] + 4)


@pytest.mark.gpu
def test_device_candidates_einval_and_no_units(hv, cands):
    from turingcodec_amd import havoc
    case, want, _ = cands["136x72_from_l0"]
    n = len(case["pus"])
    fresh = np.full(2 * n * 8 + 16, M.SENTINEL, np.uint8)
    d_store, d_pus, d_out = _up(hv, case["store"]), _up(hv, case["pus"]), _up(hv, fresh)
    f = hv.L.havoc_mi355x_temporal_candidates
    good = dict(store=d_store.data_ptr(), stride=9, pus=d_pus.data_ptr(), n=n, out=d_out.data_ptr())

    def call(params=None, null_params=False, **change):
        a = dict(good, **change)
        p = case["params"].copy()
        for k, v in (params or {}).items():
            p[k] = v
        hv._ck(f(hv.h, None if null_params else p.ctypes.data, a["store"], a["stride"], a["pus"], a["n"], a["out"]))

    # n == 0: accepted, no launch -- the destination keeps every byte
    call(n=0)
    assert hv.down(d_out, np.uint8).tobytes() == fresh.tobytes()
    call()              # the arguments as made here are accepted
    assert hv.down(d_out, np.uint8)[:2 * n * 8].tobytes() == want.tobytes()
    # none of the calls below reaches the device
    with pytest.raises(havoc.HavocError, match="null"):
        call(null_params=True)
    for k in ("store", "pus", "out"):
        with pytest.raises(havoc.HavocError, match="null"):
            call(**{k: None})
    with pytest.raises(havoc.HavocError, match="n must"):
        call(n=-1)
    for k, v, what in (("ctb_log2", 3, "ctb_log2"), ("ctb_log2", 7, "ctb_log2"), ("pic_width", 0, "pic_width"), ("pic_width", -136, "pic_width"),
                       ("pic_height", 0, "pic_height"), ("pic_height", -8, "pic_height"), ("pic_width", 145, "store_stride"), ("target_poc", (4, 8), "target_poc"),
                       ("target_poc", (0, 4), "target_poc"), ("all_backwards", 2, "flags"), ("all_backwards", -1, "flags"), ("collocated_from_l0", 2, "flags"),
                       ("reserved", (0, 0, 1), "reserved"), ("reserved", (1, 0, 0), "reserved")):
        with pytest.raises(havoc.HavocError, match=what):
            call(params={k: v})
    for v in (8, 0, -9):
        with pytest.raises(havoc.HavocError, match="store_stride"):
            call(stride=v)
    for k in ("store", "pus"):
        with pytest.raises(havoc.HavocError, match="destination"):
            call(out=good[k])
    for k in ("store", "pus", "out"):
        with pytest.raises(havoc.HavocError, match="aligned"):
            call(**{k: good[k] + 4})
    assert hv.down(d_out, np.uint8)[:2 * n * 8].tobytes() == want.tobytes()
