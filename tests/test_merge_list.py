"""The merge candidate lists of a committed picture's final coding units (havoc_mi355x_cqt_merge_lists; search/merge_list.hpp).

CPU (-m "not gpu"): merge_list.hpp's deriveMergeCandidateList beside tests/merge.hpp's deriveMergeCandidates -- the text pinned against 41 880 lists of six traced
encodes -- on 200 000 seeded random rows restricted to what the call can meet and 200 000 unrestricted ones (tests/merge_list_client.cpp includes both headers); the
same function against the traced reference encoder's own recorded lists (tests/golden/merge_list_golden.npz, and the traced encoder itself where it is built); the
host form cqtMergeList against the python restatement of tests/merge_list_tools, byte for byte, on hand-built committed maps that reach every branch by name; the
library's surface.  GPU (-m gpu): the kernel against the restatement over sentinel-filled destinations with guard records, with and without the temporal table and
extra units that are not final; graph replay; every EINVAL clause; n == 0.
"""
import collections
import os
import tempfile

import numpy as np
import pytest

import merge_list_tools as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(M.CASES)
GUARD = 2


@pytest.fixture(scope="module")
def client():
    return M.Client()


@pytest.fixture(scope="module")
def cases():
    """{(name, with_temporal): (case, the restated records, their branch counters)}, computed once"""
    out = {}
    for name in NAMES:
        case = M.make(name)
        for with_temporal in (True, False):
            tags = collections.Counter()
            out[name, with_temporal] = (case, M.restate(case, with_temporal, tags), tags)
    return out


# ------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("restricted", [True, False])
def test_merge_list_hpp_is_merge_hpp(client, restricted):
    """the product's text and the pinned text give the same list and the same return value: 200 000 rows each way"""
    rows = M.random_rows(31 if restricted else 32, 200000, restricted)
    new, old, ret = client.rows(rows)
    bad = np.flatnonzero((new != old).reshape(len(rows), -1).any(axis=1) | (ret[:, 0] != ret[:, 1]))
    assert not len(bad), (len(bad), rows[bad[0]].tolist(), new[bad[0]].tolist(), old[bad[0]].tolist(), ret[bad[0]].tolist())
    # the rows are not trivial: lists that end early, lists with combined candidates, lists with zero candidates
    bi_in = ((rows[:, 8:56].reshape(-1, 6, 8)[:, :, 0] != 0) & (rows[:, 8:56].reshape(-1, 6, 8)[:, :, 1] != 0)).sum(axis=1)
    assert (ret[:, 0] == rows[:, 6]).sum() > 20000 and (ret[:, 0] < rows[:, 6]).sum() > 20000 and (ret[:, 0] == 0).sum() > 100
    assert (((new[:, :, 0] != 0) & (new[:, :, 1] != 0)).sum(axis=1) > bi_in).sum() > 1000


def test_merge_list_hpp_gives_the_encoders_recorded_lists(client):
    """the fixture: a deduplicated sample of the lists the traced reference encoder left, with its inputs (tests/golden/make_merge_list_golden.py)"""
    g = np.load(M.golden_path())
    assert sorted(g.files) == ["lists", "rows"] and os.path.getsize(M.golden_path()) < 300 * 1000
    rows, lists = g["rows"], g["lists"].astype(np.int32)
    assert rows.shape == (len(lists), 64) and lists.shape[1:] == (5, 8) and len(rows) > 1000
    new, old, _ = client.rows(rows)
    assert np.array_equal(new, lists) and np.array_equal(old, lists)
    assert (rows[:, 7] != 0).sum() > 100       # ... with the temporal candidate
    # where the traced encoder is built: every list of one whole encode, as tests/test_trace_pin.py obtains them; where it is not, the fixture alone pins the lists
    import trace_tools as tt
    if not tt.have_trace_encoder():
        return
    with tempfile.TemporaryDirectory() as work:
        _, records, _, _ = tt.run("ra_fast_qp32", work, 1)
    m = tt.MergeTrace(records)
    assert len(m) > 3000
    new, _, _ = client.rows(m.rows)
    assert np.array_equal(new, m.out)


def test_cases_reach_every_branch(cases):
    """a condition on the inputs: every tag of REQUIRED_TAGS occurs; the named cases hold what their names say"""
    tags = collections.Counter()
    for key in cases:
        tags.update(cases[key][2])
    missing = [k for k in M.REQUIRED_TAGS if not tags[k] > 0]
    assert not missing, (missing, sorted(tags.items()))
    case, want, t = cases["64x64_one_unit", False]
    assert len(case["pus"]) == 1 and t["zero_fill_5"] == 1 and want["n_real"][0] == 0 and want["match"][0] in (0, -1)
    case, want, t = cases["136x72_ctb64_max4_undecided", True]
    assert t["own_undecided"] > 0 and t["neighbour_undecided"] > 0
    case, want, t = cases["64x64_ctb64_ends", True]
    assert want["cand"]["mv"].max() == 32767 and want["cand"]["mv"].min() == -32768
    sizes = {len(cases[n, True][0]["pus"]) for n in NAMES}
    assert min(sizes) == 1 and max(sizes) == 197       # one workgroup that is not full, and four workgroups
    for (name, with_temporal), (case, want, t) in cases.items():
        final = want["n_cand"] != 0
        assert (want["n_cand"][final] == case["params"]["max_cand"][0]).all() and final.sum() == sum(t["final_%d" % s] for s in (8, 16, 32, 64)), name
        rest = want[~final]
        assert (rest["match"] == -1).all() and not rest["cand"].view(np.uint8).any() and not rest["n_real"].any() and not want["reserved"].any(), name
        assert case["extra"] == 0 or not final[-case["extra"]:].any(), name
        if not with_temporal:
            assert t["col_no_table"] == final.sum() and not t["full_at_col"], name


@pytest.mark.parametrize("with_temporal", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_cqt_merge_list_hpp_is_the_restatement(cases, client, name, with_temporal):
    """cqtMergeList: every record byte for byte, nothing before the first or behind the last"""
    case, want, _ = cases[name, with_temporal]
    assert client.host(case, with_temporal, GUARD).tobytes() == M.guarded(want, GUARD).tobytes()


def test_library_surface():
    from turingcodec_amd import havoc
    import turingcodec_amd
    L, names = havoc._load()
    assert L.havoc_mi355x_cqt_merge_lists and "cqt_merge_lists" in names and "havoc_mi355x_cqt_merge_lists" in turingcodec_amd.exported_symbols()
    assert havoc.MERGE_CAND_DT == M.MERGE_CAND_DT and havoc.MERGE_LIST_DT == M.MERGE_LIST_DT and havoc.MERGE_PARAMS_DT == M.MERGE_PARAMS_DT
    assert (havoc.MERGE_CAND_DT.itemsize, havoc.MERGE_LIST_DT.itemsize, havoc.MERGE_PARAMS_DT.itemsize) == (12, 64, 48)
    assert havoc.CQT_CELL_DT == M.CQT_CELL_DT and havoc.TEMPORAL_CAND_DT == M.TEMPORAL_CAND_DT
    header = open(os.path.join(ROOT, "include", "havoc_mi355x.h")).read()
    assert "int havoc_mi355x_cqt_merge_lists(havoc_mi355x_ctx *ctx, const havoc_mi355x_merge_params *params, const havoc_mi355x_cqt_cell *d_cqt_cells," in header
    assert "} havoc_mi355x_merge_cand;" in header and "} havoc_mi355x_merge_list;" in header and "} havoc_mi355x_merge_params;" in header


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def hv():
    h = M.private_havoc()       # (a stream of the context's own, as tests/test_cqt_motion.py has -- but not one of torch's pool: see there)
    yield h
    h.close()


def _up(hv, a):
    import torch
    with torch.cuda.stream(hv.tstream):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(hv.device)


def _fresh(n):
    return np.full((n + 2 * GUARD) * 64, M.SENTINEL, np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [2, 0])
@pytest.mark.parametrize("with_temporal", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_device_matches_restatement(hv, cases, name, with_temporal, extra):
    """every record byte for byte; the guard records before and after keep the sentinel; the inputs are not written.  extra == 0: the same table without its trailing
    units that are not final -- the records of the others do not change"""
    case, want, _ = cases[name, with_temporal]
    n = len(case["pus"]) - (case["extra"] if extra == 0 else 0)
    d_cells, d_pus, d_temporal, d_out = _up(hv, case["cells"]), _up(hv, case["pus"][:n]), _up(hv, case["temporal"][:n]), _up(hv, _fresh(n))
    hv.cqt_merge_lists_d(case["params"], d_cells, d_pus, n, d_temporal if with_temporal else None, d_out[GUARD * 64:])
    assert hv.down(d_out, np.uint8).tobytes() == M.guarded(want[:n], GUARD).tobytes()
    assert hv.down(d_cells, np.uint8).tobytes() == np.ascontiguousarray(case["cells"]).tobytes()
    assert hv.down(d_pus, np.uint8).tobytes() == case["pus"][:n].tobytes() and hv.down(d_temporal, np.uint8).tobytes() == case["temporal"][:n].tobytes()


@pytest.mark.gpu
def test_device_replays_from_a_graph(hv, cases):
    """the call captured into one graph on the context's stream: three replays, each over a dirtied destination and CHANGED cells and records of the same geometry"""
    import torch
    names = ("136x72_ctb64_max5_same_poc", "136x72_ctb64_max5_same_poc_b", "136x72_ctb64_max5_same_poc")
    case = cases[names[0], True][0]
    n = min(len(cases[k, True][0]["pus"]) for k in names)      # (the tables differ in length: the replayed call covers the units every one of them has)
    d_cells, d_pus, d_temporal, d_out = _up(hv, case["cells"]), _up(hv, case["pus"][:n]), _up(hv, case["temporal"][:n]), _up(hv, _fresh(n))

    def run():
        hv.cqt_merge_lists_d(case["params"], d_cells, d_pus, n, d_temporal, d_out[GUARD * 64:])

    def check(c, what):
        want = M.merge_lists(c["params"], c["cells"], c["pus"][:n], c["temporal"][:n])
        assert hv.down(d_out, np.uint8).tobytes() == M.guarded(want, GUARD).tobytes(), what

    run()
    check(case, "plain")
    graph = hv.graph_capture(run)
    for k, other in enumerate(names):
        c = cases[other, True][0]
        assert np.array_equal(c["params"], case["params"])
        with torch.cuda.stream(hv.tstream):
            d_out.copy_(torch.from_numpy(_fresh(n)))
            for d, a in ((d_cells, c["cells"]), (d_pus, c["pus"][:n]), (d_temporal, c["temporal"][:n])):
                d.copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()))
        hv.graph_launch(graph)
        check(c, "replay %d" % k)
    hv.graph_destroy(graph)


@pytest.mark.gpu
def test_device_einval_and_no_units(hv, cases):
    from turingcodec_amd import havoc
    case, want, _ = cases["136x72_ctb64_max5_same_poc", True]
    n = len(case["pus"])
    fresh = _fresh(n)
    d_cells, d_pus, d_temporal, d_out = _up(hv, case["cells"]), _up(hv, case["pus"]), _up(hv, case["temporal"]), _up(hv, fresh)
    f = hv.L.havoc_mi355x_cqt_merge_lists
    good = dict(cells=d_cells.data_ptr(), pus=d_pus.data_ptr(), n=n, temporal=d_temporal.data_ptr(), out=d_out.data_ptr() + GUARD * 64)

    def call(params=None, null_params=False, **change):
        a = dict(good, **change)
        p = case["params"].copy()
        for k, v in (params or {}).items():
            p[k] = v
        hv._ck(f(hv.h, None if null_params else p.ctypes.data, a["cells"], a["pus"], a["n"], a["temporal"], a["out"]))

    # n == 0: accepted, no launch -- the destination keeps every byte
    call(n=0)
    assert hv.down(d_out, np.uint8).tobytes() == fresh.tobytes()
    call()              # the arguments as made here are accepted
    assert hv.down(d_out, np.uint8).tobytes() == M.guarded(want, GUARD).tobytes()
    call(temporal=None)         # ... and so is a call without the table
    assert hv.down(d_out, np.uint8).tobytes() == M.guarded(cases["136x72_ctb64_max5_same_poc", False][1], GUARD).tobytes()
    call()
    # none of the calls below reaches the device
    with pytest.raises(havoc.HavocError, match="null"):
        call(null_params=True)
    for k in ("cells", "pus", "out"):
        with pytest.raises(havoc.HavocError, match="null"):
            call(**{k: None})
    with pytest.raises(havoc.HavocError, match="n must"):
        call(n=-1)
    for k, v, what in (("ctb_log2", 3, "ctb_log2"), ("ctb_log2", 7, "ctb_log2"), ("min_cb_log2", 2, "min_cb_log2"), ("min_cb_log2", 7, "min_cb_log2"),
                       ("pic_width", 0, "pic_width"), ("pic_width", -136, "pic_width"), ("pic_width", 132, "pic_width"), ("pic_height", 0, "pic_height"),
                       ("pic_height", -72, "pic_height"), ("pic_height", 68, "pic_height"), ("min_cb_log2", 4, "pic_width"), ("max_cand", 0, "max_cand"),
                       ("max_cand", 6, "max_cand"), ("max_cand", -1, "max_cand"), ("reserved", (1, 0, 0, 0, 0), "reserved"), ("reserved", (0, 0, 0, 0, 1), "reserved"),
                       ("reserved", (0, 0, -1, 0, 0), "reserved")):
        with pytest.raises(havoc.HavocError, match=what):
            call(params={k: v})
    with pytest.raises(havoc.HavocError, match="min_cb_log2"):
        call(params={"ctb_log2": 4, "min_cb_log2": 5})         # above ctb_log2
    for k in ("cells", "pus", "temporal"):
        with pytest.raises(havoc.HavocError, match="destination"):
            call(out=good[k])
    for k in ("cells", "pus", "temporal", "out"):
        with pytest.raises(havoc.HavocError, match="aligned"):
            call(**{k: good[k] + 4})
    assert hv.down(d_out, np.uint8).tobytes() == M.guarded(want, GUARD).tobytes()
