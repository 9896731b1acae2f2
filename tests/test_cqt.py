"""The coding quadtree of every CTU on the device (havoc_mi355x_cqt_decide): what Search<coding_quadtree>::go decides (turing/Search.hpp:808-886) with the bits of
split_cu_flag as the reference's writer prices them (turing/Binarization.h:102-122).

CPU (-m "not gpu"): the plain-Python restatement tests/cqt_tools.decide_picture against (a) the reference's own writer and Syntax<coding_quadtree>::go over a real snake
(tests/cqt_shim.cpp, compiled at test time where the reference sources are): every priced flag's bits, ctxInc and states, and the decided trees' rates and final states
-- the identity the reference asserts itself at turing/Write.h:811-812; (b) search/cqt_decision.hpp's decideCqt; (c) the committed file tests/golden/cqt_golden.npz;
the two answers of the snake the header states, pinned; the branches the golden inputs reach, asserted by name; the library surface.  GPU (-m gpu): the kernel against
the golden file and the restatement -- every CTU record, node record, depth cell and snapshot byte -- and its contract (untouched inputs, pass-through bytes, refusals,
EINVAL, graph replay).  No test provokes a give-up: that path is read, not run.
"""
import collections
import os

import numpy as np
import pytest

import cqt_tools as Q
import sao_decision_tools as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_ref = pytest.mark.skipif(T.reference_dir() is None, reason="reference sources not present (the shim compiles them at test time)")
NAMES = list(Q.CASES)
# the sizes the device is held against the golden file and the restatement at
DEVICE_NAMES = ["136x72_wpp", "136x72_ecu_raster", "72x40_wpp_ecu", "40x24_wpp", "64x64_wpp", "64x64_raster", "64x136_wpp", "64x136_raster", "48x48_min16", "rows_12x6"]
# cases the golden file has not seen: a 12 x 6-CTU picture at CTB 64 / MinCb 8 whose rows really overlap, with and without WPP, and a partial 5 x 3
FRESH = {
    "rows_12x6_ctb64": dict(seed=21, width=768, height=384, ctb_log2=6, min_cb_log2=3, flags=Q.WPP, refuse=(17,)),
    "rows_12x6_ctb64_raster_ecu": dict(seed=22, width=768, height=384, ctb_log2=6, min_cb_log2=3, flags=Q.ECU),
    "272x144_ctb64_min16": dict(seed=23, width=272, height=144, ctb_log2=6, min_cb_log2=4, flags=Q.WPP | Q.ECU),
}


@pytest.fixture(scope="module")
def golden():
    g = np.load(Q.golden_path())
    out = {}
    for name in NAMES:
        case, res = Q.unpack(g, name)
        out[name] = dict(case=case, res=res, ref_rate=g[name + ".ref_rate"], ref_states=g[name + ".ref_states"])
    return out


@pytest.fixture(scope="module")
def restated(golden):
    """the restatement over the golden inputs, computed once: {name: (results, branch counters, flag trace)}"""
    out = {}
    for name in NAMES:
        tags, trace = collections.Counter(), []
        out[name] = (Q.decide_picture(golden[name]["case"], tags, trace), tags, trace)
    return out


@pytest.fixture(scope="module")
def fresh():
    out = {}
    for name, args in FRESH.items():
        case = Q.make_case(**args)
        out[name] = (case, Q.decide_picture(case))
    return out


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_golden_inputs_are_the_generators(golden):
    for name in NAMES:
        case, want = Q.make_case(**Q.CASES[name]), golden[name]["case"]
        for k in ("width", "height", "ctb_log2", "min_cb_log2", "flags"):
            assert case[k] == want[k], (name, k)
        assert np.array_equal(case["node_cu"], want["node_cu"]) and np.array_equal(case["cu_syntax"], want["cu_syntax"]), name
        assert case["choice"].tobytes() == want["choice"].tobytes(), name


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_golden(golden, restated, name):
    assert Q.same(restated[name][0], golden[name]["res"]) is None, Q.same(restated[name][0], golden[name]["res"])
    res = restated[name][0]
    assert np.array_equal(res["ctus"]["rate"], golden[name]["ref_rate"]) and np.array_equal(res["cu_syntax"][:, :3], golden[name]["ref_states"])
    assert np.array_equal(res["ctus"]["cost"], res["ctus"]["rate"] + res["ctus"]["lambda_distortion"])


def test_golden_inputs_reach_every_branch(restated):
    """by name, at every depth where each can occur"""
    tags = collections.Counter()
    for name in NAMES:
        tags.update(restated[name][1])
    missing = [k for k in Q.required_tags() if not tags[k]]
    assert not missing, missing
    # the named cases hold what their names say
    assert restated["64x136_wpp"][1]["wpp_start_slice",] == 2 and restated["64x136_raster"][1]["raster_carry",] == 2
    assert restated["136x72_wpp"][1]["wpp_start_ctu1",] == 1 and restated["rows_12x6"][1]["wpp_start_ctu1",] == 5
    for name, ctu in (("136x72_wpp", 1), ("136x72_ecu_raster", 4), ("40x24_wpp", 3), ("rows_12x6", 30)):
        res = restated[name][0]
        assert [int(i) for i in np.flatnonzero(res["ctus"]["decided"] == 0)] == [ctu], name
    for name in NAMES:
        if not Q.CASES[name]["flags"] & Q.ECU:
            assert not any(k[0] == "ecu_stop" for k in restated[name][1]), name


def test_decided_tree_is_a_partition(restated, golden):
    """the final coding units tile the CTU's part of the picture exactly, the depth map says their depth, deleted nodes lie outside the picture, and the CTU's rate is
    its final units' rates plus its final coded flags"""
    for name in NAMES:
        case, res = golden[name]["case"], restated[name][0]
        levels, cells, cx, cy, count = Q.geometry(case)
        wc, hc = case["width"] >> case["min_cb_log2"], case["height"] >> case["min_cb_log2"]
        for i in np.flatnonzero(res["ctus"]["decided"]):
            x0, y0 = (i % cx) * cells, (i // cx) * cells
            cover = np.full((cells, cells), -1)
            rate = dist = n = 0
            cand = Q.candidates(case, i)
            for d in range(levels):
                s = cells >> d
                for z in range(4 ** d):
                    nd = res["nodes"][i, Q.first(d) + z]
                    x = sum((z >> 2 * b & 1) << b for b in range(d)) * s
                    y = sum((z >> (2 * b + 1) & 1) << b for b in range(d)) * s
                    if nd["choice"] == Q.DELETED:
                        assert x0 + x >= wc or y0 + y >= hc
                    if nd["flags"] & Q.FINAL and nd["choice"] == Q.CU:
                        assert (cover[y:y + s, x:x + s] == -1).all()
                        cover[y:y + s, x:x + s] = d
                        rate, dist, n = rate + cand[Q.first(d) + z][0], dist + cand[Q.first(d) + z][1], n + 1
            inside = np.zeros((cells, cells), bool)
            inside[:max(0, min(cells, hc - y0)), :max(0, min(cells, wc - x0))] = True
            assert ((cover >= 0) == inside).all(), (name, i)
            assert np.array_equal(np.where(inside, cover, 0), res["depth"][y0:y0 + cells, x0:x0 + cells]), (name, i)
            c = res["ctus"][i]
            assert (c["n_cus"], c["rate"], c["lambda_distortion"]) == (n, rate + c["flag_rate"], dist), (name, i)


@needs_ref
def test_snake_answers_are_the_headers():
    """what the header states and does not guess: after the slice-start reset the snake answers CtDepth -1 for a neighbour outside the picture -- left of column 0, above
    row 0 -- which is every neighbour there is at the picture's first row and column"""
    shim = Q.Shim()
    for name in ("136x72_wpp", "72x40_wpp_ecu", "40x24_wpp", "48x48_min16"):
        case = Q.make_case(**{**Q.CASES[name], "equalise": ()})
        step = 1 << case["min_cb_log2"]
        for x in range(0, case["width"], step):
            assert shim.snake_after_reset(case, x, 0)[1] == -1, (name, x)
        for y in range(0, case["height"], step):
            assert shim.snake_after_reset(case, 0, y)[0] == -1, (name, y)
    # ... and so a flag there is coded at ctxInc 0, whatever the depth
    t = dict(x0=0, y0=0, log2=6, depth=0, left=-1, up=-1, bin=1, before=[40, 50, 60])
    bits, after, inc, left, up = shim.flag(case=Q.make_case(**Q.CASES["64x64_wpp"]), t=t)
    assert (inc, left, up) == (0, -1, -1) and after[1:] == [50, 60] and (after[0], bits) == Q.bin_cost(40, 1)


@needs_ref
def test_restatement_matches_the_reference(golden, restated):
    """every flag the restatement priced -- in winning and in losing candidates -- by the reference's writer: bits, ctxInc, states, and the depths the snake answered;
    then the decided trees by the reference's Syntax<coding_quadtree>::go in coding order: every CTU's rate and three final states"""
    shim = Q.Shim()
    seen = collections.Counter()
    for name in NAMES:
        case, (res, _, trace) = golden[name]["case"], restated[name]
        for t in trace:
            assert shim.flag(case, t) == (t["bits"], t["after"], t["inc"], t["left"], t["up"]), (name, t)
            seen[t["inc"], t["bin"]] += 1
        rate, states = shim.picture(case, res)
        assert np.array_equal(rate, res["ctus"]["rate"]) and np.array_equal(states, res["cu_syntax"][:, :3]), name
        assert np.array_equal(rate, golden[name]["ref_rate"]) and np.array_equal(states, golden[name]["ref_states"]), name
    assert all(seen[i, b] for i in range(3) for b in range(2)), seen


@needs_ref
def test_restatement_matches_the_reference_on_fresh_cases(fresh):
    shim = Q.Shim()
    name = "272x144_ctb64_min16"
    case, trace = fresh[name][0], []
    res = Q.decide_picture(case, None, trace)
    for t in trace:
        assert shim.flag(case, t) == (t["bits"], t["after"], t["inc"], t["left"], t["up"]), t
    rate, states = shim.picture(case, res)
    assert np.array_equal(rate, res["ctus"]["rate"]) and np.array_equal(states, res["cu_syntax"][:, :3])


def test_restatement_is_cqt_decision_hpp(golden, restated, fresh):
    """decideCqt, CTU by CTU: every record, node, cell and state"""
    client = Q.DecisionClient()
    for name in NAMES:
        got = client.decide_picture(golden[name]["case"])
        assert Q.same(got, restated[name][0]) is None, (name, Q.same(got, restated[name][0]))
    case, res = fresh["272x144_ctb64_min16"]
    assert Q.same(client.decide_picture(case), res) is None


def test_library_surface():
    from turingcodec_amd import havoc
    L, names = havoc._load()
    assert L.havoc_mi355x_cqt_decide and L.havoc_mi355x_cqt_decide_workspace and "cqt_decide" in names
    assert havoc.CQT_CTU_DT == Q.CTU_DT and havoc.CQT_NODE_DT == Q.NODE_DT and havoc.CU_CHOICE_DT == Q.CHOICE_DT
    assert [Q.CTU_DT.fields[k][1] for k in Q.CTU_DT.names] == [0, 4, 8, 16, 24, 32] and Q.CTU_DT.itemsize == 40
    assert [Q.NODE_DT.fields[k][1] for k in Q.NODE_DT.names] == [0, 1, 2, 3, 8, 16] and Q.NODE_DT.itemsize == 24
    assert (havoc.CQT_WPP, havoc.CQT_ECU) == (Q.WPP, Q.ECU) == (1, 2)
    assert (havoc.CQT_NOT_VISITED, havoc.CQT_CU, havoc.CQT_SPLIT, havoc.CQT_DELETED) == (Q.NOT_VISITED, Q.CU, Q.SPLIT, Q.DELETED) == (0, 1, 2, 3)
    assert (havoc.CQT_NODE_FINAL, havoc.CQT_NODE_FLAG_CODED, havoc.CQT_NODE_MUST_SPLIT, havoc.CQT_NODE_ECU_STOP, havoc.CQT_NODE_NO_CANDIDATE,
            havoc.CQT_NODE_NO_SPLIT_CANDIDATE) == (Q.FINAL, Q.FLAG_CODED, Q.MUST_SPLIT, Q.ECU_STOP, Q.NO_CANDIDATE, Q.NO_SPLIT_CANDIDATE) == (1, 2, 4, 8, 16, 32)
    assert [havoc.cqt_nodes(c, m) for c, m in ((6, 3), (5, 3), (4, 3), (3, 3), (6, 4))] == [85, 21, 5, 1, 21]
    assert L.havoc_mi355x_cqt_decide_workspace(510) >= 510 * 8 + 8 and L.havoc_mi355x_cqt_decide_workspace(0) == 0
    header = open(os.path.join(ROOT, "include", "havoc_mi355x.h")).read()
    for text in ("havoc_mi355x_cqt_decide(", "havoc_mi355x_cqt_decide_workspace(", "} havoc_mi355x_cqt_ctu;         /* sizeof: 40 */", "} havoc_mi355x_cqt_node;        /* sizeof: 24 */",
                 "HAVOC_CQT_WPP = 1, HAVOC_CQT_ECU = 2", "HAVOC_CQT_NODE_NO_CANDIDATE = 16", "HAVOC_CQT_NODE_NO_SPLIT_CANDIDATE = 32"):
        assert text in header, text


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


def _decide(hv, case, flags=None):
    return hv.cqt_decide(case["width"], case["height"], case["ctb_log2"], case["min_cb_log2"], case["flags"] if flags is None else flags, case["cu_syntax"],
                         case["node_cu"], case["choice"])


def _check_refusals_and_bytes(case, got):
    """a refused CTU leaves no trace; the thirteen other snapshot bytes are the input's everywhere"""
    levels, cells, cx, cy, count = Q.geometry(case)
    assert (got["cu_syntax"][:, 3:] == np.asarray(case["cu_syntax"])[None, 3:]).all()
    for i in np.flatnonzero(got["ctus"]["decided"] == 0):
        assert got["ctus"][i].tobytes() == bytes(Q.CTU_DT.itemsize) and got["nodes"][i].tobytes() == bytes(count * Q.NODE_DT.itemsize)
        assert not got["depth"][(i // cx) * cells:(i // cx + 1) * cells, (i % cx) * cells:(i % cx + 1) * cells].any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", DEVICE_NAMES)
def test_device_matches_golden_and_restatement(hv, golden, restated, name):
    """every CTU record, node record, depth cell and snapshot byte"""
    case = golden[name]["case"]
    got = _decide(hv, case)
    assert Q.same(got, golden[name]["res"]) is None, Q.same(got, golden[name]["res"])
    assert Q.same(got, restated[name][0]) is None
    _check_refusals_and_bytes(case, got)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FRESH))
def test_device_matches_restatement_on_fresh_pictures(hv, fresh, name):
    """12 x 6 CTUs of 85 nodes: six rows in flight, each two CTUs behind the one above"""
    case, want = fresh[name]
    got = _decide(hv, case)
    assert Q.same(got, want) is None, Q.same(got, want)
    assert (got["ctus"]["decided"] == 0).sum() == len(FRESH[name].get("refuse", ()))
    _check_refusals_and_bytes(case, got)


@pytest.mark.gpu
def test_device_flags_change_the_walk(hv, golden):
    """the same inputs under the other flags are the restatement's under those flags: WPP and ecu are read, not assumed"""
    for name, flags in (("136x72_wpp", 0), ("136x72_wpp", Q.ECU), ("136x72_ecu_raster", Q.WPP), ("64x136_raster", Q.WPP | Q.ECU)):
        case = dict(golden[name]["case"], flags=flags)
        assert Q.same(_decide(hv, case), Q.decide_picture(case)) is None, (name, flags)


@pytest.mark.gpu
def test_device_contract(hv, golden, restated):
    """no input is written; guard bytes around every output and the workspace are untouched; a dirty workspace is reset by the call; the call replays from a graph,
    twice, to the same bytes"""
    import torch
    name = "136x72_wpp"
    case, want = golden[name]["case"], restated[name][0]
    levels, cells, cx, cy, count = Q.geometry(case)
    n = cx * cy
    ins = [_torch_u8(hv, case[k]) for k in ("cu_syntax", "node_cu", "choice")]
    sizes = dict(work=int(hv.L.havoc_mi355x_cqt_decide_workspace(n)), ctu=n * 40, node=n * count * 24, depth=n * cells * cells, syntax=n * 16)
    with torch.cuda.stream(hv.tstream):
        bufs = {k: torch.full((64 + (v + 7) // 8 * 8 + 64,), 200 + j, dtype=torch.uint8, device=hv.device) for j, (k, v) in enumerate(sizes.items())}

    def run():
        hv.cqt_decide_d(case["width"], case["height"], case["ctb_log2"], case["min_cb_log2"], case["flags"], ins[0], ins[1], ins[2], bufs["work"][64:-64],
                        bufs["ctu"][64:], bufs["node"][64:], bufs["depth"][64:].view(torch.int8), bufs["syntax"][64:])

    def check(what):
        raw = {k: hv.down(bufs[k], np.uint8) for k in bufs}
        for j, (k, v) in enumerate(sizes.items()):
            assert (raw[k][:64] == 200 + j).all() and (raw[k][64 + (v + 7) // 8 * 8:] == 200 + j).all(), (what, k)
        got = dict(ctus=raw["ctu"][64:64 + sizes["ctu"]].copy().view(Q.CTU_DT), nodes=raw["node"][64:64 + sizes["node"]].copy().view(Q.NODE_DT).reshape(n, count),
                   depth=raw["depth"][64:64 + sizes["depth"]].view(np.int8).reshape(cy * cells, cx * cells), cu_syntax=raw["syntax"][64:64 + sizes["syntax"]].reshape(n, 16))
        assert Q.same(got, want) is None, (what, Q.same(got, want))
        return b"".join(raw[k][64:64 + sizes[k]].tobytes() for k in ("ctu", "node", "depth", "syntax"))

    run()           # over a workspace full of 200s: done bits set, a ticket far past the rows, the give-up word raised -- the call resets it
    first = check("direct")
    for t, k in zip(ins, ("cu_syntax", "node_cu", "choice")):
        assert np.array_equal(hv.down(t, np.uint8), np.ascontiguousarray(case[k]).view(np.uint8).reshape(-1)), k
    graph = hv.graph_capture(run)
    for k in range(2):
        with torch.cuda.stream(hv.tstream):
            for name_ in ("ctu", "node", "depth", "syntax"):
                bufs[name_][64:-64].fill_(99)
        hv.graph_launch(graph)
        assert check(f"replay {k}") == first
    hv.graph_destroy(graph)


@pytest.mark.gpu
def test_device_einval(hv, golden):
    import torch
    from turingcodec_amd.havoc import HavocError
    case = golden["40x24_wpp"]["case"]
    ins = [_torch_u8(hv, case[k]) for k in ("cu_syntax", "node_cu", "choice")]
    with torch.cuda.stream(hv.tstream):
        outs = [torch.zeros(4096, dtype=torch.uint8, device=hv.device) for _ in range(5)]
    f = hv.L.havoc_mi355x_cqt_decide
    # width, height, ctb_log2, min_cb_log2, flags, cu_syntax, node_cu, choice, n_choice, work, work_bytes, ctu, node, depth, cu_syntax_out
    p = [40, 24, 4, 3, Q.WPP] + [t.data_ptr() for t in ins] + [len(case["choice"]), outs[0].data_ptr(), 4096] + [t.data_ptr() for t in outs[1:]]
    hv._ck(f(hv.h, *p))
    for k in (5, 6, 7, 9, 11, 12, 13, 14):
        q = list(p)
        q[k] = None
        with pytest.raises(HavocError, match="null"):
            hv._ck(f(hv.h, *q))
    for k, v, what in ((0, 0, "width"), (0, 44, "width"), (1, -8, "height"), (1, 20, "height"), (2, 3, "ctb_log2"), (2, 7, "ctb_log2"), (3, 2, "min_cb_log2"),
                       (3, 5, "min_cb_log2"), (4, 4, "flags"), (4, -1, "flags"), (8, -1, "n_choice"), (10, 6 * 8 + 8, "workspace")):
        q = list(p)
        q[k] = v
        with pytest.raises(HavocError, match=what):
            hv._ck(f(hv.h, *q))
    for k_out in (9, 11, 12, 13, 14):
        for k_in in (5, 6, 7):
            q = list(p)
            q[k_out] = q[k_in]
            with pytest.raises(HavocError, match="output"):
                hv._ck(f(hv.h, *q))
    for a, b in ((11, 12), (13, 14), (9, 11), (9, 14)):
        q = list(p)
        q[a] = q[b]
        with pytest.raises(HavocError, match="distinct"):
            hv._ck(f(hv.h, *q))
    for k in (5, 7, 9, 12, 13):
        q = list(p)
        q[k] += 4
        with pytest.raises(HavocError, match="aligned"):
            hv._ck(f(hv.h, *q))
