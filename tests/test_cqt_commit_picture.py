"""DecisionPicture(commit=True): the quadtree decided over the searched units is acted on -- its final coding units into cqt_recon / cqt_crecon and one record per 8x8
cell into cqt_cells (havoc_mi355x_cqt_commit), inside the replayed graph, directly behind cqt_launch.  -m gpu.

The host side takes the DOWNLOADED records, candidate pieces and unit prediction planes and restates the call (tests/cqt_commit_tools.commit_picture); the picture is
then tied to the costs the decisions were made with: the SSD of every committed unit against the source is the SSD its records carry, to the integer.  Two pictures:
136 x 72 -- 2 x 2 CTUs, the last column and row 8 wide / high -- and 416 x 240; 8-bit, QP 32, seed 21, three steps, the third from the graph.
"""
import collections

import numpy as np
import pytest

import cqt_commit_tools as M
import cqt_tools as Q

pytestmark = pytest.mark.gpu

PICTURES = {"136x72": (136, 72, 21), "416x240": (416, 240, 21)}       # width, height, seed
BASE = dict(tree_rates=True, pu_modes=True, cu_close=True, cqt=True, unit_trees=True)


@pytest.fixture(scope="module")
def hv():
    from turingcodec_amd.havoc import Havoc
    h = Havoc(stream="new")
    yield h
    h.close()


@pytest.fixture(scope="module", params=list(PICTURES))
def pictures(hv, request):
    """the picture with commit and the same picture without it: three steps each, the third replayed from the graph"""
    from turingcodec_amd.decisions import DecisionPicture
    w, h, seed = PICTURES[request.param]
    out = {}
    for name, options in (("on", dict(BASE, commit=True)), ("off", BASE)):
        dp = DecisionPicture(hv, w, h, 8, 32, seed=seed, threads=8, intra=False, **options)
        for _ in range(3):
            searched = dp.step()
        assert all(dp._graphs.values()) and len(dp._graphs) == 1
        out[name] = (dp, searched)
    return out


@pytest.fixture(scope="module")
def host(pictures):
    """the inputs of the call as the launches before it left them on the device, downloaded once, as a case of cqt_commit_tools; what the call left; the restatement"""
    dp, _ = pictures["on"]
    hv, P, U = dp.hv, dp.pu_plan, dp.unit_plan
    d, q, cu = dp.unit_tree_decisions(planes=True), dp.cqt_decisions, dp.cu_decisions
    W, H, hw, hh = dp.W, dp.H, dp.W // 2, dp.H // 2
    piece = lambda groups, sizes: [hv.down(groups[s]["piece"], dp.dt) if s in groups else None for s in sizes]
    case = dict(bit_depth=8, S=1, dt=dp.dt, width=W, height=H, ctb_log2=6, min_cb_log2=3, units=d["units"], node_cu=q["node_cu"], ctus=q["ctus"], nodes=q["nodes"],
                cu=cu["records"], rqt=d["choice"], tree=d["tree_choice"], zero_at=U["zero_at"], one_at=U["one_at"], chroma_at=U["chroma_at"],
                luma=piece(U["sizes"], (2, 3, 4, 5)), chroma=piece(U["csizes"], (2, 3, 4)), pred_y=d["pred"].reshape(-1), pred_c=d["cpred"].reshape(-1), pred_stride=W,
                pred_stride_c=hw, pred_off=U["select_jobs"]["dst_off"], best=dp.pu_decisions["mode"], unit_cand=d["unit_cand"],
                cand_mv=hv.down(P["d_cand_mv"], np.int16).reshape(-1, 2, 2), rec_y_size=W * H, rec_origin=0, rec_stride=W, rec_c_size=2 * hw * hh, cb_origin=0,
                cr_origin=hw * hh, c_stride=hw)
    tags = collections.Counter()
    return dict(case=case, got=dp.cqt_commit_results(), want=M.commit_picture(case, tags), tags=tags)


def test_planes_and_cells_are_the_restatement(pictures, host):
    dp, _ = pictures["on"]
    case, got, want, tags = host["case"], host["got"], host["want"], host["tags"]
    assert (case["ctus"]["decided"] == 1).all() and not dp.cqt_decisions["gave_up"]
    assert got["recon"].shape == (dp.H, dp.W) and got["crecon"].shape == (2, dp.H // 2, dp.W // 2) and got["cells"].shape == (dp.H // 8, dp.W // 8)
    assert np.array_equal(got["recon"], want["rec_y"].reshape(dp.H, dp.W))
    assert np.array_equal(got["crecon"], want["rec_c"].reshape(2, dp.H // 2, dp.W // 2))
    assert got["cells"].tobytes() == want["cells"].tobytes()
    assert got["recon"].any() and got["crecon"][0].any() and got["crecon"][1].any()
    assert sum(tags[k] for k in ("coded_depth0", "coded_depth1", "coded_64", "no_residual", "skipped")) == int(case["ctus"]["n_cus"].sum())
    print("units", len(case["units"]), "|", {k: tags[k] for k in M.COMMITTED + ("not_final", "ctu_undecided", "not_its_node", "refused", "no_such_node")})
    # the padding of the destinations is nobody's yet: still as allocated
    y = dp.hv.down(dp.cqt_recon, dp.dt)[:dp.n].reshape(-1, dp.stride)
    assert not y[:dp.PAD].any() and not y[dp.PAD + dp.H:].any() and not y[:, :dp.PAD].any() and not y[:, dp.PAD + dp.W:].any()
    assert dp.cqt_commit_results() is got


def test_cells_tile_the_picture_with_the_decided_units(pictures, host):
    """every cell has a unit, the cells of a unit form exactly its square, and log2_size is what the depth map says"""
    dp, _ = pictures["on"]
    cells, u = host["got"]["cells"], host["case"]["units"]
    assert (cells["unit"] >= 0).all()
    units = np.unique(cells["unit"])
    assert len(units) == int(host["case"]["ctus"]["n_cus"].sum())
    for p in units:
        x, y, s = int(u["x0"][p]) >> 3, int(u["y0"][p]) >> 3, 1 << (int(u["log2_size"][p]) - 3)
        inside = np.zeros(cells.shape, bool)
        inside[y:y + s, x:x + s] = True
        assert ((cells["unit"] == p) == inside).all(), p
        assert (cells["log2_size"][inside] == u["log2_size"][p]).all()
    depth = dp.cqt_decisions["depth"][:dp.H // 8, :dp.W // 8]
    assert np.array_equal(cells["log2_size"], 6 - depth)


def test_committed_units_carry_the_ssd_their_decisions_were_made_with(pictures, host):
    """integer-exact: CODED -> the standing tree's luma SSDs and chroma_ssd; left at the prediction -> cu_close's pred_ssd per plane"""
    dp, _ = pictures["on"]
    case, got = host["case"], host["got"]
    pad, c2, hw, hh = dp.PAD, dp.PAD // 2, dp.W // 2, dp.H // 2
    src = [dp.host_planes[0].reshape(-1, dp.stride)[pad:pad + dp.H, pad:pad + dp.W]]
    src += [dp.host_chroma[k].reshape(-1, dp.cstride)[c2:c2 + hh, c2:c2 + hw] for k in (0, 3)]
    rec = [got["recon"], got["crecon"][0], got["crecon"][1]]
    pred_ssd = dp.cu_decisions["pred_ssd"]
    counts = collections.Counter()
    for p in np.unique(got["cells"]["unit"]):
        u, r, t = case["units"][p], case["rqt"][p], case["tree"][p]
        x, y, n = int(u["x0"]), int(u["y0"]), 1 << int(u["log2_size"])
        ssd = []
        for c in range(3):
            xs, ys, m = (x, y, n) if c == 0 else (x // 2, y // 2, n // 2)
            e = src[c][ys:ys + m, xs:xs + m].astype(np.int64) - rec[c][ys:ys + m, xs:xs + m]
            ssd.append(int((e * e).sum()))
        outcome = int(case["cu"][p]["outcome"])
        counts[outcome] += 1
        if outcome == Q.CODED:
            zero = r["depth"] == 0 and r["tried_zero"]
            assert ssd[0] == (int(r["zero"]["ssd"]) if zero else int(r["one"]["ssd"].astype(np.int64).sum())), p
            assert ssd[1] + ssd[2] == int(t["chroma_ssd_zero"] if zero else t["chroma_ssd_one"]), p
        else:
            assert outcome in (Q.NO_RESIDUAL, Q.SKIPPED) and ssd == [int(v) for v in pred_ssd[p]], p
    print("committed units by outcome: coded", counts[Q.CODED], "no residual", counts[Q.NO_RESIDUAL], "skipped", counts[Q.SKIPPED])


def test_cells_carry_the_decided_mode_candidate_and_vectors(pictures, host):
    dp, searched = pictures["on"]
    cells, n = host["got"]["cells"], len(dp.pus)
    unit = cells["unit"]
    mode = dp.pu_decisions["mode"]
    assert np.array_equal(cells["pred"], mode[unit]) and np.array_equal(cells["cand"], dp.unit_tree_decisions()["unit_cand"][unit])
    assert np.array_equal(cells["cand"], dp.pu_plan["first"][unit] + mode[unit])
    uni, bi = searched[0]["mv"].reshape(n, 2, 2), dp.bi_results["mv"].reshape(n, 2, 2)
    want = np.zeros((n, 2, 2), np.int16)
    want[mode == 0, 0], want[mode == 1, 1], want[mode == 2] = uni[mode == 0, 0], uni[mode == 1, 1], bi[mode == 2]
    assert np.array_equal(cells["mv"], want[unit])
    assert np.array_equal(cells["outcome"], dp.cu_decisions["records"]["outcome"][unit])
    coded = cells["outcome"] == Q.CODED
    assert not cells["cbf"][~coded].any() and not cells["tr_depth"][~coded].any() and (cells["cbf"][coded] != 0).all()


def test_the_step_is_otherwise_unchanged(pictures):
    """the same options without commit leave recon, crecon, cells and every record of the options byte-identical"""
    (on, r_on), (off, r_off) = pictures["on"], pictures["off"]
    assert not hasattr(off, "cqt_recon") and not hasattr(off, "cqt_cells") and "d_cand_mv" not in off.pu_plan
    down = lambda dp, t: dp.hv.down(t, dp.dt)
    def chroma_area(dp):
        # (the picture's part of each plane: crecon's lower padding holds the legacy plan's dump block, where every candidate outside a chosen tree is written in no
        # order -- nobody's bytes, different from run to run)
        c2, c = dp.PAD // 2, down(dp, dp.crecon)
        return np.stack([c[k * dp.cpe:k * dp.cpe + dp.cn].reshape(-1, dp.cstride)[c2:c2 + dp.H // 2, c2:c2 + dp.W // 2] for k in (0, 1)])

    assert np.array_equal(down(on, on.recon), down(off, off.recon)) and down(on, on.recon).any()
    assert np.array_equal(chroma_area(on), chroma_area(off)) and chroma_area(on).any()
    assert np.array_equal(on.cells.view(np.uint8), off.cells.view(np.uint8))

    def same(a, b):
        assert set(a) == set(b)
        return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) if isinstance(a[k], np.ndarray) else a[k] == b[k]
                   for k in a)

    assert same(on.pu_decisions, off.pu_decisions) and same(on.unit_tree_decisions(), off.unit_tree_decisions())
    assert same(on.cu_decisions, off.cu_decisions) and same(on.cqt_decisions, off.cqt_decisions)
    assert np.array_equal(r_on[0], r_off[0]) and np.array_equal(r_on[1], r_off[1])
    assert len(on._graphs) == 1 and len(off._graphs) == 1 and all(on._graphs.values())
    with pytest.raises(ValueError, match="commit"):
        off.cqt_commit_results()


def test_commit_is_refused_without_its_options(hv, pictures):
    from turingcodec_amd.decisions import DecisionPicture
    w, h = pictures["on"][0].W, pictures["on"][0].H
    for options in (dict(tree_rates=True, pu_modes=True, cu_close=True, cqt=True), dict(tree_rates=True, pu_modes=True, cu_close=True, unit_trees=True), {}):
        with pytest.raises(ValueError, match="commit"):
            DecisionPicture(hv, w, h, 8, 32, seed=21, threads=8, intra=False, commit=True, **options)
    with pytest.raises(ValueError):
        DecisionPicture(hv, w, h, 8, 32, seed=21, threads=8, intra=False, commit=True, **dict(BASE, search_on_device=False))
    with pytest.raises(ValueError):
        pictures["on"][0].step_banded(hv)
