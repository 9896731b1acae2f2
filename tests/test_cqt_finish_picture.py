"""DecisionPicture(finish=True): the committed picture finished as turing/TaskDeblock.cpp:105-167 finishes a picture before it is used for prediction -- the committed
cells as 4x4 cells (havoc_mi355x_cqt_block_cells), boundary strengths, deblocking of cqt_recon / cqt_crecon in place, padding of the three planes -- inside the
replayed graph, directly behind cqt_commit_launch.  -m gpu.

The same picture with commit=True alone gives the unfiltered planes and the committed cells; the host side takes those through the reference's own derivation over
unit lists, its own deblocking templates and its own padBlock, and the finished planes must equal that sample for sample, padding included.  Two pictures: 136 x 72 and
416 x 240; 8-bit, QP 32, seed 21 (the content tests/test_decisions.py relies on for units with different motion next to each other), three steps, the third from the
graph.
"""
import numpy as np
import pytest

import cqt_finish_tools as F

pytestmark = pytest.mark.gpu

PICTURES = {"136x72": (136, 72, 21), "416x240": (416, 240, 21)}       # width, height, seed
BASE = dict(tree_rates=True, pu_modes=True, cu_close=True, cqt=True, unit_trees=True, commit=True)
QP = 32


@pytest.fixture(scope="module")
def hv():
    from turingcodec_amd.havoc import Havoc
    h = Havoc(stream="new")
    yield h
    h.close()


@pytest.fixture(scope="module", params=list(PICTURES))
def pictures(hv, request):
    """the picture with finish and the same picture with commit alone: three steps each, the third replayed from the graph"""
    from turingcodec_amd.decisions import DecisionPicture
    w, h, seed = PICTURES[request.param]
    out = {}
    for name, options in (("on", dict(BASE, finish=True)), ("off", BASE)):
        dp = DecisionPicture(hv, w, h, 8, QP, seed=seed, threads=8, intra=False, **options)
        for _ in range(3):
            searched = dp.step()
        assert all(dp._graphs.values()) and len(dp._graphs) == 1
        out[name] = (dp, searched)
    return out


@pytest.fixture(scope="module")
def host(pictures, reference_c):
    """the commit-only picture's planes and cells, and from them, by the reference alone: the strengths over unit lists, the deblocked planes, the padded planes"""
    on, off = pictures["on"][0], pictures["off"][0]
    W, H, pad, c2 = on.W, on.H, on.PAD, on.PAD // 2
    committed = off.cqt_commit_results()
    cqt = committed["cells"]
    data, bs = reference_c.derive_bs(W, H, *F.unit_lists(cqt, W, H, 3, QP, 0, 1))
    y, cb, cr = committed["recon"].copy(), committed["crecon"][0].copy(), committed["crecon"][1].copy()
    reference_c.deblock(y, W, cb, cr, W // 2, W, H, 8, data, bs)
    planes = []
    for p, (w, h, stride, border, size) in zip((y, cb, cr), ((W, H, on.stride, pad, on.n), (W // 2, H // 2, on.cstride, c2, on.cn), (W // 2, H // 2, on.cstride, c2, on.cn))):
        full = np.zeros(size, on.dt)
        full.reshape(-1, stride)[border:border + h, border:border + w] = p
        reference_c.pad_block(full, border * stride + border, w, h, stride, border, True, True, True, True)
        planes.append(full.reshape(-1, stride))
    return dict(cqt=cqt, committed=committed, data=data, bs=bs, deblocked=(y, cb, cr), planes=planes, got=on.cqt_finish_results())


def test_same_inputs_and_the_map_is_the_restatement(pictures, host):
    on = pictures["on"][0]
    cqt_on = on.hv.cqt_cells_download(on.cqt_cells, on.W, on.H, 3)
    assert cqt_on.tobytes() == host["cqt"].tobytes() and (host["cqt"]["unit"] >= 0).all()
    got = host["got"]["cells"]
    assert got.dtype == F.CELL_DT and got.shape == (on.H // 4, on.W // 4)
    assert got.tobytes() == F.block_cells(host["cqt"], on.W, on.H, 3, QP, 0, 1).tobytes()
    assert on.cqt_finish_results() is host["got"]


def test_strengths_are_the_reference_derivation_over_the_units(pictures, host):
    got = host["got"]
    assert np.array_equal(got["data"], host["data"]) and np.array_equal(got["bs"], host["bs"])
    assert (got["bs"] != 0).any()
    on = pictures["on"][0]
    edges = F.unit_edge_strengths(host["cqt"], on.W, on.H, 3, host["bs"])
    print("units", len(F.units_of(host["cqt"], 3)), "| unit-edge segments by strength 0 / 1 / 2:", np.bincount(edges, minlength=3), "| regions with a strength:",
          int((got["bs"] != 0).sum()), "of", got["bs"].size)


def test_planes_are_the_reference_deblocked_and_padded(pictures, host):
    """the whole padded planes, sample for sample: the committed planes through the reference's deblocking (luma with Cb and Cr, the strengths above) and its padBlock
    (96 / 48 samples); and not vacuously: the filter changed luma samples"""
    on = pictures["on"][0]
    got, want = host["got"], host["planes"]
    assert got["recon"].shape == want[0].shape and got["crecon"].shape == (2,) + want[1].shape
    assert np.array_equal(got["recon"], want[0])
    assert np.array_equal(got["crecon"][0], want[1]) and np.array_equal(got["crecon"][1], want[2])
    pad, c2 = on.PAD, on.PAD // 2
    luma = got["recon"][pad:pad + on.H, pad:pad + on.W]
    changed = [int((a != b).sum()) for a, b in zip((luma, got["crecon"][0][c2:c2 + on.H // 2, c2:c2 + on.W // 2], got["crecon"][1][c2:c2 + on.H // 2, c2:c2 + on.W // 2]),
                                                   (host["committed"]["recon"], host["committed"]["crecon"][0], host["committed"]["crecon"][1]))]
    print("samples the filter changed: luma", changed[0], "of", luma.size, "| Cb", changed[1], "| Cr", changed[2])
    assert changed[0] > 0
    # the padding is written: the corners replicate the picture's corner samples
    assert got["recon"][0, 0] == luma[0, 0] and got["recon"][pad + on.H + pad - 1, pad + on.W + pad - 1] == luma[-1, -1]


def test_the_step_is_otherwise_unchanged(pictures):
    """finish leaves recon, crecon, cells and every record of the options byte-identical to the commit-only picture; one graph"""
    (on, r_on), (off, r_off) = pictures["on"], pictures["off"]
    assert not hasattr(off, "cqt_block") and not hasattr(off, "cqt_data") and not hasattr(off, "cqt_bs")
    down = lambda dp, t: dp.hv.down(t, dp.dt)

    def chroma_area(dp):      # (the picture's part of each plane: crecon's lower padding holds the legacy plan's dump block, different from run to run)
        c2, c = dp.PAD // 2, down(dp, dp.crecon)
        return np.stack([c[k * dp.cpe:k * dp.cpe + dp.cn].reshape(-1, dp.cstride)[c2:c2 + dp.H // 2, c2:c2 + dp.W // 2] for k in (0, 1)])

    assert np.array_equal(down(on, on.recon), down(off, off.recon)) and down(on, on.recon).any()
    assert np.array_equal(chroma_area(on), chroma_area(off)) and chroma_area(on).any()
    assert np.array_equal(on.cells.view(np.uint8), off.cells.view(np.uint8))
    assert np.array_equal(on.hv.down(on.d_data, np.int8), off.hv.down(off.d_data, np.int8)) and np.array_equal(on.hv.down(on.d_bs, np.uint8), off.hv.down(off.d_bs, np.uint8))

    def same(a, b):
        assert set(a) == set(b)
        return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) if isinstance(a[k], np.ndarray) else a[k] == b[k]
                   for k in a)

    assert same(on.pu_decisions, off.pu_decisions) and same(on.unit_tree_decisions(), off.unit_tree_decisions())
    assert same(on.cu_decisions, off.cu_decisions) and same(on.cqt_decisions, off.cqt_decisions)
    assert np.array_equal(r_on[0], r_off[0]) and np.array_equal(r_on[1], r_off[1])
    assert len(on._graphs) == 1 and len(off._graphs) == 1 and all(on._graphs.values())


def test_refusals(hv, pictures):
    from turingcodec_amd.decisions import DecisionPicture
    on, off = pictures["on"][0], pictures["off"][0]
    without_commit = dict(BASE, commit=False)
    with pytest.raises(ValueError, match="finish"):
        DecisionPicture(hv, on.W, on.H, 8, QP, seed=21, threads=8, intra=False, finish=True, **without_commit)
    with pytest.raises(ValueError, match="finish"):
        DecisionPicture(hv, on.W, on.H, 8, QP, seed=21, threads=8, intra=False, finish=True)
    with pytest.raises(ValueError, match="commit"):      # wherever commit is refused
        DecisionPicture(hv, on.W, on.H, 8, QP, seed=21, threads=8, intra=False, finish=True, commit=True, tree_rates=True, pu_modes=True, cu_close=True, cqt=True)
    with pytest.raises(ValueError, match="cqt_finish_results"):
        on.cqt_commit_results()
    with pytest.raises(ValueError, match="finish"):
        off.cqt_finish_results()
    with pytest.raises(ValueError):
        on.step_banded(hv)
