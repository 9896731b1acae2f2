"""The temporal candidate in the picture search's predictor derivation: picture_order.hpp's derivePredictors / walkPictureSequential with a table of
havoc_mi355x_temporal_cand records (the host form), and havoc_mi355x_search_temporal + havoc_mi355x_search_picture_uni (k_search_rows / k_search_step with a table; -m gpu).

Pictures: 136 x 72 (3 x 2 CTUs) and 416 x 240 (7 x 4 CTUs), both cut by the right and the bottom edge; the units of workload.picture_pus as DecisionPicture(seed=5) has
them.  The candidate table is synthetic (search_temporal_tools.make_table, seed 3): about three quarters available, vectors within +-40 quarter samples, and on units
at all four picture edges components at +-32767, -32768 and one full sample beyond the unit's LimitFullPelMv bounds.

What that table does to the walk over the CPU oracle (8-bit), recorded from a run of these tests:
    136 x 72:   the candidate changed the predictor pair in 26 of 54 derivations; 21 result records differ from the walk without a table, final vectors 7 (list 0) and
                8 (list 1), 22 refinement records; slot taken: first 2, second 27, not consulted (two different spatial predictors) 25
    416 x 240:  131 of 478 derivations; 141 result records, final vectors 29 and 38, 129 refinement records; first 2, second 165, not consulted 311
"""
import functools

import numpy as np
import pytest

import search_temporal_tools as T
import search_tools as st

EINVAL = -10001
CASES = [(name, bd) for name in T.PICTURES for bd in (8, 10)]


@functools.lru_cache(maxsize=None)
def table(name):
    return T.make_table(T.make_case(name, 8))      # (the units do not depend on the bit depth)


@functools.lru_cache(maxsize=None)
def walk(kind, name, bd, which):
    """the walk once per (back end, picture, table): shared by the tests, never changed"""
    case = T.make_case(name, bd)
    cands = {"none": None, "unavailable": T.unavailable_table(case), "table": table(name)[0]}[which]
    return T.Client(kind).walk(case, cands, report=True)


def _bytes_equal(a, b):
    return all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(a, b))


# ---- CPU -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(T.PICTURES))
def test_walk_without_candidates_is_the_existing_walk(name):
    """a nullptr table and a table of unavailable candidates: results, field and refinements of search_client.cpp's picture_uni, byte for byte"""
    case = T.make_case(name, 8)
    want = st.Client("oracle").picture_uni(case["params"], *case["planes"], case["stride"], T.PAD, case["pus"], case["ctu_first"], case["cx"], case["cy"], case["mvp_rate"],
                                           bi=True)
    assert want[0]["calls"].all() and want[2]["calls"].any()
    for which in ("none", "unavailable"):
        got = walk("oracle", name, 8, which)
        assert _bytes_equal(got[:3], want), which
        assert np.array_equal(got[3][..., 2:6], got[3][..., 6:10]), which      # an unavailable candidate changes no derivation


@pytest.mark.parametrize("name", list(T.PICTURES))
def test_the_rule_per_derivation(name):
    """every derivation of the temporal walk, from the field as the walk had it: the candidate is used exactly when it is available and the list has fewer than two
    different spatial predictors; it takes the first free slot; every other slot is what it was"""
    cands, _ = table(name)
    rep = walk("oracle", name, 8, "table")[3]
    free, without, with_ = rep[..., 0], rep[..., 2:6].reshape(rep.shape[:2] + (2, 2)), rep[..., 6:10].reshape(rep.shape[:2] + (2, 2))
    assert set(np.unique(free)) == {-1, 0, 1}                                    # all three cases occur: first slot, second slot, not consulted
    # (what "free" means, from the derivation without a candidate: the list is zero-filled behind its spatial predictors)
    assert not without[free == 0].any() and not without[free == 1][:, 1].any()
    want = without.copy()
    used = (cands["available"] != 0) & (free >= 0)
    for p, l in zip(*np.nonzero(used)):
        want[p, l, free[p, l]] = cands["mv"][p, l]
    assert np.array_equal(with_, want)
    assert np.array_equal(with_[~used], without[~used])
    changed = (with_ != without).any(axis=(-1, -2))
    print(name, "derivations changed", int(changed.sum()), "of", changed.size, "slots", {int(s): int((free == s).sum()) for s in (-1, 0, 1)})
    assert changed.sum() >= 0.10 * changed.size


@pytest.mark.parametrize("name", list(T.PICTURES))
def test_the_table_changes_the_walk(name):
    """the tests below compare something: final vectors of both lists and refinements differ from the walk without a table, the int16 extremes among them"""
    cands, extreme = table(name)
    res, field, bi, rep = walk("oracle", name, 8, "table")
    res0, field0, bi0, _ = walk("oracle", name, 8, "none")
    differ = (res["mv"] != res0["mv"]).any(-1)
    records = sum(a.tobytes() != b.tobytes() for a, b in zip(res, res0))
    refinements = sum(a.tobytes() != b.tobytes() for a, b in zip(bi, bi0))
    print(name, "result records", records, "final vectors", int(differ[0::2].sum()), int(differ[1::2].sum()), "refinement records", refinements)
    assert differ[0::2].any() and differ[1::2].any() and refinements > 0 and not np.array_equal(field, field0)
    # the extreme records are consumed (their units lie at the edges, early in their CTUs) and the vectors they lead to stay inside the search limits
    took = (rep[extreme][..., 2:6] != rep[extreme][..., 6:10]).any(-1)
    assert took.sum() >= len(extreme) // 2 and np.abs(cands["mv"][extreme].astype(np.int32)).max() == 32768
    pus, W, H = T.make_case(name, 8)["pus"], *T.PICTURES[name]
    full = res["mv_integer"].reshape(-1, 2, 2) // 4
    assert (full[..., 0] >= -64 - pus["x0"][:, None]).all() and (full[..., 0] <= W + 64 - (pus["x0"] + pus["w"])[:, None]).all()
    assert (full[..., 1] >= -64 - pus["y0"][:, None]).all() and (full[..., 1] <= H + 64 - (pus["y0"] + pus["h"])[:, None]).all()


@pytest.mark.parametrize("name,bd", CASES)
def test_temporal_walk_over_oracle_equals_walk_over_reference_tables(name, bd):
    if not T.have_ref():
        pytest.skip("oracle/_ref not built")
    assert _bytes_equal(walk("oracle", name, bd, "table"), walk("ref", name, bd, "table"))


def test_decision_picture_refuses_temporal_mvp_without_col():
    from turingcodec_amd.decisions import DecisionPicture
    with pytest.raises(ValueError, match="temporal_mvp"):
        DecisionPicture(None, 136, 72, 8, 32, temporal_mvp=True)
    with pytest.raises(ValueError, match="col"):      # col's own refusal comes first where both apply
        DecisionPicture(None, 136, 72, 8, 32, temporal_mvp=True, col=dict(), search_on_device=False)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hv():
    from turingcodec_amd.havoc import Havoc
    h = Havoc(stream="new")
    yield h
    h.close()


@pytest.fixture(scope="module")
def device_pictures(hv):
    made = {}

    def get(name, bd):
        if (name, bd) not in made:
            made[name, bd] = T.DevicePicture(hv, T.make_case(name, bd))
        return made[name, bd]
    return get


def _searched(pic, step_launches, bi):
    rc, res, field, refinements, gave_up = pic.search(step_launches, bi)
    assert rc == 0 and gave_up == 0
    return res, field, refinements


@pytest.mark.gpu
@pytest.mark.parametrize("name,bd", CASES)
def test_device_search_with_the_table_equals_the_temporal_walk(hv, device_pictures, name, bd):
    """results and motion field for both launch forms, refinements with d_out_bi: whole sentinel-filled destinations against the walk over the CPU oracle (and over the
    reference's tables where they travelled); the table is not written"""
    pic = device_pictures(name, bd)
    cands = table(name)[0]
    d_table = hv.up(cands.view(np.uint8).reshape(-1))
    wants = [walk("oracle", name, bd, "table")] + ([walk("ref", name, bd, "table")] if T.have_ref() else [])
    hv.search_temporal_d(d_table, pic.n)
    try:
        got = {(s, b): _searched(pic, s, b) for s, b in ((0, False), (1, False), (0, True), (1, True))}
    finally:
        hv.search_temporal_d(None, 0)
    assert hv.down(d_table, np.uint8).tobytes() == cands.tobytes()
    for want in wants:
        for (s, b), (res, field, refinements) in got.items():
            wrong = [i for i in range(len(res)) if res[i].tobytes() != want[0][i].tobytes()]
            assert not wrong, (s, b, len(wrong), wrong[:4], res[wrong[0]], want[0][wrong[0]])
            assert field.tobytes() == want[1].tobytes(), (s, b)
            if b:
                wrong = [i for i in range(len(refinements)) if refinements[i].tobytes() != want[2][i].tobytes()]
                assert not wrong, (s, b, len(wrong), wrong[:4], refinements[wrong[0]], want[2][wrong[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("name,bd", CASES)
def test_device_search_without_candidates_is_the_search_without_a_table(hv, device_pictures, name, bd):
    """an all-unavailable table, and no table again after search_temporal(NULL): byte for byte the search that never saw a table"""
    pic = device_pictures(name, bd)
    before = {s: _searched(pic, s, True) for s in (0, 1)}
    d_table = hv.up(T.unavailable_table(pic.case).view(np.uint8).reshape(-1))
    hv.search_temporal_d(d_table, pic.n)
    try:
        unavailable = {s: _searched(pic, s, True) for s in (0, 1)}
    finally:
        hv.search_temporal_d(None, 0)
    after = {s: _searched(pic, s, True) for s in (0, 1)}
    want = walk("oracle", name, bd, "none")
    for s in (0, 1):
        assert _bytes_equal(before[s], want[:3]), s
        assert _bytes_equal(unavailable[s], before[s]), s
        assert _bytes_equal(after[s], before[s]), s


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(hv, device_pictures):
    pic = device_pictures("136x72", 8)
    cands = table("136x72")[0]
    d_table = hv.up(np.concatenate([cands.view(np.uint8).reshape(-1), np.zeros(8, np.uint8)]))
    f = hv.L.havoc_mi355x_search_temporal
    assert f(hv.h, d_table.data_ptr(), 0) == EINVAL and f(hv.h, d_table.data_ptr(), -3) == EINVAL
    assert b"n_pus" in hv.L.havoc_mi355x_last_error()
    assert f(hv.h, d_table.data_ptr() + 4, pic.n) == EINVAL
    assert b"aligned" in hv.L.havoc_mi355x_last_error()
    # none of them set a table: the search is the one without
    want = walk("oracle", "136x72", 8, "none")
    assert _bytes_equal(_searched(pic, 0, True), want[:3])
    # a table for another number of units than the search's
    assert f(hv.h, d_table.data_ptr(), pic.n + 1) == 0
    try:
        assert pic.search(0, True)[0] == EINVAL and pic.search(1, False)[0] == EINVAL
        assert b"temporal" in hv.L.havoc_mi355x_last_error()
        assert f(hv.h, d_table.data_ptr(), pic.n) == 0
        assert _bytes_equal(_searched(pic, 0, True), walk("oracle", "136x72", 8, "table")[:3])
    finally:
        assert f(hv.h, None, 0) == 0
    assert f(hv.h, None, -1) == 0      # NULL removes the table whatever the count
    assert _bytes_equal(_searched(pic, 0, True), want[:3])
