"""DecisionPicture's launch plan, recorded WITHOUT a device (tests/test_decision_launch_plan.py): a stand-in for the Havoc context that builds every buffer in
host memory and, instead of launching, notes each `*_d` call with its arguments -- so that a change of DecisionPicture's structure can be held, launch for launch,
against the record of the code before it (tests/golden/decision_launch_plan.json).

What a record keeps of an argument: a tensor as (allocation, byte offset, shape, dtype, sha1 of its bytes when the call is made), allocations numbered in the order
the record first meets them (the order they were CREATED in does not show); a uint64 numpy table as device addresses, each resolved to (allocation, byte offset) or
None; any other numpy array as shape, dtype, sha1; a ctypes structure or array as its bytes; lists and tuples element by element.

    python tests/launch_plan_tools.py --write      regenerates the golden file from the code as it stands
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "decision_launch_plan.json")
FULL = dict(tree_rates=True, pu_modes=True, cu_close=True, cqt=True, unit_trees=True, commit=True, finish=True, motion=(8, 4, 16), merge_lists=5)


def library_built():
    from turingcodec_amd import havoc
    return os.path.exists(havoc.LIB_PATH)


def make_recorder():
    """a Havoc whose buffers live in host memory and whose `*_d` methods append (name, args, kwargs) to `.calls`.  up / zeros / field_layout / the workspaces /
    cqt_buffers are Havoc's own; nothing here touches a device"""
    import torch
    from turingcodec_amd import havoc

    class Recorder(havoc.Havoc):
        def __init__(self):
            self.torch, self.h, self.calls = torch, None, []
            self.L, _ = havoc._load()
            self.device, self.tstream = torch.device("cpu"), None

        def sync(self):
            pass

    def recording(name):
        def call(self, *args, **kwargs):
            self.calls.append((name, _frozen(args), {k: _frozen(v) for k, v in kwargs.items()}))
        return call

    for name in dir(havoc.Havoc):
        if name.endswith("_d") and callable(getattr(havoc.Havoc, name)):
            setattr(Recorder, name, recording(name))
    return Recorder()


def _sha(b):
    return hashlib.sha1(b).hexdigest()


class _Tensor:
    """a tensor argument as it was when the call was made; the tensor itself is kept so that its allocation can neither move nor be handed out again"""

    def __init__(self, t):
        self.t, store = t, t.untyped_storage()
        self.base, self.nbytes = store.data_ptr(), store.nbytes()
        self.offset = t.storage_offset() * t.element_size()
        self.shape, self.dtype = tuple(t.shape), str(t.dtype)
        self.sha = _sha(t.numpy().tobytes())


def _frozen(a):
    """the argument with everything a later call could change copied out of it"""
    import torch
    if isinstance(a, torch.Tensor):
        return _Tensor(a)
    if isinstance(a, np.ndarray):
        return a.copy()
    if isinstance(a, (C.Structure, C.Array)):
        return bytes(a)
    if isinstance(a, (list, tuple)):
        return tuple(_frozen(v) for v in a)
    if isinstance(a, (np.integer, np.bool_)):
        return int(a)
    if isinstance(a, np.floating):
        return float(a)
    assert a is None or isinstance(a, (bool, int, float, str)), type(a)
    return a


def _tensors(a):
    if isinstance(a, _Tensor):
        yield a
    elif isinstance(a, tuple):
        for v in a:
            yield from _tensors(v)


def canonical(calls):
    """the calls of one record with allocations numbered in order of first appearance and addresses resolved: a list of (name, printable arguments)"""
    spans = {}
    for _, args, kwargs in calls:
        for t in _tensors(tuple(args) + tuple(kwargs.values())):
            if t.nbytes:
                spans[t.base] = max(spans.get(t.base, 0), t.nbytes)
    bases = sorted(spans)
    number = {}

    def allocation(base):
        return number.setdefault(base, len(number))

    def address(v):
        v = int(v)
        if v == 0:
            return None
        k = int(np.searchsorted(bases, v, side="right")) - 1
        if k < 0 or v >= bases[k] + spans[bases[k]]:
            raise AssertionError(f"an address table names {v:#x}, which no launch of the record takes as a tensor")
        return allocation(bases[k]), v - bases[k]

    def show(a):
        if isinstance(a, _Tensor):
            return ("tensor", allocation(a.base) if a.nbytes else None, a.offset, a.shape, a.dtype, a.sha)
        if isinstance(a, np.ndarray):
            if a.dtype == np.uint64:
                return ("addresses", a.shape, tuple(address(v) for v in a.ravel()))
            return ("array", a.shape, str(a.dtype), _sha(np.ascontiguousarray(a).tobytes()))
        if isinstance(a, bytes):
            return ("bytes", a.hex())
        if isinstance(a, tuple):
            return tuple(show(v) for v in a)
        return a

    return [(name, repr((show(args), sorted((k, show(v)) for k, v in kwargs.items())))) for name, args, kwargs in calls]


def digest(calls):
    """dict(names, digests): one entry per launch"""
    rows = canonical(calls)
    return dict(names=[n for n, _ in rows], digests=[_sha((n + r).encode())[:16] for n, r in rows])


# ---- driving a picture through its stage methods in step()'s order ----------------------------------------------------------------------------------------------
def seeded_results(dp, seed):
    """search records (RESULT_DT [2 * units]) with vectors within +-20 quarter samples: they stay inside the padded planes at every unit"""
    from turingcodec_amd.decisions import RESULT_DT
    rng = np.random.default_rng(seed)
    res = np.zeros(2 * len(dp.pus), RESULT_DT)
    res["mv"] = rng.integers(-20, 21, res["mv"].shape)
    res["mvd"] = rng.integers(-9, 10, res["mvd"].shape)
    res["mvp_flag"] = rng.integers(0, 2, len(res))
    return res


def drive(dp):
    """what step() issues after its searches on the device route, stage method by stage method"""
    if dp.pu_modes:
        res = seeded_results(dp, 5)
        dp.bi_results = res
        dp.pu_candidates(res)
    dp.merge_candidates(None)
    dp.predict(None)
    if dp.sao:
        dp.sao_filter_inputs(None)
        dp.sao_loop_filter()
    elif dp.tree_rates:
        dp.tree_and_filter_on_device()
    else:
        dp.tree_and_filter_on_device()
        dp.chroma_chain(None)
    for on, stage in ((dp.pu_modes, dp.pu_mode_launches), (dp.unit_trees, dp.unit_tree_launches), (dp.cu_close, dp.cu_close_launches), (dp.cqt, dp.cqt_launch),
                      (dp.commit, dp.cqt_commit_launch), (dp.motion is not None, dp.cqt_motion_launch), (dp.finish, dp.cqt_finish_launch),
                      (dp.col is not None and not dp.temporal_mvp, dp.temporal_launch), (dp.merge_lists is not None, dp.cqt_merge_launch)):
        if on:
            stage()
    # (what step() reports of the plan: not a launch, kept beside them)
    dp.hv.calls.append(("plan_launches_d", (int(dp.rqt_plan["launches"]), int(dp.unit_plan["launches"]) if dp.unit_trees else None), {}))


def drive_host_route(dp):
    """search_on_device=False: the launches of step()'s host route around its two library calls, with the fixed-size chain on a seeded field"""
    from turingcodec_amd.havoc import CELL_DT
    rng = np.random.default_rng(9)
    field = rng.integers(-20, 21, (2, (dp.H + 3) // 4, (dp.W + 3) // 4, 2)).astype(np.int16)
    dp.merge_candidates(field)
    dp.predict(field)
    dp.tu_chain_fixed(field)
    dp.chroma_chain(field)
    dp.loop_filter(np.zeros((dp.H // 4, dp.W // 4), CELL_DT))


def drive_bands(dp, side):
    """the band views of step_banded (one CTU row each), every view through the stage methods a band issues"""
    for v in dp._band_views(1, side):
        v.merge_candidates(None)
        v.predict(None)
        v.tree_decisions()
        v.chroma_chain(None)


def _col(width, height):
    import torch
    from turingcodec_amd.havoc import COL_CELL_DT
    store = torch.zeros(((height + 15) // 16) * ((width + 15) // 16) * COL_CELL_DT.itemsize, dtype=torch.uint8)
    return dict(store=store, col_poc=16, cur_poc=8, target_poc=(4, 16), all_backwards=0, collocated_from_l0=1)


CONFIGS = {
    "default_56x56_8bit": (56, 56, 8, {}),
    "default_136x72_10bit": (136, 72, 10, {}),
    "residual_rates_56x56": (56, 56, 8, dict(residual_rates=True)),
    "tree_rates_56x56": (56, 56, 8, dict(tree_rates=True)),
    "sao_136x72": (136, 72, 8, dict(sao=True)),
    "full_136x72": (136, 72, 8, FULL),
    "full_col_136x72": (136, 72, 8, dict(FULL, col=True)),
    "host_route_136x72": (136, 72, 8, dict(search_on_device=False)),
    "bands_72x136": (72, 136, 8, {}),
}


def record(name):
    """the digest of configuration `name`"""
    from turingcodec_amd.decisions import DecisionPicture
    width, height, bit_depth, options = CONFIGS[name]
    options = dict(options)
    if options.get("col"):
        options["col"] = _col(width, height)
    rec = make_recorder()
    dp = DecisionPicture(rec, width, height, bit_depth, 32, seed=21, intra=False, **options)
    if name.startswith("bands"):
        side = make_recorder()
        drive_bands(dp, side)
        assert not rec.calls
        return digest(side.calls)
    if name.startswith("host_route"):
        drive_host_route(dp)
    else:
        drive(dp)
    return digest(rec.calls)


def first_difference(got, want):
    """None, or a sentence naming the first launch at which two digests part"""
    for i, (gn, gd, wn, wd) in enumerate(zip(got["names"], got["digests"], want["names"], want["digests"])):
        if gn != wn:
            return f"launch {i} is {gn}, the golden record has {wn}"
        if gd != wd:
            return f"launch {i} ({gn}) differs from the golden record in its arguments"
    if len(got["names"]) != len(want["names"]):
        return f"{len(got['names'])} launches, the golden record has {len(want['names'])}"
    return None


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    out = {name: record(name) for name in CONFIGS}
    if "--write" in sys.argv:
        with open(GOLDEN, "w") as f:
            json.dump(out, f, indent=0, sort_keys=True)
            f.write("\n")
    print({name: len(d["names"]) for name, d in out.items()})
