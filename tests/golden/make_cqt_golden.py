"""Generates tests/golden/cqt_golden.npz: per entry of cqt_tools.CASES the inputs of one call of havoc_mi355x_cqt_decide (tests/cqt_tools.make_case: the node table
and what the quadtree reads of the candidates' records) and the recorded results: the decision as tests/cqt_tools.decide_picture restates it -- CTU records, node
records, the CtDepth map, the contexts after every CTU -- and what the REFERENCE gives for the decided trees (tests/cqt_shim.cpp: its own Syntax<coding_quadtree>::go
and split_cu_flag writer over a real snake): the rate and the three context states of every CTU.  Before anything is written every flag the restatement priced is held
against the reference's writer, the decided trees' rates and states against the reference's pass, and the cases are asserted to reach every branch of
cqt_tools.required_tags between them.  Needs the reference sources (the shim compiles them): python tests/golden/make_cqt_golden.py"""
import collections
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import cqt_tools as Q   # noqa: E402


def main():
    shim = Q.Shim()
    out, tags, flags = {}, collections.Counter(), 0
    for name, args in Q.CASES.items():
        case = Q.make_case(**args)
        trace = []
        res = Q.decide_picture(case, tags, trace)
        for t in trace:
            bits, after, inc, left, up = shim.flag(case, t)
            assert (bits, after, inc, left, up) == (t["bits"], t["after"], t["inc"], t["left"], t["up"]), (name, t)
        flags += len(trace)
        rate, states = shim.picture(case, res)
        assert np.array_equal(rate, res["ctus"]["rate"]) and np.array_equal(states, res["cu_syntax"][:, :3]), name
        for k, a in Q.pack(case, res).items():
            out[f"{name}.{k}"] = a
        out[name + ".ref_rate"], out[name + ".ref_states"] = rate, states
    missing = [k for k in Q.required_tags() if not tags[k]]
    assert not missing, missing
    path = Q.golden_path()
    np.savez_compressed(path, **out)
    print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes,", flags, "flags held against the reference's writer")


if __name__ == "__main__":
    main()
