"""Generates tests/golden/tree_rate_golden.npz: the trees of tests/tree_rate_tools.make_cases per unit size and depth (levels, job records, what their flags were derived
from, snapshots) and what the REFERENCE's own Syntax<transform_tree> gives for them under EstimateRate<void> (tests/tree_rate_shim.cpp: the rate and cbf mask of every
tree, the 128 + 4 context states it leaves, the residual_coding calls the syntax reaches).  Needs the reference sources (the shim compiles them):
python tests/golden/make_tree_rate_golden.py"""
import collections
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import reflibs                 # noqa: E402
import tree_rate_tools as TR   # noqa: E402

COUNT = 264      # trees per (unit size, depth): at least 257, so that a launch has a fifth, partly filled workgroup


def main():
    oracle, shim = reflibs.Oracle(), TR.Shim()
    out = {}
    for L, depth in TR.UNITS:
        luma, chroma, states, syntax, jobs, aux = TR.make_cases(oracle, 7000 + 10 * L + depth, L, depth, COUNT)
        rates, masks, after, after_syntax, calls = shim.walk_jobs(L, depth, luma, chroma, states, syntax, jobs, aux)
        tags = collections.Counter()
        TR.walk_jobs(L, depth, luma, chroma, states, syntax, jobs, tags)
        missing = [k for k in TR.required_tags(L, depth) if not tags[k]]
        assert not missing, (L, depth, missing)
        k = f"l{L}d{depth}"
        out[k + ".luma"], out[k + ".chroma"], out[k + ".states"], out[k + ".syntax"] = luma, chroma, states, syntax
        out[k + ".jobs"], out[k + ".aux"] = jobs.view(np.uint8).reshape(len(jobs), -1), aux.view(np.int32).reshape(len(jobs), -1)
        out[k + ".rates"], out[k + ".masks"], out[k + ".after"], out[k + ".after_syntax"] = rates, masks, after, after_syntax
        flat = np.full((len(jobs), 12, 5), -1, np.int16)
        for j, c in enumerate(calls):
            if c:
                flat[j, :len(c)] = c
        out[k + ".calls"] = flat
    path = os.path.join(HERE, "tree_rate_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
