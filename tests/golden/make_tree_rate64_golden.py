"""Generates tests/golden/tree_rate64_golden.npz: the 64x64 trees of tests/unit_tree_tools.make_cases64 (levels, job records, what their flags were derived from,
snapshots) and what the REFERENCE's own Syntax<transform_tree> gives for them under EstimateRate<void> (tests/tree_rate_shim.cpp with log2Cb 6, depth 1, MaxTrafoDepth 1,
MinTbLog2SizeY 2, MaxTbLog2SizeY 5: the rate and cbf mask of every tree, the 128 + 4 context states it leaves, the residual_coding calls the syntax reaches).  Needs the
reference sources (the shim compiles them):
python tests/golden/make_tree_rate64_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import reflibs                 # noqa: E402
import tree_rate_tools as TR   # noqa: E402
import unit_tree_tools as UT   # noqa: E402

COUNT = 200      # four workgroups, the last partly filled; a tree is 6144 levels (about 1.2 KB of the file each), and the file stays below the tree-rate golden


def main():
    oracle, shim = reflibs.Oracle(), TR.Shim()
    luma, chroma, states, syntax, jobs, aux = UT.make_cases64(oracle, 7061, COUNT)
    rates, masks, after, after_syntax, calls = shim.walk_jobs(UT.L64, UT.DEPTH64, luma, chroma, states, syntax, jobs, aux)
    tags = UT.reached(masks, jobs)
    missing = [k for k in UT.REQUIRED_CASES if not tags[k]]
    assert not missing, missing
    flat = np.full((len(jobs), 12, 5), -1, np.int16)
    for j, c in enumerate(calls):
        if c:
            flat[j, :len(c)] = c
    out = dict(luma=luma, chroma=chroma, states=states, syntax=syntax, jobs=jobs.view(np.uint8).reshape(len(jobs), -1), aux=aux.view(np.int32).reshape(len(jobs), -1),
               rates=rates, masks=masks, after=after, after_syntax=after_syntax, calls=flat)
    path = os.path.join(HERE, "tree_rate64_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes;", dict(tags))


if __name__ == "__main__":
    main()
