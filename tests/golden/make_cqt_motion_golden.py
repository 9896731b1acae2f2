"""Generates tests/golden/cqt_motion_golden.npz: per entry of cqt_motion_tools.STORE_CASES what the REFERENCE's own collocated motion store holds after one
fillRectangle per committed coding unit (tests/cqt_motion_shim.cpp: a real StateCollocatedMotion; units in a random order): int32 [rows, cols, 8] = predFlag0,
predFlag1, mv0 x, y, mv1 x, y, dpb index 0, 1 with the dpb indices cqt_motion_tools.GOLDEN_DPB.  Data only.  Before anything is written the restatement is held
against those entries and the cases are asserted to reach every tag of cqt_motion_tools.STORE_TAGS.  Needs the reference sources (the shim compiles them):
python tests/golden/make_cqt_motion_golden.py"""
import collections
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import cqt_motion_tools as M   # noqa: E402


def main():
    shim = M.Shim()
    out, tags = {}, collections.Counter()
    for i, name in enumerate(M.STORE_CASES):
        case = M.make_store_case(name)
        entries = shim.entries(case, *M.GOLDEN_DPB, rng=np.random.default_rng(i))
        want = M.shim_view(M.restate_store(case, tags), case["ref_poc0"], case["ref_poc1"], *M.GOLDEN_DPB)
        assert np.array_equal(entries, want), name
        out[name] = entries
    missing = [k for k in M.STORE_TAGS if not tags[k]]
    assert not missing, missing
    path = M.golden_path()
    np.savez_compressed(path, **out)
    print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
