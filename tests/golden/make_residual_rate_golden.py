"""Generates tests/golden/residual_rate_golden.npz: the blocks of tests/residual_rate_tools.make_cases (levels, job fields, snapshots) and what the REFERENCE's
own CodedData::storeResidual + EncodeResidual::inner<EstimateRate> give for them (tests/residual_rate_shim.cpp: the rate of every block, the 128 context states after
every job).  Needs the reference sources (the shim compiles them):  python tests/golden/make_residual_rate_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import reflibs                     # noqa: E402
import residual_rate_tools as R    # noqa: E402

CASES = {2: 560, 3: 560, 4: 560, 5: 590}      # RDOQ blocks per transform size: with the hand-made ones, at least 257 jobs each


def main():
    oracle, shim = reflibs.Oracle(), R.Shim()
    out = {}
    for log2, count in CASES.items():
        levels, states, jobs = R.make_cases(oracle, 4000 + log2, log2, count)
        assert len(jobs) >= 257, (log2, len(jobs))
        rates, after = shim.walk_jobs(log2, levels, states, jobs)
        k = f"l{log2}"
        out[k + ".levels"], out[k + ".states"], out[k + ".jobs"] = levels, states, jobs.view(np.uint8).reshape(len(jobs), -1)
        out[k + ".rates"], out[k + ".after"] = rates, after
    path = os.path.join(HERE, "residual_rate_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
