"""Generates tests/golden/intra_rate_golden.npz: the candidates of tests/intra_rate_tools.make_cases (levels, job records, what they were derived from, snapshots) and
what the REFERENCE's own Syntax<IntraPartition> gives for them under EstimateRateLuma (tests/intra_rate_shim.cpp: the rate of every candidate, the 128 + 4 context
states it leaves).  Needs the reference sources (the shim compiles them):  python tests/golden/make_intra_rate_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import reflibs                  # noqa: E402
import intra_rate_tools as I    # noqa: E402

CASES = {2: 245, 3: 245, 4: 245, 5: 245}      # RDOQ blocks per transform size: with the hand-made ones, at least 257 candidates each


def main():
    oracle, shim = reflibs.Oracle(), I.Shim()
    out = {}
    for log2, count in CASES.items():
        levels, states, syntax, jobs, aux = I.make_cases(oracle, 5000 + log2, log2, count)
        assert len(jobs) >= 257, (log2, len(jobs))
        rates, after, after_syntax, info = shim.walk_jobs(log2, levels, states, syntax, jobs, aux)
        assert np.array_equal(info[:, 0], jobs["mpm_idx"])
        k = f"l{log2}"
        out[k + ".levels"], out[k + ".states"], out[k + ".syntax"] = levels, states, syntax
        out[k + ".jobs"], out[k + ".aux"] = jobs.view(np.uint8).reshape(len(jobs), -1), aux.view(np.int32).reshape(len(jobs), -1)
        out[k + ".rates"], out[k + ".after"], out[k + ".after_syntax"] = rates, after, after_syntax
    path = os.path.join(HERE, "intra_rate_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
