"""Generates tests/golden/pu_rate_golden.npz: the candidates of tests/pu_rate_tools.make_cases per slice of pu_rate_tools.SLICES (job records, snapshots) and what the
REFERENCE's own Syntax<prediction_unit> gives for them under Measure<void> (tests/pu_rate_shim.cpp: the rate of every candidate the contract does not refuse and the
16 context states it leaves; a refused candidate: -1 and its input snapshot), and measurePuCost's sum with the reference's Cost and Lambda types for a table of
(rate, SATDs, reciprocalSqrtLambda).  Needs the reference sources (the shim compiles them): python tests/golden/make_pu_rate_golden.py"""
import collections
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import pu_rate_tools as PR   # noqa: E402


def cost_table(seed, n):
    """(rate, satdY, satdCb, satdCr) int64 [n, 4] and reciprocalSqrtLambda float64 [n]"""
    rng = np.random.default_rng(seed)
    rows = np.concatenate([rng.integers(0, 80 << 16, (n, 1)), rng.integers(0, 1 << 22, (n, 3))], axis=1).astype(np.int64)
    lam = np.exp(rng.uniform(np.log(0.005), np.log(8.0), n))
    return rows, lam


def main():
    shim = PR.Shim()
    out = {}
    for i, sl in enumerate(PR.SLICES):
        states, jobs = PR.make_cases(8100 + i, sl)
        rates, after = shim.walk_jobs(jobs, sl, states)
        tags = collections.Counter()
        PR.walk_jobs(jobs, sl, states, tags)
        missing = [k for k in PR.required_tags(sl) if not tags[k]]
        assert not missing, (sl, missing)
        k = f"s{i}"
        out[k + ".slice"], out[k + ".states"], out[k + ".jobs"] = np.array(sl, np.int32), states, jobs.view(np.uint8).reshape(len(jobs), -1)
        out[k + ".rates"], out[k + ".after"] = rates, after
    rows, lam = cost_table(8200, 400)
    got = np.array([shim.cost(r[0], r[1:], d) for r, d in zip(rows, lam)], np.int64)
    out["cost.rows"], out["cost.lambda"], out["cost.cost"], out["cost.lambda_q16"] = rows, lam, got[:, 0], got[:, 1].astype(np.int32)
    path = os.path.join(HERE, "pu_rate_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes,", sum(len(out[f"s{i}.jobs"]) for i in range(len(PR.SLICES))), "jobs")


if __name__ == "__main__":
    main()
