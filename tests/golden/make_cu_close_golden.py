"""Generates tests/golden/cu_close_golden.npz: the inputs of one launch of havoc_mi355x_cu_close per entry of cu_close_tools.SLICES (tests/cu_close_tools.make_cases: job
records, snapshots, tree decisions, rates, SSDs) and what the REFERENCE gives for them (tests/cu_close_shim.cpp: its own Syntax<coding_unit> under Measure<void> and the
close's two costs with its Cost and Lambda types: outcome, rate, lambdaDistortion, both costs and both snapshots of every job the contract does not refuse; a refused job:
-1 and its input snapshots), and closeInterCu's arithmetic for a table of (rates, SSDs, reciprocalLambda).  The seeds are chosen so that the reference's results alone
show every outcome -- coded wins, no residual wins, equal costs keep the residual, skipped -- in every launch; that is asserted here and again in tests/test_cu_close.py.
Needs the reference sources (the shim compiles them): python tests/golden/make_cu_close_golden.py"""
import collections
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import cu_close_tools as CC   # noqa: E402

CASE_KEYS = ("cu_syntax", "pu_before", "pu_after", "pu_rate", "choice", "tree_choice", "tree_rate", "pred_ssd", "jobs")
SEED = 9100


def outcomes_shown(out):
    """which of the four placements the results show"""
    both = out["have_residual"] == 1
    return {"coded wins": bool(((out["outcome"] == CC.CODED) & (out["cost_coded"] < out["cost_no_residual"])).any()),
            "no residual wins": bool((both & (out["outcome"] == CC.NO_RESIDUAL)).any()),
            "equal cost keeps the residual": bool(((out["outcome"] == CC.CODED) & (out["cost_coded"] == out["cost_no_residual"])).any()),
            "skipped": bool((out["outcome"] == CC.SKIPPED).any()), "skip wins": bool((both & (out["outcome"] == CC.SKIPPED)).any())}


def cost_table(seed, n):
    """(haveResidual, merged, rateCoded, rateWithout, ssd[3], ssdPrediction[3]) int64 [n, 10] and reciprocalLambda float64 [n]"""
    rng = np.random.default_rng(seed)
    rows = np.concatenate([rng.integers(0, 2, (n, 2)), rng.integers(0, 900 << 16, (n, 2)), rng.integers(0, 1 << 22, (n, 6))], axis=1).astype(np.int64)
    rows[::7, 4:7] = 0x30000000         # the sum of the three wraps in int32
    lam = np.exp(rng.uniform(np.log(0.001), np.log(0.5), n))
    return rows, lam


def main():
    shim = CC.Shim()
    out = {}
    for i, sl in enumerate(CC.SLICES):
        case = CC.make_cases(SEED + i, sl)
        res, cu, pu, _ = CC.walk_jobs(case, sl, closer=shim.close)
        shown = outcomes_shown(res)
        assert all(shown.values()), (sl, shown)
        tags = collections.Counter()
        CC.walk_jobs(case, sl, tags)
        missing = [k for k in CC.required_tags(sl) if not tags[k]]
        assert not missing, (sl, missing)
        k = f"s{i}"
        out[k + ".slice"] = np.array(sl, np.float64)
        for name in CASE_KEYS:
            a = case[name]
            out[f"{k}.{name}"] = a.view(np.uint8).reshape(len(a), -1) if a.dtype.names else a
        out[k + ".out"], out[k + ".cu_after"], out[k + ".pu_after_out"] = res.view(np.uint8).reshape(len(res), -1), cu, pu
    rows, lam = cost_table(SEED + 100, 400)
    got = []
    for r, d in zip(rows, lam):
        dc, cc, dn, cn, drop, q = shim.costs(r[2], r[4:7], r[3], r[7:10], d)
        got.append([dc, cc, dn, cn, drop, q])
    out["cost.rows"], out["cost.lambda"], out["cost.ref"] = rows, lam, np.array(got, np.int64)
    path = os.path.join(HERE, "cu_close_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes,", sum(len(out[f"s{i}.jobs"]) for i in range(len(CC.SLICES))), "jobs")


if __name__ == "__main__":
    main()
