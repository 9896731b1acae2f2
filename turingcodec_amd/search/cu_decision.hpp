// cu_decision.hpp -- closing one inter coding unit, restated data-only beside decidePu (pu_decision.hpp).  Reference: turing/Search.hpp
//   :2362-2568  Search<IfCbf<rqt_root_cbf, transform_tree>>::go:
//   :2384-2397  lambdaDistortion += ssd * reciprocalLambda with ssd = ssd[0] + ssd[1] + ssd[2] as reconstructInter returns it (turing/Reconstruct.cpp:1427): the
//               UNWEIGHTED int32 sum, not the ssdY + 4 ssdCb + 4 ssdCr of the depth decision;
//   :2415-2441  haveResidual = rqt_root_cbf; a merged 2Nx2N unit without residual becomes a skipped CU: contexts and rate as before the CU, merge_idx, cu_skip_flag(1);
//   :2443-2456  else the preamble, rqt_root_cbf unless merged 2Nx2N, the tree when there is a residual;
//   :2462-2531  with a residual the unit is priced without it as well (skip syntax when merged, else the state after the preamble + rqt_root_cbf(0)) at
//               lambda * ssdPrediction[0] + lambda * ssdPrediction[1] + lambda * ssdPrediction[2]; it wins on cost2() < cost2().
// The RATES are the caller's: the whole coded candidate, the unit without residual (for a unit whose tree has no residual, its only candidate).
// havoc_mi355x_cu_close measures them on the device, bit for bit; this is the host form of its decision.
#pragma once

#include "decision.hpp"

namespace havoc_search {

enum CuOutcome { kCuCoded = 0, kCuNoResidual = 1, kCuSkipped = 2 };

struct CuCandidate
{
    bool haveResidual;      // the chosen tree's cbf mask != 0
    bool merged2Nx2N;
    Cost rateCoded;         // read with haveResidual: PU + preamble + rqt_root_cbf(1) unless merged + tree
    Cost rateNoResidual;    // skipped: merge_idx + cu_skip_flag(1); else PU + preamble + rqt_root_cbf(0)
    int32_t ssd[3];         // the reconstruction's, Y, Cb, Cr
    int32_t ssdPrediction[3];
};

struct CuDecision
{
    int outcome;            // CuOutcome
    Cost rate, lambdaDistortion, cost;
    Cost costCoded;         // -1 without a residual
    Cost costNoResidual;
};

inline CuDecision closeInterCu(const CuCandidate &c, Lambda reciprocalLambda)
{
    CuDecision d;
    const int32_t ssd = int32_t(uint32_t(c.ssd[0]) + uint32_t(c.ssd[1]) + uint32_t(c.ssd[2]));
    const Cost distCoded = reciprocalLambda * ssd;
    const int without = c.merged2Nx2N ? kCuSkipped : kCuNoResidual;
    if (!c.haveResidual)
    {
        d.outcome = without;
        d.rate = c.rateNoResidual;
        d.lambdaDistortion = distCoded;
        d.costCoded = -1;
        d.costNoResidual = d.rate + distCoded;
    }
    else
    {
        Cost distPred = reciprocalLambda * c.ssdPrediction[0];
        distPred += reciprocalLambda * c.ssdPrediction[1];
        distPred += reciprocalLambda * c.ssdPrediction[2];
        d.costCoded = c.rateCoded + distCoded;
        d.costNoResidual = c.rateNoResidual + distPred;
        const bool drop = d.costNoResidual < d.costCoded;
        d.outcome = drop ? without : kCuCoded;
        d.rate = drop ? c.rateNoResidual : c.rateCoded;
        d.lambdaDistortion = drop ? distPred : distCoded;
    }
    d.cost = d.rate + d.lambdaDistortion;
    return d;
}

} // namespace havoc_search
