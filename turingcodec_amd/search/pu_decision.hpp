// pu_decision.hpp -- the mode decision of one prediction unit among the candidates the search tried, restated data-only beside decideRqt and decideIntraRd
// (tu_decision.hpp).  Reference: turing/Search.hpp
//   :1656-1706  measurePuCost: rate(Syntax<prediction_unit> under Measure<void>) + (satdY + satdCb + satdCr) * reciprocalSqrtLambda -- the sum in int32,
//               FixedPoint<int32_t, 16> * int32_t -> FixedPoint<int64_t, 16> (turing/FixedPoint.h:79);
//   :1829-1842  compare: a candidate replaces the best only when cost < bestCost, so the first of the cheapest wins;
//   :1844-1902  go2: the candidates in the order they are tried -- merge 0..N-1 for units that are not 2Nx2N, uni L0, uni L1, bi -- each priced from the contexts
//               the unit started with; which of them exist (a list without a reference, no bi on 8x4 / 4x8 or without both uni candidates) is the caller's list.
// The RATE is the caller's per candidate: havoc_mi355x_pu_rate measures it on the device, bit for bit; a rate of -1 marks a candidate the syntax cannot code,
// which is never chosen.  This is the host form of havoc_mi355x_pu_decide.
#pragma once

#include "decision.hpp"

namespace havoc_search {

struct PuCandidate
{
    Cost rate;              // Q16 bits, or -1
    int32_t satd[3];        // Y, Cb, Cr
};

struct PuDecision
{
    int best;               // index among the candidates, -1: none is valid
    Cost bestCost;          // its cost, -1 when best == -1
};

inline Cost puCost(const PuCandidate &c, Lambda reciprocalSqrtLambda)
{
    if (c.rate < 0) return -1;
    const int32_t satd = int32_t(uint32_t(c.satd[0]) + uint32_t(c.satd[1]) + uint32_t(c.satd[2]));
    return c.rate + reciprocalSqrtLambda * satd;
}

// costs: NULL, or `count` entries: every candidate's cost (-1 for a refused one)
inline PuDecision decidePu(const PuCandidate *candidates, int count, Lambda reciprocalSqrtLambda, Cost *costs = nullptr)
{
    PuDecision d = {-1, -1};
    for (int k = 0; k < count; ++k)
    {
        const Cost cost = puCost(candidates[k], reciprocalSqrtLambda);
        if (costs) costs[k] = cost;
        if (candidates[k].rate < 0) continue;
        if (d.best < 0 || cost < d.bestCost)
        {
            d.best = k;
            d.bestCost = cost;
        }
    }
    return d;
}

} // namespace havoc_search
