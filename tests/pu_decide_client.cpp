// TEST INFRASTRUCTURE ONLY.  search/pu_decision.hpp's decidePu -- the host form of havoc_mi355x_pu_decide -- for tests/pu_rate_tools.py to hold its numpy
// restatement (and through it the device) against.  Compiled at test time into a temporary directory.
#include "../turingcodec_amd/search/pu_decision.hpp"
#include <vector>

using namespace havoc_search;

// first, count: int32 [n]; rates: int64 per candidate; satd: int32 [3][m] (Y, Cb, Cr); cost: int64 [m]; best: int32 [n]; best_cost: int64 [n]
extern "C" int pu_decide(const int32_t *first, const int32_t *count, int n, const int64_t *rates, const int32_t *satd, int m, int32_t lambdaQ16, int64_t *cost,
                         int32_t *best, int64_t *bestCost)
{
    Lambda l;
    l.value = lambdaQ16;
    for (int i = 0; i < n; ++i)
    {
        std::vector<PuCandidate> c(count[i]);
        for (int k = 0; k < count[i]; ++k)
        {
            const int t = first[i] + k;
            c[k] = PuCandidate{rates[t], {satd[t], satd[m + t], satd[2 * m + t]}};
        }
        const PuDecision d = decidePu(c.data(), count[i], l, cost + first[i]);
        best[i] = d.best;
        bestCost[i] = d.bestCost;
    }
    return 0;
}
