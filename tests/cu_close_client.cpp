// TEST INFRASTRUCTURE ONLY.  search/cu_decision.hpp's closeInterCu -- the host form of havoc_mi355x_cu_close's decision -- for tests/cu_close_tools.py to hold its
// numpy restatement (and through it the device) against.  Compiled at test time into a temporary directory.
#include "../turingcodec_amd/search/cu_decision.hpp"

using namespace havoc_search;

// per unit: in int64 [10] = haveResidual, merged2Nx2N, rateCoded, rateNoResidual, ssd[3], ssdPrediction[3]; out int64 [6] = outcome, rate, lambdaDistortion, cost,
// costCoded, costNoResidual
extern "C" int cu_close_decide(const int64_t *in, int n, int32_t lambdaQ16, int64_t *out)
{
    Lambda l;
    l.value = lambdaQ16;
    for (int i = 0; i < n; ++i, in += 10, out += 6)
    {
        const CuCandidate c = {in[0] != 0, in[1] != 0, in[2], in[3], {int32_t(in[4]), int32_t(in[5]), int32_t(in[6])}, {int32_t(in[7]), int32_t(in[8]), int32_t(in[9])}};
        const CuDecision d = closeInterCu(c, l);
        out[0] = d.outcome, out[1] = d.rate, out[2] = d.lambdaDistortion, out[3] = d.cost, out[4] = d.costCoded, out[5] = d.costNoResidual;
    }
    return 0;
}
