// TEST INFRASTRUCTURE ONLY.  search/cqt_decision.hpp's decideCqt -- the host form of havoc_mi355x_cqt_decide's walk of one CTU -- for tests/cqt_tools.py to hold its
// Python restatement (and through it the device) against.  Compiled at test time into a temporary directory.
#include "../turingcodec_amd/search/cqt_decision.hpp"

using namespace havoc_search;

// geometry: int32 [4] = levels, cellsX, cellsY, ecu; cand: int64 [nodes][4] = present, skipped, rate, lambdaDistortion; bins: int32 [256]; ctx: 3 states, updated;
// left, up: int8 [8]; out: int64 [6] = decided, nCus, rate, flagRate, lambdaDistortion, cost; nodes: int64 [nodes][5] = choice, flags, ctxInc, costFull, costSplit;
// depth: int8 [64]
extern "C" int cqt_decide_ctu(const int32_t *geometry, const int64_t *cand, const int32_t *bins, uint8_t *ctx, const int8_t *left, const int8_t *up, int64_t *out,
                              int64_t *nodes, int8_t *depth)
{
    const CqtGeometry g = {geometry[0], geometry[1], geometry[2], geometry[3] != 0};
    const int count = cqtNodes(g.levels);
    CqtCandidate c[85];
    CqtNode n[85];
    for (int k = 0; k < count; ++k) c[k] = CqtCandidate{cand[4 * k] != 0, cand[4 * k + 1] != 0, cand[4 * k + 2], cand[4 * k + 3]};
    const CqtCtu r = decideCqt(c, bins, g, ctx, left, up, n, reinterpret_cast<int8_t(*)[8]>(depth));
    out[0] = r.decided, out[1] = r.nCus, out[2] = r.rate, out[3] = r.flagRate, out[4] = r.lambdaDistortion, out[5] = r.cost;
    for (int k = 0; k < count; ++k)
        nodes[5 * k] = n[k].choice, nodes[5 * k + 1] = n[k].flags, nodes[5 * k + 2] = n[k].ctxInc, nodes[5 * k + 3] = n[k].costFull, nodes[5 * k + 4] = n[k].costSplit;
    return 0;
}
