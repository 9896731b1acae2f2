// TEST INFRASTRUCTURE ONLY.  search/tu_decision.hpp's decideIntraRd with a rate per candidate, for tests/intra_rate_tools.py to hold its numpy restatement (and through
// it havoc_mi355x_intra_decide_rated) against.  Compiled at test time into a temporary directory.
//
// measureLikeTheReference: the rate functor answers kCostMax -- "not measured" -- for a challenger whose distortion alone is not below the champion's cost, as
// searchIntraPartition does (turing/Search.hpp:242-246); such a candidate cannot win, so the champion and its cost must be those of measuring every candidate.
#include "../turingcodec_amd/search/tu_decision.hpp"

using namespace havoc_search;

namespace {

struct View
{
    const uint32_t *ssd;
    havoc_tu_outcome evaluate(int, int j)
    {
        havoc_tu_outcome o = havoc_tu_outcome();
        o.ssd = ssd[j];
        return o;
    }
};

struct Rate
{
    const int64_t *rates;
    Lambda reciprocalLambda;
    bool measureLikeTheReference;
    Cost *champion;
    int64_t *unmeasured;
    Cost operator()(int, int j, const havoc_tu_outcome &o) const
    {
        const Cost distortion = reciprocalLambda * int32_t(o.ssd);
        if (measureLikeTheReference && !(distortion < *champion))
        {
            ++*unmeasured;
            return kCostMax;
        }
        const Cost cost = rates[j] + distortion;
        if (cost < *champion) *champion = cost;
        return rates[j];
    }
};

} // namespace

// order: int32 [n][HAVOC_MI355X_INTRA_MAX_ORDER = 12]; count, slot: int32 [n]; ssd, rates: per candidate slot; out: int64 [n][5] = mode, index, evaluated, cost, candidates
// whose rate was not measured
extern "C" int intra_rated_decide(const int32_t *order, const int32_t *count, const int32_t *slot, const uint32_t *ssd, const int64_t *rates, int n, int32_t rlQ16,
                                  int measureLikeTheReference, int64_t *out)
{
    for (int i = 0; i < n; ++i)
    {
        havoc_search_intra_result o = havoc_search_intra_result();
        o.count = count[i];
        for (int j = 0; j < count[i]; ++j) o.order[j] = order[12 * i + j];
        View view{ssd + slot[i]};
        Lambda l;
        l.value = rlQ16;
        Cost champion = kCostMax;
        int64_t unmeasured = 0;
        const havoc_intra_rd_result r = decideIntraRd(view, o, l, Rate{rates + slot[i], l, measureLikeTheReference != 0, &champion, &unmeasured});
        out[5 * i] = r.mode;
        out[5 * i + 1] = r.index;
        out[5 * i + 2] = r.evaluated;
        out[5 * i + 3] = r.cost;
        out[5 * i + 4] = unmeasured;
    }
    return 0;
}
