// TEST INFRASTRUCTURE ONLY.  search/tu_decision.hpp's decideRqt with the whole tree's rate per depth and the chroma functor -- the host form of
// havoc_mi355x_rqt_decide_tree -- for tests/tree_rate_tools.py to hold its numpy restatement (and through it the device) against.  Compiled at test time into a
// temporary directory.
#include "../turingcodec_amd/search/tu_decision.hpp"

using namespace havoc_search;

namespace {

struct View
{
    const int64_t *row;
    int evaluated[2];
    havoc_tu_outcome evaluate(int, int, int, int depth)
    {
        havoc_tu_outcome o = havoc_tu_outcome();
        if (depth == 1)
        {
            const int k = evaluated[1]++;
            o.cbf = int32_t(row[0] >> k & 1);
            o.ssd = uint32_t(row[1 + k]);
        }
        else
        {
            ++evaluated[0];
            o.cbf = int32_t(row[8] & 1);
            o.ssd = uint32_t(row[9]);
        }
        return o;
    }
};

struct Rate
{
    const int64_t *row;
    Cost operator()(int depth, const havoc_tu_outcome *, int) const { return depth ? row[7] : row[12]; }
};

struct Chroma
{
    const int64_t *row;
    ChromaOutcome operator()(int depth) const
    {
        const int64_t *p = depth ? row : row + 8;
        return ChromaOutcome{(p[0] & 0xff0) != 0, int32_t(uint32_t(depth ? p[5] : p[2])), int32_t(uint32_t(depth ? p[6] : p[3]))};
    }
};

} // namespace

// rows: int64 [n][13] = depth 1: cbf mask, ssdY of the four blocks, ssdCb, ssdCr (sums), the tree's rate; depth 0: cbf mask, ssdY, ssdCb, ssdCr, rate.
// out: int64 [n][5] = depth, tried_zero, cost_zero, cost_one, depth-0 blocks evaluated
extern "C" int tree_decide(const int64_t *rows, int n, int32_t rlQ16, int64_t *out)
{
    for (int i = 0; i < n; ++i)
    {
        const int64_t *row = rows + 13 * i;
        View view{row, {0, 0}};
        havoc_rqt_cu cu = havoc_rqt_cu();
        cu.log2_size = 4;
        Lambda l;
        l.value = rlQ16;
        const havoc_rqt_result r = decideRqt(view, cu, l, Rate{row}, Chroma{row});
        out[5 * i] = r.depth;
        out[5 * i + 1] = r.tried_zero;
        out[5 * i + 2] = r.cost_zero;
        out[5 * i + 3] = r.cost_one;
        out[5 * i + 4] = view.evaluated[0];
    }
    return 0;
}
