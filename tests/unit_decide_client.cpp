// TEST INFRASTRUCTURE ONLY.  search/tu_decision.hpp's decideRqt with the whole tree's rate per depth, the chroma functor and the unit's OWN size -- the host form of
// havoc_mi355x_rqt_decide_units, the inferred split of a 64x64 unit included -- for tests/unit_tree_tools.py to hold its numpy restatement (and through it the device)
// against.  Compiled at test time into a temporary directory.
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
    int asked[2];
    ChromaOutcome operator()(int depth)
    {
        ++asked[depth];
        const int64_t *p = depth ? row : row + 8;
        return ChromaOutcome{(p[0] & 0xff0) != 0, int32_t(uint32_t(depth ? p[5] : p[2])), int32_t(uint32_t(depth ? p[6] : p[3]))};
    }
};

struct ChromaRef
{
    Chroma *c;
    ChromaOutcome operator()(int depth) const { return (*c)(depth); }
};

} // namespace

// rows: int64 [n][14] = depth 1: cbf mask, ssdY of the four blocks, ssdCb, ssdCr (sums), the tree's rate; depth 0: cbf mask, ssdY, ssdCb, ssdCr, rate; the unit's
// log2 size (3..6; at 6 nothing of depth 0 may be asked for).  out: int64 [n][6] = depth, tried_zero, cost_zero, cost_one, depth-0 luma blocks evaluated, depth-0
// chroma asked for
extern "C" int unit_decide(const int64_t *rows, int n, int32_t rlQ16, int64_t *out)
{
    for (int i = 0; i < n; ++i)
    {
        const int64_t *row = rows + 14 * i;
        View view{row, {0, 0}};
        Chroma chroma{row, {0, 0}};
        havoc_rqt_cu cu = havoc_rqt_cu();
        cu.log2_size = int32_t(row[13]);
        Lambda l;
        l.value = rlQ16;
        const havoc_rqt_result r = decideRqt(view, cu, l, Rate{row}, ChromaRef{&chroma});
        out[6 * i] = r.depth;
        out[6 * i + 1] = r.tried_zero;
        out[6 * i + 2] = r.cost_zero;
        out[6 * i + 3] = r.cost_one;
        out[6 * i + 4] = view.evaluated[0];
        out[6 * i + 5] = chroma.asked[0];
    }
    return 0;
}
