// cqt_decision.hpp -- the coding quadtree of one CTU, restated data-only beside closeInterCu (cu_decision.hpp).  Reference:
//   turing/SyntaxCtu.hpp:95-139   Syntax<coding_quadtree>::go: split_cu_flag is coded only for a node wholly inside the picture and larger than MinCb (:97-102), else
//                                 inferred (1 across the picture edge, 0 at MinCb); children in z-order (:117-135), a child whose origin lies outside the picture
//                                 is a Deleted<coding_quadtree>: no bits, no context;
//   turing/Binarization.h:102-122 the writer: one context-coded bin at ctxInc = (CtDepth left of (x0, y0) > cqtDepth) + (CtDepth above (x0, y0) > cqtDepth), the
//                                 depths from Neighbourhood::snake;
//   turing/Search.hpp:808-886     Search<coding_quadtree>::go:
//     :810-823  mustSplit (the node crosses the picture edge): split_cu_flag = 1, not coded, the children are walked, nothing is compared;
//     :839-851  testFull: the single CU from the state before the node, split_cu_flag(0) then the coding unit.  testFull == false (the reference reaches it through
//               rcudepth, :798-806) is generalised to "the node has no candidate CU";
//     :852-855  trySplit = !testFull || (testSplit && log2CbSize > MinCbLog2SizeY && !(ecu && CuPredMode == MODE_SKIP) && Speed::trySplit (always true,
//               turing/Speed.h:54)).  testSplit == false (rcudepth again, :795-801) is generalised to "no node below this one has a candidate CU": the unit stands;
//     :857-871  the split from the state before the node: split_cu_flag(1), then the children, each from what its predecessor left;
//     :875-884  the split replaces the single CU when !testFull || splitCandidate.cost2() < singleCandidate.cost2(): strict, equal costs keep the single CU.  The
//               reference's candidates carry the cost of the whole CTU so far; both hold the same prefix, so the node's own rate + lambdaDistortion compares the same.
// CtDepth of a neighbour the snake has not seen -- outside the picture, which is all there is at the picture's first row and column -- is -1: preCtu resets the
// picture's upper row and left column at the slice's first CTU (turing/StatePictures.h:1086-1101, BlockData::reset: CtDepth = -1), so it adds nothing to ctxInc.
// One CtDepth map per CTU is enough: a split candidate reads only cells it wrote itself or that lie outside the node; when the single CU wins after a split was tried
// the node's cells are rewritten.
// The candidates' RATES and the bin table are the caller's.  havoc_mi355x_cqt_decide walks every CTU of a picture on the device, bit for bit; this is its host form.
#pragma once

#include "decision.hpp"

namespace havoc_search {

enum CqtChoice { kCqtNotVisited = 0, kCqtCu = 1, kCqtSplit = 2, kCqtDeleted = 3 };
enum CqtNodeFlags { kCqtFinal = 1, kCqtFlagCoded = 2, kCqtMustSplit = 4, kCqtEcuStop = 8, kCqtNoCandidate = 16, kCqtNoSplitCandidate = 32 };

struct CqtCandidate         // a node's closed coding unit
{
    bool present;           // false: the node has no candidate
    bool skipped;           // it ended as a skipped CU (read with ecu)
    Cost rate, lambdaDistortion;
};

struct CqtNode
{
    uint8_t choice, flags, ctxInc;
    Cost costFull, costSplit;       // -1: not tried
};

struct CqtGeometry
{
    int levels;             // CtbLog2SizeY - MinCbLog2SizeY + 1, 1..4
    int cellsX, cellsY;     // the part of the CTU inside the picture, in MinCb cells, 1 .. 1 << (levels - 1)
    bool ecu;
};

struct CqtCtu
{
    bool decided;           // false: a node at MinCb had no candidate; nothing else is then set, the contexts and depths are the caller's to leave alone
    int nCus;
    Cost rate, flagRate, lambdaDistortion, cost;
};

constexpr int cqtNodes(int levels) { return levels <= 0 ? 0 : 1 + 4 * cqtNodes(levels - 1); }
constexpr int cqtFirst(int depth) { return cqtNodes(depth); }       // (4^depth - 1) / 3

struct CqtWalk
{
    const CqtCandidate *cand;
    const int32_t *bins;    // [2 state + bin] = new state | Q16 rate << 8 (measureEncodeDecision, turing/Write.h:476-492)
    CqtGeometry g;
    uint8_t ctx[3];
    int8_t cell[9][9];      // [y + 1][x + 1]: row 0 the upper neighbours, column 0 the left ones
    CqtNode *node;
    bool below[cqtNodes(4)];    // some node below this one has a candidate
    bool refused;

    struct Sum { Cost rate, flagRate, lambdaDistortion; };

    Cost bin(int inc, int b)
    {
        const int32_t e = bins[2 * ctx[inc] + b];
        ctx[inc] = uint8_t(e & 255);
        return e >> 8;
    }

    void fill(int x, int y, int s, int d)
    {
        for (int j = 0; j < s; ++j)
            for (int i = 0; i < s; ++i) cell[y + j + 1][x + i + 1] = int8_t(d);
    }

    Sum go(int d, int z, int x, int y)
    {
        const int s = 1 << (g.levels - 1 - d);
        CqtNode &n = node[cqtFirst(d) + z];
        const CqtCandidate &c = cand[cqtFirst(d) + z];
        const bool mustSplit = x + s > g.cellsX || y + s > g.cellsY, minCb = d == g.levels - 1, coded = !mustSplit && !minCb;
        n.costFull = n.costSplit = -1;
        n.ctxInc = 0;
        n.flags = 0;
        int inc = 0;
        if (coded)
        {
            inc = (cell[y + 1][x] > d) + (cell[y][x + 1] > d);
            n.ctxInc = uint8_t(inc);
            n.flags |= kCqtFlagCoded;
        }
        if (mustSplit)
        {
            n.flags |= kCqtMustSplit;
            n.choice = kCqtSplit;
            const Sum r = children(d, z, x, y);
            n.costSplit = r.rate + r.lambdaDistortion;
            return r;
        }
        const uint8_t before[3] = {ctx[0], ctx[1], ctx[2]};
        Sum full = {0, 0, 0};
        if (c.present)
        {
            if (coded) full.flagRate = bin(inc, 0);
            full.rate = full.flagRate + c.rate;
            full.lambdaDistortion = c.lambdaDistortion;
            fill(x, y, s, d);
            n.costFull = full.rate + full.lambdaDistortion;
            n.choice = kCqtCu;
        }
        else
            n.flags |= kCqtNoCandidate;
        const bool ecuStop = c.present && !minCb && g.ecu && c.skipped;
        if (ecuStop) n.flags |= kCqtEcuStop;
        const bool bare = c.present && !minCb && !below[cqtFirst(d) + z];
        if (bare) n.flags |= kCqtNoSplitCandidate;
        if (c.present && (minCb || ecuStop || bare)) return full;
        if (minCb)
        {
            refused = true;
            return full;
        }
        const uint8_t after[3] = {ctx[0], ctx[1], ctx[2]};
        for (int k = 0; k < 3; ++k) ctx[k] = before[k];
        const Cost flag = coded ? bin(inc, 1) : 0;
        Sum split = children(d, z, x, y);
        if (refused) return split;
        split.rate += flag;
        split.flagRate += flag;
        n.costSplit = split.rate + split.lambdaDistortion;
        if (!c.present || n.costSplit < n.costFull)
        {
            n.choice = kCqtSplit;
            return split;
        }
        for (int k = 0; k < 3; ++k) ctx[k] = after[k];
        fill(x, y, s, d);
        return full;
    }

    Sum children(int d, int z, int x, int y)
    {
        const int h = 1 << (g.levels - 2 - d);
        Sum r = {0, 0, 0};
        for (int k = 0; k < 4 && !refused; ++k)
        {
            const int cx = x + (k & 1) * h, cy = y + (k >> 1) * h;
            if (cx >= g.cellsX || cy >= g.cellsY)
            {
                node[cqtFirst(d + 1) + 4 * z + k].choice = kCqtDeleted;
                continue;
            }
            const Sum c = go(d + 1, 4 * z + k, cx, cy);
            r.rate += c.rate;
            r.flagRate += c.flagRate;
            r.lambdaDistortion += c.lambdaDistortion;
        }
        return r;
    }
};

// cand, node: cqtNodes(g.levels) entries in node-index order; ctx: split_cu_flag's three ContextModel::state, moved by the decided tree; left[y], up[x]: CtDepth of
// the cells left of and above the CTU (-1 outside the picture); depth[y][x]: the CTU's cells, written for the decided tree (0 outside the picture).
// A refused CTU: decided false, ctx as it came, node records and depths all 0.
inline CqtCtu decideCqt(const CqtCandidate *cand, const int32_t *bins, const CqtGeometry &g, uint8_t ctx[3], const int8_t left[8], const int8_t up[8], CqtNode *node,
                        int8_t depth[8][8])
{
    CqtWalk w;
    w.cand = cand, w.bins = bins, w.g = g, w.node = node, w.refused = false;
    const int cells = 1 << (g.levels - 1), count = cqtNodes(g.levels);
    for (int k = 0; k < 3; ++k) w.ctx[k] = ctx[k];
    for (int j = 0; j < 9; ++j)
        for (int i = 0; i < 9; ++i) w.cell[j][i] = 0;
    for (int k = 0; k < cells; ++k) w.cell[k + 1][0] = left[k], w.cell[0][k + 1] = up[k];
    for (int k = 0; k < count; ++k) node[k] = CqtNode{0, 0, 0, 0, 0};
    for (int d = g.levels - 1; d >= 0; --d)
        for (int z = 0; z < 1 << (2 * d); ++z)
        {
            bool any = false;
            for (int k = 0; k < 4 && d + 1 < g.levels; ++k) any = any || cand[cqtFirst(d + 1) + 4 * z + k].present || w.below[cqtFirst(d + 1) + 4 * z + k];
            w.below[cqtFirst(d) + z] = any;
        }
    const CqtWalk::Sum r = w.go(0, 0, 0, 0);
    CqtCtu out = {!w.refused, 0, 0, 0, 0, 0};
    for (int j = 0; j < 8; ++j)
        for (int i = 0; i < 8; ++i) depth[j][i] = w.refused || j >= cells || i >= cells ? 0 : w.cell[j + 1][i + 1];
    if (w.refused)
    {
        for (int k = 0; k < count; ++k) node[k] = CqtNode{0, 0, 0, 0, 0};
        return out;
    }
    // the decided tree: a node whose every ancestor chose the split
    node[0].flags |= kCqtFinal;
    for (int d = 1; d < g.levels; ++d)
        for (int z = 0; z < 1 << (2 * d); ++z)
        {
            const CqtNode &p = node[cqtFirst(d - 1) + (z >> 2)];
            CqtNode &n = node[cqtFirst(d) + z];
            if ((p.flags & kCqtFinal) && p.choice == kCqtSplit && n.choice != kCqtNotVisited) n.flags |= kCqtFinal;
        }
    for (int k = 0; k < count; ++k) out.nCus += (node[k].flags & kCqtFinal) && node[k].choice == kCqtCu;
    for (int k = 0; k < 3; ++k) ctx[k] = w.ctx[k];
    out.rate = r.rate, out.flagRate = r.flagRate, out.lambdaDistortion = r.lambdaDistortion, out.cost = r.rate + r.lambdaDistortion;
    return out;
}

} // namespace havoc_search
