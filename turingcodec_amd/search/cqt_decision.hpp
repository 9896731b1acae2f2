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

// ---- acting on the decision: the final coding units of one CTU into the picture and the per-cell field.  havoc_mi355x_cqt_commit does this for every CTU of a
// picture in one launch, byte for byte; this is its host form, data-only: every sample was made before (the winner's prediction of each searched unit, the candidate
// pieces of both transform depths), commitCqt selects.  What the reference's picture holds after Search<coding_quadtree>::go kept the CTU's winner (turing/Search.hpp:
// 808-886 over :2362-2568): a unit left without residual or skipped is its prediction, a coded unit the reconstruction of the transform depth that stands.
struct CqtCommitUnit { int32_t x0, y0, log2Size, ctxIndex; };       // a searched unit (= havoc_mi355x_rqt_unit)
struct CqtCommitTree        // what is read of a unit's transform-tree records
{
    int32_t depth, triedZero;           // rqt_decide_units': the depth that stands is (log2Size < 6 && depth == 0 && triedZero) ? 0 : 1
    uint32_t maskZero, maskOne;         // the trees' cbf masks
    int32_t zeroAt, oneAt;              // the luma candidates: one of size log2Size, the first of four of size log2Size - 1
    int32_t cbZero, crZero, cbOne, crOne;   // the chroma candidates: one of size log2Size - 1, the first of four of size log2Size - 2 (an 8x8 unit: cbZero / crZero only)
};
struct CqtCommitCell        // = havoc_mi355x_cqt_cell, 24 bytes
{
    int32_t unit, cand;
    int16_t mv[2][2];
    uint8_t log2Size, outcome, pred, trDepth;
    uint32_t cbf;
};
template <class Sample>
struct CqtCommit
{
    int width, height, ctbLog2, minCbLog2, n;
    const CqtCommitUnit *units;         // [n]; index p means the same unit in every table
    const int32_t *outcome;             // the close's: -1 refused, 0 coded, 1 no residual, 2 skipped
    const CqtCommitTree *tree;
    const Sample *lumaPieces[4];        // transform sizes 2..5: candidate j of size s is the contiguous block at j << 2 s
    const Sample *chromaPieces[3];      // 2..4
    const Sample *predY, *predC;        // the unit prediction planes
    long predStride, predStrideC;
    const int32_t *predOff;             // [n][3]: a unit's block in predY; in predC for Cb, Cr
    const int32_t *best, *unitCand;     // the winning mode (0 L0, 1 L1, 2 bi) and candidate
    const int16_t *candMv;              // [candidates][2 lists][x, y], or null: zero vectors
    Sample *recY;
    long recOrigin, recStride;
    Sample *recC;
    long cbOrigin, crOrigin, cStride;
    CqtCommitCell *cells;               // one per MinCb cell of the picture; a cell no unit covers is the caller's (all-ones bytes)
};

template <class Sample>
inline void cqtCopyBlock(Sample *d, long sd, const Sample *a, long sa, int log2)
{
    for (int y = 0; y < 1 << log2; ++y)
        for (int x = 0; x < 1 << log2; ++x) d[y * sd + x] = a[y * sa + x];
}

// one piece of size log2, or four of size log2 - 1 in z-order
template <class Sample>
inline void cqtCopyPieces(Sample *d, long sd, const Sample *const *pieces, int log2, bool quads, int at)
{
    if (!quads)
    {
        cqtCopyBlock(d, sd, pieces[log2 - 2] + (long(at) << 2 * log2), 1l << log2, log2);
        return;
    }
    const int l = log2 - 1;
    for (int q = 0; q < 4; ++q) cqtCopyBlock(d + (long(q >> 1) << l) * sd + (long(q & 1) << l), sd, pieces[l - 2] + (long(at + q) << 2 * l), 1l << l, l);
}

// ctu: raster index; nodeCu, node: the CTU's cqtNodes(levels) entries as decideCqt read and wrote them.  Unit p = nodeCu[k] is committed when node k is final with
// choice kCqtCu, p's own origin and size name node k of this CTU, and its outcome is one of the three that are not refused.  -> the units committed
template <class Sample>
inline int commitCqt(const CqtCommit<Sample> &P, int ctu, bool decided, const int32_t *nodeCu, const CqtNode *node)
{
    if (!decided) return 0;
    const int levels = P.ctbLog2 - P.minCbLog2 + 1, count = cqtNodes(levels), cx = (P.width + (1 << P.ctbLog2) - 1) >> P.ctbLog2;
    int done = 0;
    for (int k = 0; k < count; ++k)
    {
        const int p = nodeCu[k];
        if (p < 0 || p >= P.n || !(node[k].flags & kCqtFinal) || node[k].choice != kCqtCu) continue;
        const CqtCommitUnit &u = P.units[p];
        const int L = u.log2Size, size = 1 << L, d = P.ctbLog2 - L;
        if (L < P.minCbLog2 || d < 0) continue;
        if (u.x0 < 0 || u.y0 < 0 || ((u.x0 | u.y0) & (size - 1)) || u.x0 + size > P.width || u.y0 + size > P.height) continue;
        const int px = (u.x0 & ((1 << P.ctbLog2) - 1)) >> L, py = (u.y0 & ((1 << P.ctbLog2) - 1)) >> L;
        int z = 0;
        for (int b = 0; b < 3; ++b) z |= (px >> b & 1) << 2 * b | (py >> b & 1) << (2 * b + 1);
        if ((u.y0 >> P.ctbLog2) * cx + (u.x0 >> P.ctbLog2) != ctu || cqtFirst(d) + z != k) continue;
        const int outcome = P.outcome[p];
        if (outcome < 0 || outcome > 2) continue;
        Sample *recY = P.recY + P.recOrigin + long(u.y0) * P.recStride + u.x0;
        const long cAt = long(u.y0 >> 1) * P.cStride + (u.x0 >> 1);
        int trDepth = 0;
        uint32_t cbf = 0;
        if (outcome == 0)
        {
            const CqtCommitTree &t = P.tree[p];
            trDepth = (L < 6 && t.depth == 0 && t.triedZero) ? 0 : 1;
            cbf = trDepth ? t.maskOne : t.maskZero;
            cqtCopyPieces(recY, P.recStride, P.lumaPieces, L, trDepth != 0, trDepth ? t.oneAt : t.zeroAt);
            const bool quads = trDepth != 0 && L > 3;
            cqtCopyPieces(P.recC + P.cbOrigin + cAt, P.cStride, P.chromaPieces, L - 1, quads, quads ? t.cbOne : t.cbZero);
            cqtCopyPieces(P.recC + P.crOrigin + cAt, P.cStride, P.chromaPieces, L - 1, quads, quads ? t.crOne : t.crZero);
        }
        else
        {
            const int32_t *off = P.predOff + 3 * long(p);
            cqtCopyBlock(recY, P.recStride, P.predY + off[0], P.predStride, L);
            cqtCopyBlock(P.recC + P.cbOrigin + cAt, P.cStride, P.predC + off[1], P.predStrideC, L - 1);
            cqtCopyBlock(P.recC + P.crOrigin + cAt, P.cStride, P.predC + off[2], P.predStrideC, L - 1);
        }
        CqtCommitCell cell = {p, P.unitCand[p], {{0, 0}, {0, 0}}, uint8_t(L), uint8_t(outcome), uint8_t(P.best[p]), uint8_t(trDepth), cbf};
        if (P.candMv && cell.cand >= 0)
            for (int l = 0; l < 2; ++l)
                if (cell.pred == l || cell.pred == 2) cell.mv[l][0] = P.candMv[4 * long(cell.cand) + 2 * l], cell.mv[l][1] = P.candMv[4 * long(cell.cand) + 2 * l + 1];
        const int cl = L - P.minCbLog2, wc = P.width >> P.minCbLog2;
        for (int j = 0; j < 1 << cl; ++j)
            for (int i = 0; i < 1 << cl; ++i) P.cells[long((u.y0 >> P.minCbLog2) + j) * wc + (u.x0 >> P.minCbLog2) + i] = cell;
        ++done;
    }
    return done;
}

// ---- the committed cells as the loop filter's block structure: the map of 4x4 cells havoc_mi355x_derive_bs reads, every coding unit one inter 2Nx2N prediction unit.
// havoc_mi355x_cqt_block_cells does this in one launch, byte for byte; this is its host form, data-only.  What LoopFilter::Picture::processCu / processPu / processTu /
// processRc see of the decided picture (turing/LoopFilter.h:541-737).
struct CqtBlockCell         // = havoc_mi355x_cell, 16 bytes
{
    int16_t mv[2][2];
    int8_t dpbIndex[2];
    uint8_t flags;
    int8_t qpY;
    uint8_t tuLog2;
    uint8_t reserved[3];
};
constexpr int kCellCoded = 2, kCellNoFilter = 4, kCellPuLeft = 8, kCellPuTop = 16;      // HAVOC_CELL_*

// cqt: (height >> minCbLog2) rows of (width >> minCbLog2) committed cells; cells: (height / 4) rows of (width / 4), `stride` cells apart, every one written.  A coding
// unit is aligned to its size, so a cell's own position names its unit's origin.
inline void cqtBlockCells(int width, int height, int minCbLog2, int qp, int dpb0, int dpb1, const CqtCommitCell *cqt, CqtBlockCell *cells, long stride)
{
    const int wc = width >> minCbLog2;
    for (int y = 0; y < height; y += 4)
        for (int x = 0; x < width; x += 4)
        {
            const CqtCommitCell &q = cqt[long(y >> minCbLog2) * wc + (x >> minCbLog2)];
            CqtBlockCell c = {{{0, 0}, {0, 0}}, {-1, -1}, uint8_t(kCellNoFilter), int8_t(qp), 2, {0, 0, 0}};     // an undecided CTU's: nobody's samples, left alone
            if (q.unit >= 0)
            {
                const int size = 1 << q.log2Size, ox = x & (size - 1), oy = y & (size - 1);
                const int k = q.trDepth ? (oy >= size / 2) * 2 + (ox >= size / 2) : 0;
                for (int l = 0; l < 2; ++l) c.mv[l][0] = q.mv[l][0], c.mv[l][1] = q.mv[l][1];
                c.dpbIndex[0] = int8_t(q.pred != 1 ? dpb0 : -1);
                c.dpbIndex[1] = int8_t(q.pred != 0 ? dpb1 : -1);
                c.flags = uint8_t((q.outcome == 0 && (q.cbf >> k & 1) ? kCellCoded : 0) | (ox == 0 ? kCellPuLeft : 0) | (oy == 0 ? kCellPuTop : 0));
                c.tuLog2 = uint8_t(q.log2Size - q.trDepth < 5 ? q.log2Size - q.trDepth : 5);
            }
            cells[long(y >> 2) * stride + (x >> 2)] = c;
        }
}

// ---- the committed cells as the collocated motion store (turing/StateCollocatedMotion.h:51-122): what the NEXT picture's temporal candidate is derived from.
// havoc_mi355x_cqt_motion_store does this in one launch, byte for byte; this is its host form, data-only.  fillRectangle (:75-90) writes entry (X, Y) for every
// x0 <= 16 X < x1, y0 <= 16 Y < y1 of a unit: the entry holds the motion of the unit that CONTAINS luma sample (16 X, 16 Y) -- an 8x8 unit off the 16-grid writes
// none, a 64x64 unit sixteen -- and the final units partition a CTU, so the cell that covers that sample names the one writer.
struct CqtColCell           // = havoc_mi355x_col_cell = amvp.hpp's ColStoreCell, 24 bytes
{
    int16_t mv[2][2];
    int32_t refPoc[2];
    uint8_t predFlag[2], longTerm[2];
    uint32_t reserved;
};

// cqt: (height >> minCbLog2) rows of (width >> minCbLog2) committed cells; store: (height + 15) / 16 dense rows of (width + 15) / 16 records, every one written.
// refPoc0 / refPoc1: the picture order counts of the pictures behind lists 0 and 1 (reference index 0).  An undecided CTU's entries are "not available" (all zero),
// as the reference's default PuData is
inline void cqtMotionStore(int width, int height, int minCbLog2, int refPoc0, int refPoc1, const CqtCommitCell *cqt, CqtColCell *store)
{
    const int wc = width >> minCbLog2, sw = (width + 15) / 16, sh = (height + 15) / 16;
    for (int Y = 0; Y < sh; ++Y)
        for (int X = 0; X < sw; ++X)
        {
            const CqtCommitCell &q = cqt[long(16 * Y >> minCbLog2) * wc + (16 * X >> minCbLog2)];
            CqtColCell c = {{{0, 0}, {0, 0}}, {0, 0}, {0, 0}, {0, 0}, 0};
            if (q.unit >= 0)
                for (int l = 0; l < 2; ++l)
                    if (q.pred != 1 - l)       // 0 L0, 1 L1, 2 bi
                    {
                        c.predFlag[l] = 1;
                        c.mv[l][0] = q.mv[l][0], c.mv[l][1] = q.mv[l][1];
                        c.refPoc[l] = l ? refPoc1 : refPoc0;
                    }
            store[long(Y) * sw + X] = c;
        }
}

} // namespace havoc_search
