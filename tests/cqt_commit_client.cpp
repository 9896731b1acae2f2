// TEST INFRASTRUCTURE ONLY.  search/cqt_decision.hpp's commitCqt -- the host form of havoc_mi355x_cqt_commit, one CTU per call -- over a whole picture, for
// tests/cqt_commit_tools.py to hold its numpy restatement (and through it the device) against.  Compiled at test time into a temporary directory.
#include "../turingcodec_amd/search/cqt_decision.hpp"

using namespace havoc_search;

static_assert(sizeof(CqtCommitCell) == 24 && sizeof(CqtCommitTree) == 40 && sizeof(CqtCommitUnit) == 16, "the records cqt_commit_tools.py passes");

template <class Sample>
static int run(const int64_t *g, void *const *p)
{
    CqtCommit<Sample> P;
    P.width = int(g[1]), P.height = int(g[2]), P.ctbLog2 = int(g[3]), P.minCbLog2 = int(g[4]), P.n = int(g[5]);
    P.predStride = long(g[6]), P.predStrideC = long(g[7]), P.recOrigin = long(g[8]), P.recStride = long(g[9]);
    P.cbOrigin = long(g[10]), P.crOrigin = long(g[11]), P.cStride = long(g[12]);
    P.units = static_cast<const CqtCommitUnit *>(p[0]);
    P.outcome = static_cast<const int32_t *>(p[1]);
    P.tree = static_cast<const CqtCommitTree *>(p[2]);
    for (int k = 0; k < 4; ++k) P.lumaPieces[k] = static_cast<const Sample *>(p[3 + k]);
    for (int k = 0; k < 3; ++k) P.chromaPieces[k] = static_cast<const Sample *>(p[7 + k]);
    P.predY = static_cast<const Sample *>(p[10]), P.predC = static_cast<const Sample *>(p[11]);
    P.predOff = static_cast<const int32_t *>(p[12]), P.best = static_cast<const int32_t *>(p[13]), P.unitCand = static_cast<const int32_t *>(p[14]);
    P.candMv = static_cast<const int16_t *>(p[15]);
    P.recY = static_cast<Sample *>(p[16]), P.recC = static_cast<Sample *>(p[17]);
    P.cells = static_cast<CqtCommitCell *>(p[18]);
    const int32_t *nodeCu = static_cast<const int32_t *>(p[19]), *decided = static_cast<const int32_t *>(p[20]);
    const uint8_t *choice = static_cast<const uint8_t *>(p[21]), *flags = static_cast<const uint8_t *>(p[22]);
    const int count = cqtNodes(P.ctbLog2 - P.minCbLog2 + 1), size = 1 << P.ctbLog2;
    const int ctus = ((P.width + size - 1) >> P.ctbLog2) * ((P.height + size - 1) >> P.ctbLog2);
    int done = 0;
    for (int c = 0; c < ctus; ++c)
    {
        CqtNode node[85];
        for (int k = 0; k < count; ++k) node[k] = CqtNode{choice[c * count + k], flags[c * count + k], 0, 0, 0};
        done += commitCqt(P, c, decided[c] == 1, nodeCu + c * count, node);
    }
    return done;
}

// g: int64 [13] = bit depth, width, height, ctbLog2, minCbLog2, n, predStride, predStrideC, recOrigin, recStride, cbOrigin, crOrigin, cStride; p: the 23 arrays in
// run()'s order (candMv may be null).  The caller has set the cells to all-ones bytes.  -> the units committed
extern "C" int cqt_commit_picture(const int64_t *g, void *const *p) { return g[0] == 8 ? run<uint8_t>(g, p) : run<uint16_t>(g, p); }
