// TEST INFRASTRUCTURE ONLY.  search/cqt_decision.hpp's cqtBlockCells -- the host form of havoc_mi355x_cqt_block_cells -- for tests/cqt_finish_tools.py to hold its
// numpy restatement (and through it the device) against.  Compiled at test time into a temporary directory.
#include "../turingcodec_amd/search/cqt_decision.hpp"

using namespace havoc_search;

static_assert(sizeof(CqtCommitCell) == 24 && sizeof(CqtBlockCell) == 16, "the records cqt_finish_tools.py passes");

// g: int32 [7] = width, height, minCbLog2, qp, dpb0, dpb1, stride (in cells); cqt: the committed cells; cells: the destination, the caller's sentinel in it
extern "C" void cqt_block_cells_picture(const int32_t *g, const void *cqt, void *cells)
{
    cqtBlockCells(g[0], g[1], g[2], g[3], g[4], g[5], static_cast<const CqtCommitCell *>(cqt), static_cast<CqtBlockCell *>(cells), g[6]);
}
