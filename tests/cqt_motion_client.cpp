// TEST INFRASTRUCTURE ONLY.  The host forms of havoc_mi355x_cqt_motion_store (search/cqt_decision.hpp's cqtMotionStore) and of havoc_mi355x_temporal_candidates
// (search/amvp.hpp's deriveTemporalCandidate, through temporalCandidateOf -- the record the kernel writes) for tests/cqt_motion_tools.py to hold its numpy
// restatements (and through them the device) against.  Compiled at test time into a temporary directory.
#include "../turingcodec_amd/search/amvp.hpp"
#include "../turingcodec_amd/search/cqt_decision.hpp"
#include "../turingcodec_amd/search/search_abi.h"

using namespace havoc_search;

static_assert(sizeof(CqtCommitCell) == 24 && sizeof(CqtColCell) == 24 && sizeof(ColStoreCell) == 24, "the records cqt_motion_tools.py passes");
static_assert(sizeof(TemporalParams) == 48 && sizeof(TemporalCand) == 8 && sizeof(havoc_picture_pu) == 32, "the records cqt_motion_tools.py passes");

// g: int32 [5] = width, height, minCbLog2, refPoc0, refPoc1; cqt: the committed cells; store: the destination, the caller's sentinel in it
extern "C" void cqt_motion_store_picture(const int32_t *g, const void *cqt, void *store)
{
    cqtMotionStore(g[0], g[1], g[2], g[3], g[4], static_cast<const CqtCommitCell *>(cqt), static_cast<CqtColCell *>(store));
}

// the call restated on the host: the two cells picked as the header states, the record made by amvp.hpp.  stride: records per store row
extern "C" void temporal_candidates_picture(const void *params, const void *store, long stride, const void *pus, int n, void *out)
{
    const TemporalParams &P = *static_cast<const TemporalParams *>(params);
    const ColStoreCell *s = static_cast<const ColStoreCell *>(store);
    const havoc_picture_pu *q = static_cast<const havoc_picture_pu *>(pus);
    TemporalCand *o = static_cast<TemporalCand *>(out);
    for (int p = 0; p < n; ++p)
        for (int X = 0; X < 2; ++X)
        {
            const int x0 = q[p].x0, y0 = q[p].y0, w = q[p].w, h = q[p].h;
            const bool inside = temporalPuInside(x0, y0, w, h, P), consulted = inside && temporalBottomRightConsulted(x0, y0, w, h, P);
            const ColStoreCell &centre = s[inside ? long((y0 + h / 2) >> 4) * stride + ((x0 + w / 2) >> 4) : 0];
            const ColStoreCell &bottomRight = consulted ? s[long((y0 + h) >> 4) * stride + ((x0 + w) >> 4)] : centre;
            o[2 * p + X] = temporalCandidateOf(x0, y0, w, h, P, bottomRight, centre, X);
        }
}
