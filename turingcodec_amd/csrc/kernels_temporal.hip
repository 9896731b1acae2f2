// k_temporal_candidates: the temporal motion vector candidate of every prediction unit of a picture, per list, from the collocated picture's motion store
// (turing/Mvp.h:44-181; HEVC 8.5.3.2.8 / 8.5.3.2.9).  DESIGN 7, row f2^10.  The rule is NOT restated here: search/amvp.hpp's deriveTemporalCandidate -- pinned against
// the traced reference encoder's own derivations -- is one text compiled for the host and for gfx950, as decision.hpp is in kernels_search.hip, and
// temporalCandidateOf (same file) is the record this kernel writes, so the host form and the device form cannot drift apart.
//
// A lane per (prediction unit, list): two aligned 8-byte loads of the unit's geometry, at most two 24-byte cell reads (three aligned 8-byte loads each: the centre cell,
// and the bottom-right cell where the rule consults it -- where it does not, the lane reads the centre cell's address again, never a cell outside the store), one
// aligned 8-byte store.  No LDS, no atomics.  A 1080p picture has a few thousand units: the launch is bound by its latency.
#include "common.h"
#include "launch.h"

#include "../search/search_abi.h"
#include "../search/amvp.hpp"

namespace havoc_gpu {

namespace {

using havoc_search::ColStoreCell;
using havoc_search::TemporalCand;
using havoc_search::TemporalParams;

static_assert(sizeof(ColStoreCell) == sizeof(havoc_mi355x_col_cell) && sizeof(ColStoreCell) == 24, "amvp.hpp's store record is the ABI's");
static_assert(sizeof(TemporalParams) == sizeof(havoc_mi355x_temporal_params) && sizeof(TemporalParams) == 48, "amvp.hpp's parameters are the ABI's");
static_assert(sizeof(TemporalCand) == sizeof(havoc_mi355x_temporal_cand) && sizeof(TemporalCand) == 8, "amvp.hpp's candidate record is the ABI's");
static_assert(sizeof(havoc_picture_pu) == 32, "search_abi.h");

__device__ __forceinline__ ColStoreCell load_col_cell(const havoc_mi355x_col_cell *p)
{
    const unsigned long long *r = reinterpret_cast<const unsigned long long *>(p);
    const unsigned long long a = r[0], b = r[1], f = r[2];
    ColStoreCell c;
    c.mv[0][0] = (int16_t)a; c.mv[0][1] = (int16_t)(a >> 16); c.mv[1][0] = (int16_t)(a >> 32); c.mv[1][1] = (int16_t)(a >> 48);
    c.refPoc[0] = (int32_t)(uint32_t)b; c.refPoc[1] = (int32_t)(uint32_t)(b >> 32);
    c.predFlag[0] = (uint8_t)f; c.predFlag[1] = (uint8_t)(f >> 8); c.longTerm[0] = (uint8_t)(f >> 16); c.longTerm[1] = (uint8_t)(f >> 24);
    c.reserved = (uint32_t)(f >> 32);
    return c;
}

__global__ __launch_bounds__(256) void k_temporal_candidates(TemporalParams P, const havoc_mi355x_col_cell *__restrict__ store, long stride,
                                                             const havoc_picture_pu *__restrict__ pus, int count, havoc_mi355x_temporal_cand *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int p = i >> 1, X = i & 1;
    const u32x2 *g = reinterpret_cast<const u32x2 *>(pus + p);
    const u32x2 g0 = g[0], g1 = g[1];
    const int x0 = (int)g0.x, y0 = (int)g0.y, w = (int)g1.x, h = (int)g1.y;
    // a unit that is not inside the picture reads cell (0, 0) -- which exists -- and gets no candidate
    const bool inside = havoc_search::temporalPuInside(x0, y0, w, h, P);
    const bool consulted = inside && havoc_search::temporalBottomRightConsulted(x0, y0, w, h, P);
    const int xc = inside ? (x0 + w / 2) >> 4 : 0, yc = inside ? (y0 + h / 2) >> 4 : 0;
    const int xb = consulted ? (x0 + w) >> 4 : xc, yb = consulted ? (y0 + h) >> 4 : yc;
    const ColStoreCell centre = load_col_cell(store + (long)yc * stride + xc), bottomRight = load_col_cell(store + (long)yb * stride + xb);
    const TemporalCand r = havoc_search::temporalCandidateOf(x0, y0, w, h, P, bottomRight, centre, X);
    *reinterpret_cast<u32x2 *>(out + i) = u32x2{(uint32_t)(uint16_t)r.mv[0] | (uint32_t)(uint16_t)r.mv[1] << 16, (uint32_t)(uint16_t)r.available | (uint32_t)(uint16_t)r.source << 16};
}

} // namespace

hipError_t launch_temporal_candidates(hipStream_t st, const havoc_mi355x_temporal_params &params, const havoc_mi355x_col_cell *store, long stride, const void *pus, int n,
                                      havoc_mi355x_temporal_cand *out)
{
    const TemporalParams P = {params.pic_width, params.pic_height, params.ctb_log2, params.col_poc, params.cur_poc, {params.target_poc[0], params.target_poc[1]},
                              params.all_backwards, params.collocated_from_l0, {0, 0, 0}};
    const int count = 2 * n;
    hipLaunchKernelGGL(k_temporal_candidates, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, P, store, stride, static_cast<const havoc_picture_pu *>(pus), count, out);
    return hipGetLastError();
}

} // namespace havoc_gpu
