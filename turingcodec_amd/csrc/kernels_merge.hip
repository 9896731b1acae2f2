// k_cqt_merge_lists: the merge candidate list of every final coding unit of a committed picture, and the lowest merge index that carries the unit's committed motion
// (turing/Mvp.h:486-716; HEVC 8.5.3.2.2 - 8.5.3.2.5).  DESIGN 7, row f2^12.  The rule is NOT restated here: search/merge_list.hpp's cqtMergeList -- the fetch stated
// in include/havoc_mi355x.h plus deriveMergeCandidateList, held against tests/merge.hpp and the traced reference encoder's own lists -- is one text compiled for the
// host and for gfx950, as amvp.hpp's temporalCandidateOf is in kernels_temporal.hip, so the host form and the device form cannot drift apart.
//
// A lane per searched unit, 64-lane workgroups: two aligned 8-byte loads of the unit's geometry; for a unit whose geometry can be a final unit's the origin cell,
// then at most five neighbour cells (three aligned 8-byte loads each, only where neighbourPositionAvailable allows the position -- never a cell outside the map) and
// the unit's two temporal records (two aligned 8-byte loads); eight aligned 8-byte stores.  Neighbours and list live in registers: merge_list.hpp indexes nothing by
// a run-time value.  No LDS, no atomics, no scratch.  A 1080p picture has a few thousand units: the launch is bound by its latency.
#include "common.h"
#include "launch.h"

#include "../search/search_abi.h"
#include "../search/merge_list.hpp"

namespace havoc_gpu {

namespace {

using havoc_search::merge_list::CqtMergeParams;
using havoc_search::merge_list::CqtMergeRecord;

static_assert(sizeof(CqtMergeParams) == sizeof(havoc_mi355x_merge_params) && sizeof(CqtMergeParams) == 48, "merge_list.hpp's parameters are the ABI's");
static_assert(sizeof(CqtMergeRecord) == sizeof(havoc_mi355x_merge_list) && sizeof(CqtMergeRecord) == 64, "merge_list.hpp's record is the ABI's");
static_assert(sizeof(havoc_mi355x_cqt_cell) == 24 && sizeof(havoc_mi355x_temporal_cand) == 8 && sizeof(havoc_picture_pu) == 32, "the tables cqtMergeList reads in 8-byte words");

__global__ __launch_bounds__(64) void k_cqt_merge_lists(CqtMergeParams P, const unsigned long long *__restrict__ cells, const havoc_picture_pu *__restrict__ pus, int n,
                                                        const unsigned long long *__restrict__ temporal, havoc_mi355x_merge_list *__restrict__ out)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    const u32x2 *g = reinterpret_cast<const u32x2 *>(pus + p);
    const u32x2 g0 = g[0], g1 = g[1];
    const CqtMergeRecord r = havoc_search::merge_list::cqtMergeList(P, cells, temporal, p, (int)g0.x, (int)g0.y, (int)g1.x, (int)g1.y);
    unsigned long long *o = reinterpret_cast<unsigned long long *>(out + p);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = r.w[j];
}

} // namespace

hipError_t launch_cqt_merge_lists(hipStream_t st, const havoc_mi355x_merge_params &params, const havoc_mi355x_cqt_cell *cqtCells, const void *pus, int n,
                                  const havoc_mi355x_temporal_cand *temporal, havoc_mi355x_merge_list *out)
{
    const CqtMergeParams P = {params.pic_width, params.pic_height, params.ctb_log2, params.min_cb_log2, params.max_cand, {params.ref_poc[0], params.ref_poc[1]}, {0, 0, 0, 0, 0}};
    hipLaunchKernelGGL(k_cqt_merge_lists, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, P, reinterpret_cast<const unsigned long long *>(cqtCells),
                       static_cast<const havoc_picture_pu *>(pus), n, reinterpret_cast<const unsigned long long *>(temporal), out);
    return hipGetLastError();
}

} // namespace havoc_gpu
