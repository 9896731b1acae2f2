// k_cu_close: closing an inter coding unit -- Search<IfCbf<rqt_root_cbf, transform_tree>>::go (turing/Search.hpp:2362-2568): the CU preamble's bits (cu_skip_flag,
// pred_mode_flag, part_mode, rqt_root_cbf: turing/SyntaxCtu.hpp:143-264, writers turing/Binarization.h:283-375), the skipped CU, and the comparison of the coded unit
// with the unit left at its prediction -- k_unit_pred_ssd: the ssdPrediction that comparison needs (turing/Reconstruct.cpp:856) -- and k_unit_pred_select: the
// winning candidate's prediction of every searched unit into the unit prediction planes.  DESIGN 7.
//
// k_cu_close's form is k_pu_rate's: a lane per candidate CU, sequential, 64-lane workgroups, the (state, bin) -> (state, rate) table of cabac_tables.h in LDS, the
// CU's 16 context bytes in two 64-bit registers.  Of the prediction-unit snapshot only merge_idx's byte is ever moved (the skip paths), so it is copied through.
//
// k_unit_pred_ssd's form: a wavefront per unit, four units per workgroup, no LDS.  The picture's units are 32x32 (96 row pieces of 8 bytes per lane-pass in luma
// alone) down to 8x8; a wavefront covers a 32x32 unit's three planes in three passes of 8-byte reads and closes with the DPP reduction of common.h.  A 16-lane group
// per unit would fill the lanes of an 8x8 unit (16 pieces) but walk a 64x64 unit in 48 passes per lane with a quarter of the loads in flight, and the units along a
// partial edge are few; one form for every size keeps the launch count at one.
#include "common.h"
#include "launch.h"
#include "cabac_tables.h"

namespace havoc_gpu {

namespace {

using CuCloseJob = havoc_mi355x_cu_close_job;
using CuChoice = havoc_mi355x_cu_choice;
using PredSsdJob = havoc_mi355x_pred_ssd_job;
using PredSelectJob = havoc_mi355x_pred_select_job;

static_assert(HAVOC_CU_SYNTAX_CTX_CU_SKIP_FLAG + 2 < 8 && HAVOC_CU_SYNTAX_CTX_PRED_MODE_FLAG < 8 && HAVOC_CU_SYNTAX_CTX_PART_MODE == 7 &&
              HAVOC_CU_SYNTAX_CTX_RQT_ROOT_CBF < 16 && HAVOC_CU_SYNTAX_CTX_BYTES == 16, "the snapshot is walked as two 64-bit words");

__global__ __launch_bounds__(64) void k_cu_close(const uint8_t *__restrict__ cuSyntax, const uint8_t *__restrict__ puBefore, const uint8_t *__restrict__ puAfter,
                                                 const int64_t *__restrict__ puRate, const havoc_mi355x_rqt_choice *__restrict__ choice,
                                                 const havoc_mi355x_rqt_tree_choice *__restrict__ treeChoice, const int64_t *__restrict__ treeRate,
                                                 const int32_t *__restrict__ predSsd, const CuCloseJob *__restrict__ jobs, int njobs, int maxNumMergeCand, int32_t lamQ16,
                                                 CuChoice *__restrict__ out, uint8_t *__restrict__ cuOut, uint8_t *__restrict__ puOut)
{
    __shared__ int bins[256];       // 2 state + bin -> new state | Q16 rate << 8
    const int lane = threadIdx.x, j = blockIdx.x * 64 + lane;
    for (int k = lane; k < 256; k += 64) bins[k] = bin_entry(k >> 1, k & 1);
    __syncthreads();
    if (j >= njobs) return;
    const CuCloseJob job = jobs[j];
    const uint64_t *in = reinterpret_cast<const uint64_t *>(cuSyntax) + 2 * (long)job.ctx_index;
    const uint64_t lo0 = in[0], hi0 = in[1];
    uint64_t lo = lo0, hi = hi0;        // bytes 0..7 and 8..15 of the CU snapshot
    auto priceIn = [&](uint64_t &v, int ctx, int bin) -> int {
        const int s = 8 * ctx, e = bins[2 * (int)(v >> s & 255) + bin];
        v = (v & ~(0xffull << s)) | (uint64_t)(e & 255) << s;
        return e >> 8;
    };
    auto price = [&](int ctx, int bin) -> int { return ctx < 8 ? priceIn(lo, ctx, bin) : priceIn(hi, ctx - 8, bin); };
    const uint64_t *pa = reinterpret_cast<const uint64_t *>(puAfter) + 2 * (long)job.pu_after_index;
    uint64_t puLo = pa[0], puHi = pa[1];
    const int pm = job.part_mode, log2 = job.log2_cb_size;
    const bool minCb = (job.flags & HAVOC_CU_CLOSE_MIN_CB) != 0, amp = (job.flags & HAVOC_CU_CLOSE_AMP) != 0, merged = (job.flags & HAVOC_CU_CLOSE_MERGE_2Nx2N) != 0;
    // a job the syntax cannot code is not walked
    bool valid = (job.flags & ~(HAVOC_CU_CLOSE_MIN_CB | HAVOC_CU_CLOSE_AMP | HAVOC_CU_CLOSE_MERGE_2Nx2N)) == 0 && job.skip_ctx_inc <= 2 && log2 >= 3 && log2 <= 6 &&
                 (log2 > 3 || minCb) && pm <= 7 && job.pu_rate_index >= 0;
    if (pm == 3) valid = valid && minCb && log2 > 3;
    if (pm >= 4) valid = valid && !minCb && amp;
    if (merged) valid = valid && pm == 0 && job.merge_idx < maxNumMergeCand;
    const int64_t ratePu = valid ? puRate[job.pu_rate_index] : -1;
    valid = valid && ratePu >= 0;
    const havoc_mi355x_rqt_choice *ch = choice + job.unit_index;
    const havoc_mi355x_rqt_tree_choice tc = treeChoice[job.unit_index];
    const bool zero = ch->depth == 0 && ch->tried_zero != 0;
    const bool haveResidual = (zero ? tc.mask_zero : tc.mask_one) != 0;
    const int64_t rateTree = valid && haveResidual ? treeRate[2 * (long)job.unit_index + (zero ? 0 : 1)] : 0;
    valid = valid && rateTree >= 0;
    CuChoice r = {HAVOC_CU_OUTCOME_REFUSED, 0, -1, -1, -1, -1, -1};
    if (valid)
    {
        const uint32_t ssdY = zero ? ch->zero.ssd : ch->one[0].ssd + ch->one[1].ssd + ch->one[2].ssd + ch->one[3].ssd;
        const int32_t ssd = (int32_t)(ssdY + (uint32_t)(zero ? tc.chroma_ssd_zero : tc.chroma_ssd_one));
        const int64_t distCoded = (int64_t)lamQ16 * ssd;
        // the skipped CU's two elements from the contexts before the CU: cu_skip_flag(1), merge_idx (TR, cMax = MaxNumMergeCand - 1, bin 0 context-coded)
        auto skipped = [&]() -> int64_t {
            lo = lo0, hi = hi0;
            const uint64_t *pb = reinterpret_cast<const uint64_t *>(puBefore) + 2 * (long)job.pu_before_index;
            puLo = pb[0], puHi = pb[1];
            int bits = 0, bypass = 0;
            if (maxNumMergeCand > 1)
            {
                bits += priceIn(puLo, HAVOC_PU_SYNTAX_CTX_MERGE_IDX, job.merge_idx > 0);
                bypass = job.merge_idx + (job.merge_idx < maxNumMergeCand - 1) - 1;
            }
            bits += price(HAVOC_CU_SYNTAX_CTX_CU_SKIP_FLAG + job.skip_ctx_inc, 1);
            return (int64_t)bits + ((int64_t)bypass << 16);
        };
        r.have_residual = haveResidual;
        if (!haveResidual && merged)
        {
            r.outcome = HAVOC_CU_OUTCOME_SKIPPED;
            r.rate = skipped();
            r.lambda_distortion = distCoded;
            r.cost_no_residual = r.rate + distCoded;
        }
        else
        {
            // the preamble of a CU that is not skipped
            int bits = price(HAVOC_CU_SYNTAX_CTX_CU_SKIP_FLAG + job.skip_ctx_inc, 0), bypass = 0;
            bits += price(HAVOC_CU_SYNTAX_CTX_PRED_MODE_FLAG, 0);
            bits += price(HAVOC_CU_SYNTAX_CTX_PART_MODE, pm == 0);
            if (pm != 0)
            {
                bits += price(HAVOC_CU_SYNTAX_CTX_PART_MODE + 1, ~pm >> 1 & 1);
                if (minCb)
                {
                    if (log2 > 3 && pm != 1) bits += price(HAVOC_CU_SYNTAX_CTX_PART_MODE + 2, ~pm >> 2 & 1);
                }
                else if (amp)
                {
                    bits += price(HAVOC_CU_SYNTAX_CTX_PART_MODE + 3, ~pm >> 2 & 1);
                    if (pm >= 4) bypass = 1;
                }
            }
            const int64_t ratePre = ratePu + bits + ((int64_t)bypass << 16);
            if (!haveResidual)
            {   // not merged: rqt_root_cbf(0), no tree
                r.outcome = HAVOC_CU_OUTCOME_NO_RESIDUAL;
                r.rate = ratePre + price(HAVOC_CU_SYNTAX_CTX_RQT_ROOT_CBF, 0);
                r.lambda_distortion = distCoded;
                r.cost_no_residual = r.rate + distCoded;
            }
            else
            {
                const uint64_t loPre = lo, hiPre = hi;      // `snapshot`: the state after the preamble
                const int64_t rateCoded = ratePre + (merged ? 0 : price(HAVOC_CU_SYNTAX_CTX_RQT_ROOT_CBF, 1)) + rateTree;
                const int32_t *sp = predSsd + 3 * (long)job.unit_index;
                const int64_t distPred = (int64_t)lamQ16 * sp[0] + (int64_t)lamQ16 * sp[1] + (int64_t)lamQ16 * sp[2];
                const uint64_t loCoded = lo, hiCoded = hi, puLoCoded = puLo, puHiCoded = puHi;
                int64_t rateNone;
                if (merged)
                    rateNone = skipped();
                else
                {
                    lo = loPre, hi = hiPre;
                    rateNone = ratePre + price(HAVOC_CU_SYNTAX_CTX_RQT_ROOT_CBF, 0);
                }
                r.cost_coded = rateCoded + distCoded;
                r.cost_no_residual = rateNone + distPred;
                if (r.cost_no_residual < r.cost_coded)
                {
                    r.outcome = merged ? HAVOC_CU_OUTCOME_SKIPPED : HAVOC_CU_OUTCOME_NO_RESIDUAL;
                    r.rate = rateNone;
                    r.lambda_distortion = distPred;
                }
                else
                {
                    r.outcome = HAVOC_CU_OUTCOME_CODED;
                    r.rate = rateCoded;
                    r.lambda_distortion = distCoded;
                    lo = loCoded, hi = hiCoded, puLo = puLoCoded, puHi = puHiCoded;
                }
            }
        }
        r.cost = r.rate + r.lambda_distortion;
    }
    out[j] = r;
    uint64_t *co = reinterpret_cast<uint64_t *>(cuOut) + 2 * (long)j, *po = reinterpret_cast<uint64_t *>(puOut) + 2 * (long)j;
    co[0] = lo;
    co[1] = hi;
    po[0] = puLo;
    po[1] = puHi;
}

// a wavefront per unit: the row pieces of the three planes go round the lanes (8 bytes each; a 4x4 block of 8-bit chroma has 4-byte rows), three unsigned dot
// instructions per dword (ssd_dword: mod 2^32, which is the wrapping int32 sum), one DPP reduction per plane
template <int S>
__global__ __launch_bounds__(256) void k_unit_pred_ssd(const char *__restrict__ srcY, long srcStride, const char *__restrict__ srcC, long srcStrideC,
                                                       const char *__restrict__ predY, long predStride, const char *__restrict__ predC, long predStrideC,
                                                       const PredSsdJob *__restrict__ jobs, int n, int32_t *__restrict__ out)
{
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;     // wave-uniform
    const PredSsdJob job = jobs[i];
#pragma unroll
    for (int c = 0; c < 3; ++c)
    {
        const int log2 = job.log2_size - (c > 0), rowBytes = S << log2;
        const char *a = (c ? srcC : srcY) + (long)job.src_off[c] * S, *b = (c ? predC : predY) + (long)job.pred_off[c] * S;
        const long sa = (c ? srcStrideC : srcStride) * S, sb = (c ? predStrideC : predStride) * S;
        uint32_t acc = 0;
        if (rowBytes >= 8)
        {
            const int lp = __builtin_ctz(rowBytes) - 3, items = (1 << log2) << lp;     // pieces per row (a power of two), pieces of the block
            for (int t = lane; t < items; t += 64)
            {
                const int y = t >> lp, x = (t & ((1 << lp) - 1)) * 8;
                const u32x2 va = ld8(a + y * sa + x), vb = ld8(b + y * sb + x);
                acc = ssd_dword<S>(va.x, vb.x, acc);
                acc = ssd_dword<S>(va.y, vb.y, acc);
            }
        }
        else if (lane < 4)      // 4 rows of 4 bytes
            acc = ssd_dword<S>(ld4(a + lane * sa), ld4(b + lane * sb), 0);
        const int sum = wave_sum((int)acc);
        if (lane == 0) out[3 * (long)i + c] = sum;
    }
}

// k_unit_pred_select: the prediction go2 leaves behind for reconstructInter -- the WINNER's (havoc_mi355x_pu_decide's d_best) of a unit's three candidates, copied
// out of the contiguous candidate blocks into the unit's place in a prediction plane, with the winner's rate and candidate index beside it.  k_unit_pred_ssd's form:
// a wavefront per unit, wave-uniform on `best`, the 8-byte row pieces of the three planes round the lanes (dword pieces for an 8-bit 4x4 chroma block).  A unit
// without a winner copies nothing.
template <int S>
__global__ __launch_bounds__(256) void k_unit_pred_select(const char *__restrict__ candY, const char *__restrict__ candC, char *__restrict__ dstY, long dstStride,
                                                          char *__restrict__ dstC, long dstStrideC, const int32_t *__restrict__ first, const int32_t *__restrict__ best,
                                                          const int64_t *__restrict__ rate, const PredSelectJob *__restrict__ jobs, int n,
                                                          int64_t *__restrict__ unitRate, int32_t *__restrict__ unitCand)
{
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;     // wave-uniform
    const PredSelectJob job = jobs[i];
    const int b = best[job.unit];
    const bool won = b >= 0 && b <= 2;     // wave-uniform; -1: the unit has no winner (a value outside 0..2 selects nothing either)
    if (lane == 0)
    {
        const int cand = won ? first[job.unit] + b : -1;
        unitCand[job.unit] = cand;
        unitRate[job.unit] = won ? rate[cand] : -1;
    }
    if (!won) return;
#pragma unroll
    for (int c = 0; c < 3; ++c)
    {
        const int log2 = job.log2_size - (c > 0), rowBytes = S << log2;
        const char *a = (c ? candC : candY) + ((long)job.cand_off[c] + ((long)b << 2 * log2)) * S;
        char *d = (c ? dstC : dstY) + (long)job.dst_off[c] * S;
        const long sd = (c ? dstStrideC : dstStride) * S;
        if (rowBytes >= 8)
        {
            const int lp = __builtin_ctz(rowBytes) - 3, items = (1 << log2) << lp;     // pieces per row (a power of two), pieces of the block
            for (int t = lane; t < items; t += 64)
            {
                const int y = t >> lp, x = (t & ((1 << lp) - 1)) * 8;
                st8(d + y * sd + x, ld8(a + (long)y * rowBytes + x));
            }
        }
        else if (lane < 4)      // 4 rows of 4 bytes
            st4(d + lane * sd, ld4(a + lane * 4));
    }
}

} // namespace

hipError_t launch_unit_pred_select(hipStream_t st, int S, const void *candY, const void *candC, void *dstY, long dstStride, void *dstC, long dstStrideC,
                                   const int32_t *first, const int32_t *best, const int64_t *rate, const PredSelectJob *jobs, int n, int64_t *unitRate, int32_t *unitCand)
{
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n + 3) / 4)), block(256);
    auto c = [](const void *p) { return static_cast<const char *>(p); };
    auto m = [](void *p) { return static_cast<char *>(p); };
    if (S == 1)
        hipLaunchKernelGGL(k_unit_pred_select<1>, grid, block, 0, st, c(candY), c(candC), m(dstY), dstStride, m(dstC), dstStrideC, first, best, rate, jobs, n, unitRate, unitCand);
    else
        hipLaunchKernelGGL(k_unit_pred_select<2>, grid, block, 0, st, c(candY), c(candC), m(dstY), dstStride, m(dstC), dstStrideC, first, best, rate, jobs, n, unitRate, unitCand);
    return hipGetLastError();
}

hipError_t launch_cu_close(hipStream_t st, const uint8_t *cuSyntax, const uint8_t *puBefore, const uint8_t *puAfter, const int64_t *puRate,
                           const havoc_mi355x_rqt_choice *choice, const havoc_mi355x_rqt_tree_choice *treeChoice, const int64_t *treeRate, const int32_t *predSsd,
                           const CuCloseJob *jobs, int njobs, int maxNumMergeCand, int32_t lamQ16, CuChoice *out, uint8_t *cuOut, uint8_t *puOut)
{
    if (njobs <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_cu_close, dim3((unsigned)((njobs + 63) / 64)), dim3(64), 0, st, cuSyntax, puBefore, puAfter, puRate, choice, treeChoice, treeRate, predSsd, jobs,
                       njobs, maxNumMergeCand, lamQ16, out, cuOut, puOut);
    return hipGetLastError();
}

hipError_t launch_unit_pred_ssd(hipStream_t st, int S, const void *srcY, long srcStride, const void *srcC, long srcStrideC, const void *predY, long predStride,
                                const void *predC, long predStrideC, const PredSsdJob *jobs, int n, int32_t *out)
{
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n + 3) / 4)), block(256);
    auto c = [](const void *p) { return static_cast<const char *>(p); };
    if (S == 1)
        hipLaunchKernelGGL(k_unit_pred_ssd<1>, grid, block, 0, st, c(srcY), srcStride, c(srcC), srcStrideC, c(predY), predStride, c(predC), predStrideC, jobs, n, out);
    else
        hipLaunchKernelGGL(k_unit_pred_ssd<2>, grid, block, 0, st, c(srcY), srcStride, c(srcC), srcStrideC, c(predY), predStride, c(predC), predStrideC, jobs, n, out);
    return hipGetLastError();
}

} // namespace havoc_gpu
