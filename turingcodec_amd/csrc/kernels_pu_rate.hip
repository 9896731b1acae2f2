// k_pu_rate: the bits measurePuCost measures for one candidate of a prediction unit -- Syntax<prediction_unit> under Measure<void> (turing/Search.hpp:1656-1706,
// turing/SyntaxCtu.hpp:267-314, 382-405) -- and k_pu_decide: go2's comparison of a unit's candidates (Search.hpp:1829-1902).  DESIGN 0 (the row after the transform-tree rates), 7.
//
// Reference: the writers of turing/Binarization.h:538-612 (merge_flag, merge_idx, inter_pred_idc) and :745-831 (mvd_coding's elements, mvp_lX_flag) measured by
// measureEncodeDecision (turing/Write.h:476-506); a bypass bin costs 1 << 16 (:559-567).  ref_idx_lX has NO writer in the reference (the generic
// Write<Element<V, ae>>, Binarization.h:52-59, asserts "not yet implemented" and writes nothing in a release build; the encoder runs with one reference per list):
// it is priced as the inverse of the reference's reader ReadRefIdx (turing/Read.h:1864-1888), which is H.265 9.3.4.2 -- truncated Rice with cMax =
// num_ref_idx_lX_active_minus1, bins 0 and 1 context-coded with ctxInc = binIdx, the rest bypass.
//
// Form: a lane per candidate, sequential, 64-lane workgroups, as the three kernels of kernels_residual_rate.hip.  The (state, bin) -> (state, rate)
// table of cabac_tables.h lies in LDS; a candidate's 16 context bytes live in two 64-bit registers from its first bin to its last: the contexts are shared between
// the lists (ref_idx_lX, abs_mvd_greater0_flag, abs_mvd_greater1_flag, mvp_lX_flag: turing/Cabac.h:112-126), so the walk is strictly in the syntax's order.
#include "common.h"
#include "launch.h"
#include "cabac_tables.h"

namespace havoc_gpu {

namespace {

using PuRateJob = havoc_mi355x_pu_rate_job;
using PuSlice = havoc_mi355x_pu_slice;

// every context that a dynamic index can reach (inter_pred_idc by cqtDepth, ref_idx by binIdx) lies where the code below looks for it
static_assert(HAVOC_PU_SYNTAX_CTX_INTER_PRED_IDC + 4 < 8 && HAVOC_PU_SYNTAX_CTX_REF_IDX == 7 && HAVOC_PU_SYNTAX_CTX_ABS_MVD_GREATER0 >= 8 &&
              HAVOC_PU_SYNTAX_CTX_MVP_FLAG < 16 && HAVOC_PU_SYNTAX_CTX_BYTES == 16, "the snapshot is walked as two 64-bit words");

// abs_mvd_minus2's bypass bins: EG1 (Binarization.h:767-798) of v >= 0: floor(log2(v + 2)) - 1 ones, a zero, floor(log2(v + 2)) suffix bits
__device__ __forceinline__ int eg1Bits(int v) { return 2 * (31 - __clz(v + 2)); }

__global__ __launch_bounds__(64) void k_pu_rate(const uint8_t *__restrict__ syntaxStates, const PuRateJob *__restrict__ jobs, int njobs, PuSlice sl,
                                                int64_t *__restrict__ rates, uint8_t *__restrict__ syntaxOut)
{
    __shared__ int bins[256];       // 2 state + bin -> new state | Q16 rate << 8
    const int lane = threadIdx.x, j = blockIdx.x * 64 + lane;
    for (int k = lane; k < 256; k += 64) bins[k] = bin_entry(k >> 1, k & 1);
    __syncthreads();
    if (j >= njobs) return;
    const PuRateJob job = jobs[j];
    const uint64_t *in = reinterpret_cast<const uint64_t *>(syntaxStates) + 2 * (long)job.ctx_index;
    uint64_t lo = in[0], hi = in[1];    // bytes 0..7 and 8..15 of the snapshot
    // measureEncodeDecision on context byte `ctx` of one half of the candidate's snapshot: the bin's Q16 rate, the context moved
    auto priceIn = [&](uint64_t &v, int ctx, int bin) -> int {
        const int s = 8 * ctx, e = bins[2 * (int)(v >> s & 255) + bin];
        v = (v & ~(0xffull << s)) | (uint64_t)(e & 255) << s;
        return e >> 8;
    };
    auto priceLo = [&](int ctx, int bin) -> int { return priceIn(lo, ctx, bin); };
    auto priceHi = [&](int ctx, int bin) -> int { return priceIn(hi, ctx - 8, bin); };
    const bool skip = (job.flags & HAVOC_PU_RATE_SKIP) != 0, merged = skip || (job.flags & HAVOC_PU_RATE_MERGE) != 0;
    const bool bSlice = sl.slice_b != 0, bi = job.pred == 2, small = job.w + job.h == 12;
    // a job the syntax cannot code is not walked: its rate becomes -1 and its snapshot passes through
    bool valid = (job.flags & ~(HAVOC_PU_RATE_MERGE | HAVOC_PU_RATE_SKIP)) == 0;
    if (merged)
        valid = valid && job.merge_idx < sl.max_num_merge_cand;
    else
    {
        valid = valid && job.pred <= 2 && job.cqt_depth <= 3 && !(bi && small) && (bSlice || job.pred == 0);
#pragma unroll
        for (int l = 0; l < 2; ++l)
            if (valid && job.pred != 1 - l) valid = job.mvp_flag[l] <= 1 && job.ref_idx[l] <= sl.num_ref_idx_active_minus1[l];
    }
    int64_t rate = -1;
    if (valid)
    {
        int bits = 0, bypass = 0;       // Q16 of the context-coded bins (at most 18 bins below 2^21 each), the number of bypass bins
        if (merged)
        {
            if (!skip) bits += priceLo(HAVOC_PU_SYNTAX_CTX_MERGE_FLAG, 1);
            if (sl.max_num_merge_cand > 1)
            {   // TR, cMax = MaxNumMergeCand - 1: merge_idx ones, a zero unless merge_idx == cMax; bin 0 context-coded
                bits += priceLo(HAVOC_PU_SYNTAX_CTX_MERGE_IDX, job.merge_idx > 0);
                bypass += job.merge_idx + (job.merge_idx < sl.max_num_merge_cand - 1) - 1;
            }
        }
        else
        {
            bits += priceLo(HAVOC_PU_SYNTAX_CTX_MERGE_FLAG, 0);
            if (bSlice)
            {
                if (!small) bits += priceLo(HAVOC_PU_SYNTAX_CTX_INTER_PRED_IDC + job.cqt_depth, bi);
                if (!bi) bits += priceLo(HAVOC_PU_SYNTAX_CTX_INTER_PRED_IDC + 4, job.pred);
            }
#pragma unroll
            for (int l = 0; l < 2; ++l)
            {
                if (job.pred == 1 - l) continue;
                const int cMax = sl.num_ref_idx_active_minus1[l], r = job.ref_idx[l];
                if (cMax > 0)
                {
                    const int n = r + (r < cMax);
                    bits += priceLo(HAVOC_PU_SYNTAX_CTX_REF_IDX, r > 0);
                    if (n > 1) bits += priceHi(HAVOC_PU_SYNTAX_CTX_REF_IDX + 1, r > 1);
                    if (n > 2) bypass += n - 2;
                }
                if (!(l == 1 && bi && sl.mvd_l1_zero_flag))
                {
                    const int ax = abs((int)job.mvd[l][0]), ay = abs((int)job.mvd[l][1]);
                    bits += priceHi(HAVOC_PU_SYNTAX_CTX_ABS_MVD_GREATER0, ax > 0);
                    bits += priceHi(HAVOC_PU_SYNTAX_CTX_ABS_MVD_GREATER0, ay > 0);
                    if (ax > 0) bits += priceHi(HAVOC_PU_SYNTAX_CTX_ABS_MVD_GREATER1, ax > 1);
                    if (ay > 0) bits += priceHi(HAVOC_PU_SYNTAX_CTX_ABS_MVD_GREATER1, ay > 1);
                    if (ax > 0) bypass += (ax > 1 ? eg1Bits(ax - 2) : 0) + 1;
                    if (ay > 0) bypass += (ay > 1 ? eg1Bits(ay - 2) : 0) + 1;
                }
                bits += priceHi(HAVOC_PU_SYNTAX_CTX_MVP_FLAG, job.mvp_flag[l]);
            }
        }
        rate = (int64_t)bits + ((int64_t)bypass << 16);
    }
    rates[job.out_index] = rate;
    if (syntaxOut != nullptr)
    {
        uint64_t *out = reinterpret_cast<uint64_t *>(syntaxOut) + 2 * (long)j;
        out[0] = lo;
        out[1] = hi;
    }
}

// go2's comparison (Search.hpp:1829-1842, 1883-1891) over the contiguous candidates of a unit, a lane per unit: cost = rate + (satdY + satdCb + satdCr) * lambda
// (measurePuCost, :1705: the sum in int32, FixedPoint<int32_t, 16> * int32_t -> int64, FixedPoint.h:79); a later candidate replaces the best only on cost < bestCost
__global__ __launch_bounds__(256) void k_pu_decide(const int32_t *__restrict__ first, const int32_t *__restrict__ count, int n, const int64_t *__restrict__ rates,
                                                   const int32_t *__restrict__ sy, const int32_t *__restrict__ scb, const int32_t *__restrict__ scr, int32_t lamQ16,
                                                   const uint8_t *__restrict__ syntaxAfter, int64_t *__restrict__ cost, int32_t *__restrict__ best,
                                                   int64_t *__restrict__ bestCost, uint8_t *__restrict__ bestSyntax)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int f = first[i], c = count[i];
    int64_t bc = 0;
    int b = -1;
    for (int k = 0; k < c; ++k)
    {
        const int t = f + k;
        const int64_t r = rates[t];
        const int64_t v = r < 0 ? -1 : r + (int64_t)(int32_t)((uint32_t)sy[t] + (uint32_t)scb[t] + (uint32_t)scr[t]) * lamQ16;
        cost[t] = v;
        if (r >= 0 && (b < 0 || v < bc)) { bc = v; b = k; }
    }
    best[i] = b;
    bestCost[i] = b < 0 ? -1 : bc;
    if (bestSyntax != nullptr)
    {
        uint64_t *out = reinterpret_cast<uint64_t *>(bestSyntax) + 2 * (long)i;
        const uint64_t *in = reinterpret_cast<const uint64_t *>(syntaxAfter) + 2 * (long)(f + (b < 0 ? 0 : b));
        out[0] = b < 0 ? 0 : in[0];
        out[1] = b < 0 ? 0 : in[1];
    }
}

} // namespace

hipError_t launch_pu_rate(hipStream_t st, const uint8_t *syntaxStates, const PuRateJob *jobs, int njobs, const PuSlice *slice, int64_t *rates, uint8_t *syntaxOut)
{
    if (njobs <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pu_rate, dim3((unsigned)((njobs + 63) / 64)), dim3(64), 0, st, syntaxStates, jobs, njobs, *slice, rates, syntaxOut);
    return hipGetLastError();
}

hipError_t launch_pu_decide(hipStream_t st, const int32_t *first, const int32_t *count, int n, const int64_t *rates, const int32_t *sy, const int32_t *scb,
                            const int32_t *scr, int32_t lamQ16, const uint8_t *syntaxAfter, int64_t *cost, int32_t *best, int64_t *bestCost, uint8_t *bestSyntax)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pu_decide, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, first, count, n, rates, sy, scb, scr, lamQ16, syntaxAfter, cost, best, bestCost,
                       bestSyntax);
    return hipGetLastError();
}

} // namespace havoc_gpu
