// k_residual_rate: the bits the reference's EstimateRate verb measures for one residual_coding, per transform block; k_intra_rate (below):
// the same walk -- ONE device function, walkBlock -- behind the mode and transform-tree bins of an intra candidate; k_tree_rate (last): the same walk over the
// Y, Cb and Cr blocks of an inter unit's whole transform_tree at one depth, with split_transform_flag, cbf_cb, cbf_cr and cbf_luma beside them.
//
// Reference: EncodeResidual::inner<havePopcnt, is4x4, H> with H::Tag == EstimateRate<void> (turing/EncodeResidual.hpp:36-301) over the coded data
// CodedData::storeResidual (turing/CodedData.h:457-517) packs from an n x n raster of levels; WriteLastSigPrefix / WriteLastSigSuffix
// (turing/Binarization.h:854-931), CtxIncSigCoeffFlagCalculator (turing/Write.h:1292-1392), the remaining-level estimate
// (turing/Binarization.h:1199-1238) and measureEncodeDecision (turing/Write.h:476-492).  The rate is a Cost (Q16, int64): a context-coded bin costs the Q15
// table entry shifted to Q16 and MOVES its context, a bypass bin costs 1 << 16; every bin is priced from the state the previous bins left.
//
// Form: a lane per job, sequential (the step is bound by vector-instruction issue and a lane-per-block walk beat a wavefront-parallel one for the
// quantiser that produces these levels).  A job is a chain of 1..4 blocks walked in order with the contexts running on -- the four depth-1 luma blocks of a unit --
// so the 128 context states of a job live in a column of the workgroup's LDS copy from its first bin to its last, beside the (state, bin) -> (state, rate)
// table of cabac_tables.h.  Per 4x4 sub-block, from the highest in scan order down: sixteen levels are loaded (four 8-byte rows) and kept in LDS by raster
// position; ONE pass over the scan positions 15..0 prices sig_coeff_flag, coeff_abs_level_greater1_flag (at most eight), the one coeff_abs_level_greater2_flag
// (inside the greater1 loop, as the EstimateRate tag does) and the bypass bins of coeff_abs_level_remaining: the three context families are disjoint and only
// the order WITHIN a context matters.  Sign bits are popcount(sig) - signHidden.  The `snake` word of coded-sub-block flags, greater1Ctx / lastGreater1Flag
// carried from the previously visited sub-block, countdown1 / countdown2 as a count of flags and "a greater1 was seen" are the reference's, restated.
#include "common.h"
#include "launch.h"
#include "cabac_tables.h"

namespace havoc_gpu {

namespace {

using RateJob = havoc_mi355x_residual_rate_job;
using IntraRateJob = havoc_mi355x_intra_rate_job;
using TreeRateJob = havoc_mi355x_tree_rate_job;

enum { kLastX = HAVOC_RDOQ_CTX_LAST_X, kLastY = HAVOC_RDOQ_CTX_LAST_Y, kCsbf = HAVOC_RDOQ_CTX_CSBF, kSig = HAVOC_RDOQ_CTX_SIG, kG1 = HAVOC_RDOQ_CTX_GREATER1,
       kG2 = HAVOC_RDOQ_CTX_GREATER2 };

// the 4x4 scan as 16 nibbles x | y << 2 (ScanOrder.h:31-97 for a 4x4 block)
__host__ __device__ constexpr uint64_t scanNibbles(int scanIdx)
{
    uint64_t v = 0;
    int i = 0;
    if (scanIdx == 0)
    {
        for (int d = 0; d < 7; ++d)
            for (int x = 0; x <= d; ++x)
                if (x < 4 && d - x < 4) { v |= (uint64_t)(x | (d - x) << 2) << (4 * i); ++i; }
    }
    else
        for (; i < 16; ++i) v |= (uint64_t)(scanIdx == 1 ? i : (i >> 2) | (i & 3) << 2) << (4 * i);
    return v;
}

// Write.h:1331-1355 ctxIdxMap[codedSubBlockFlags][raster position in the sub-block]
__device__ __forceinline__ int sigPattern(int neighbours, int xp, int yp)
{
    if (neighbours == 0) return xp + yp == 0 ? 2 : (xp + yp < 3 ? 1 : 0);
    if (neighbours == 1) return yp == 0 ? 2 : (yp == 1 ? 1 : 0);
    if (neighbours == 2) return xp == 0 ? 2 : (xp == 1 ? 1 : 0);
    return 2;
}

// Write.h:1284: groupIdx, the prefix of a last-significant coordinate
__device__ __forceinline__ int lastGroup(int c) { return c < 4 ? c : (c < 8 ? 4 + ((c - 4) >> 1) : (c < 16 ? 6 + ((c - 8) >> 2) : 8 + ((c - 16) >> 3))); }

struct RateLds
{
    int bins[256];              // 2 state + bin -> new state | Q16 rate << 8
    uint8_t st[128][64];        // the jobs' context states, [context][lane]
    int16_t lev[16][64];        // the current sub-block's levels, [raster position][lane]
    uint32_t cls[3][4];         // per scan and neighbour case: the scan positions whose sigPattern is 1 | those where it is 2, << 16
    uint8_t subXy[3][64];       // the diagonal scan of the sub-blocks of an 8x8, 16x16, 32x32 block: x | y << 4 (a kernel fills the rows of the sizes it walks)
    int32_t ctxIndex[64];
};

// the diagonal scan of one block size's sub-blocks (ScanOrder.h:31-59 applied to the GW x GW sub-blocks); a 4x4 block has one sub-block and no row
template <int LOG2>
__device__ __forceinline__ void subBlockScan(RateLds &sh, int lane)
{
    constexpr int GW = (1 << LOG2) / 4, NSUB = GW * GW;
    if (LOG2 >= 3 && lane < NSUB)
    {
        int pos = lane, x = 0, y = 0;
        for (int d = 0; d < 2 * GW - 1; ++d)
        {
            const int lo = d < GW ? 0 : d - GW + 1, hi = d < GW ? d : GW - 1, len = hi - lo + 1;
            if (pos < len) { x = lo + pos; y = d - x; break; }
            pos -= len;
        }
        sh.subXy[LOG2 >= 3 ? LOG2 - 3 : 0][lane] = (uint8_t)(x | y << 4);
    }
}

// the tables every walk reads: the (state, bin) table, the sig_coeff_flag classes per scan and neighbour case, the diagonal scan of the sub-blocks of the size LOG2
template <int LOG2>
__device__ __forceinline__ void rateTables(RateLds &sh, int lane)
{
    for (int k = lane; k < 256; k += 64) sh.bins[k] = bin_entry(k >> 1, k & 1);
    if (lane < 12)
    {
        const int t = lane >> 2, nb = lane & 3;
        const uint64_t sc = t == 0 ? scanNibbles(0) : (t == 1 ? scanNibbles(1) : scanNibbles(2));
        uint32_t one = 0, two = 0;
        for (int n = 0; n < 16; ++n)
        {
            const int nib = (int)(sc >> (4 * n)) & 15, p = sigPattern(nb, nib & 3, nib >> 2);
            one |= (uint32_t)(p == 1) << n;
            two |= (uint32_t)(p == 2) << n;
        }
        sh.cls[t][nb] = one | two << 16;
    }
    subBlockScan<LOG2>(sh, lane);
}

// the workgroup's 64 snapshots into sh.st, transposed (sh.ctxIndex filled and a barrier passed before; one follows)
__device__ __forceinline__ void loadStates(RateLds &sh, int lane, const uint8_t *__restrict__ states)
{
    for (int k = 0; k < 128; ++k)
    {   // 64 consecutive bytes of a snapshot per step
        const int idx = k * 64 + lane, jj = idx >> 7, byte = idx & 127, ci = sh.ctxIndex[jj];
        if (ci >= 0) sh.st[byte][jj] = states[(long)ci * 128 + byte];
    }
}

// ... and back: job first + jj's snapshot as its walk left it (a barrier passed before)
__device__ __forceinline__ void storeStates(const RateLds &sh, int lane, int first, int njobs, uint8_t *__restrict__ statesOut)
{
    for (int k = 0; k < 128; ++k)
    {
        const int idx = k * 64 + lane, jj = idx >> 7, byte = idx & 127;
        if (first + jj < njobs) statesOut[(long)(first + jj) * 128 + byte] = sh.st[byte][jj];
    }
}

// measureEncodeDecision on the lane's column: the bin's Q16 rate, the context moved
__device__ __forceinline__ int priceBin(RateLds &sh, int lane, int ctx, int bin)
{
    const int e = sh.bins[2 * sh.st[ctx][lane] + bin];
    sh.st[ctx][lane] = (uint8_t)e;
    return e >> 8;
}

// ONE residual_coding: the walk of a block's sub-blocks from the lane's states, which it moves -> its Q16 rate; coded = the block has a level (an all-zero
// block: IfCbf skips it, rate 0, no context touched).  All three kernels of this file call it.
template <int LOG2>
__device__ __forceinline__ int64_t walkBlock(RateLds &sh, int lane, const int16_t *__restrict__ src, int cIdx, int scanIdx, int sdh, bool &coded)
{
    constexpr int N = 1 << LOG2, GW = N / 4, NSUB = GW * GW;
    auto price = [&](int ctx, int bin) -> int { return priceBin(sh, lane, ctx, bin); };
    const uint64_t scan4 = scanIdx == 0 ? scanNibbles(0) : (scanIdx == 1 ? scanNibbles(1) : scanNibbles(2));
    int64_t rate = 0;
    bool seen = false;                       // the last significant sub-block has been met
    int lastG1 = 1, c1 = -1;                 // lastGreater1Flag, greater1Ctx (EncodeResidual.hpp:83-84)
    uint32_t snake = 0;
    for (int i = NSUB - 1; i >= 0; --i)
    {
        int xS = 0, yS = 0;
        if (GW > 1)
        {
            if (scanIdx == 1) { xS = i & (GW - 1); yS = i / GW; }
            else if (scanIdx == 2) { xS = i / GW; yS = i & (GW - 1); }
            else { const int p = sh.subXy[LOG2 >= 3 ? LOG2 - 3 : 0][i]; xS = p & 15; yS = p >> 4; }
        }
        const int16_t *sb = src + (yS * 4) * N + xS * 4;
        uint32_t any = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
        {
            const uint2 w = *reinterpret_cast<const uint2 *>(sb + r * N);
            any |= w.x | w.y;
            sh.lev[4 * r + 0][lane] = (int16_t)(w.x & 0xffff);
            sh.lev[4 * r + 1][lane] = (int16_t)(w.x >> 16);
            sh.lev[4 * r + 2][lane] = (int16_t)(w.y & 0xffff);
            sh.lev[4 * r + 3][lane] = (int16_t)(w.y >> 16);
        }
        const bool codedSb = any != 0;
        if (!seen && !codedSb) continue;       // above the last significant sub-block: nothing is coded
        const bool isLast = !seen;
        // sig: bit n = scan position n is significant; mag: CodedData's values (`value = -value` in int16: -32768 stays negative, so it is no greater1)
        uint32_t sig = 0;
        if (codedSb)
#pragma unroll
            for (int n = 0; n < 16; ++n) sig |= (uint32_t)(sh.lev[(int)(scan4 >> (4 * n)) & 15][lane] != 0) << n;
        int ctxBits = 0, bypass = 0;
        int lastPos = 16;                    // sig flags are priced below this scan position
        if (isLast)
        {
            seen = true;
            lastPos = 31 - __clz(sig);
            const int nib = (int)(scan4 >> (4 * lastPos)) & 15, xC = (xS << 2) + (nib & 3), yC = (yS << 2) + (nib >> 2);
            // last_sig_coeff_{x,y}_prefix: truncated unary, cMax = 2 log2 - 1 (Binarization.h:854-899); the suffix is bypass; scanIdx 2 swaps x and y
            const int ctxOffset = cIdx ? 15 : 3 * (LOG2 - 2) + ((LOG2 - 1) >> 2), ctxShift = cIdx ? LOG2 - 2 : (LOG2 + 1) >> 2, cMax = 2 * LOG2 - 1;
            for (int c = 0; c < 2; ++c)
            {
                const int v = (c == 0) == (scanIdx != 2) ? xC : yC, prefix = lastGroup(v), base = c == 0 ? kLastX : kLastY;
                for (int b = 0; b < prefix; ++b) ctxBits += price(base + ctxOffset + (b >> ctxShift), 1);
                if (prefix < cMax) ctxBits += price(base + ctxOffset + (prefix >> ctxShift), 0);
                if (prefix > 3) bypass += (prefix >> 1) - 1;
            }
        }
        const int d = 7 + yS - xS, neighbours = (int)(snake >> d) & 3;      // EncodeResidual.hpp:98-102
        snake &= ~(3u << d);
        if (codedSb) snake |= 3u << d;
        bool infer = false;
        if (!isLast && i != 0)
        {
            ctxBits += price(kCsbf + (cIdx ? 2 : 0) + (neighbours ? 1 : 0), codedSb);
            infer = true;
        }
        if (codedSb || i == 0)
        {
            if (sig & 0xfffe) infer = false;
            // sig_coeff_flag's context (Write.h:1292-1392)
            const uint32_t cls = sh.cls[scanIdx][neighbours];
            int sigBase;
            if (LOG2 == 2) sigBase = 0;
            else if (cIdx == 0) sigBase = (i != 0 ? 3 : 0) + (LOG2 == 3 ? (scanIdx == 0 ? 9 : 15) : 21);
            else sigBase = LOG2 == 3 ? 9 : 12;
            const int ctxSet = ((i != 0 && cIdx == 0) ? 2 : 0) | (((c1 > 0 && lastG1) || c1 == 0) ? 1 : 0);
            c1 = 1;
            const int g1Base = kG1 + ctxSet * 4 + (cIdx ? 16 : 0);
            int numG1 = 0, rice = 0;
            bool g2Done = false, sawG1 = false;
            for (int n = 15; n >= 0; --n)
            {
                const int s = (int)(sig >> n) & 1;
                if (n < lastPos && !(n == 0 && infer))
                {
                    int inc;
                    if (LOG2 == 2) inc = (int)(0x8877886654325410ull >> (4 * ((int)(scan4 >> (4 * n)) & 15))) & 15;      // 0 1 4 5 / 2 3 4 5 / 6 6 8 8 / 7 7 8 8
                    else if (i == 0 && n == 0) inc = 0;
                    else inc = sigBase + ((int)(cls >> n) & 1) + 2 * ((int)(cls >> (16 + n)) & 1);
                    ctxBits += price(kSig + (cIdx ? 27 : 0) + inc, s);
                }
                if (!s) continue;
                const int v = sh.lev[(int)(scan4 >> (4 * n)) & 15][lane];
                const int mag = v < 0 ? (int)(int16_t)(-v) : v;
                const int g1 = mag > 1;
                // the base level: 3 while the first eight flags run and no greater1 was seen, then 2; 1 from the ninth (countdown1 / countdown2, :265-283)
                const int base = numG1 < 8 ? (sawG1 ? 2 : 3) : 1;
                if (numG1 < 8)
                {
                    ctxBits += price(g1Base + c1, g1);
                    if (c1 > 0) lastG1 = g1;
                    if (g1 && !g2Done)
                    {
                        g2Done = true;
                        ctxBits += price(kG2 + ctxSet + (cIdx ? 4 : 0), mag > 2);
                    }
                    if (++numG1 < 8)      // (the reference breaks out of the loop at the eighth flag before it moves greater1Ctx)
                    {
                        if (lastG1) c1 = 0;
                        else if (c1 < 3) ++c1;
                    }
                }
                else
                    ++numG1;
                sawG1 |= g1 != 0;
                const int absCoeff = g1 ? (mag & 0xffff) : 1, remaining = absCoeff - base;
                if (remaining >= 0)
                {   // Binarization.h:1205-1237
                    const int a = (remaining >> rice) - 3;
                    bypass += rice + 4 + (a < 0 ? a : 2 * (31 - __clz(a + 1)));
                    rice = min(rice + (absCoeff > (3 << rice) ? 1 : 0), 4);
                }
            }
            // coeff_sign_flag: whole bits, one less when the sign of the first coefficient is hidden (:190-249)
            int signBits = __popc(sig);
            if (sdh && (sig & 0xfff8) && (31 - __clz(sig)) - (__ffs(sig) - 1) > 3) --signBits;
            bypass += signBits;
        }
        rate += (int64_t)ctxBits + ((int64_t)bypass << 16);
    }
    coded = seen;
    return rate;
}

template <int LOG2>
__global__ __launch_bounds__(64) void k_residual_rate(const int16_t *__restrict__ levels, const uint8_t *__restrict__ states, const RateJob *__restrict__ jobs, int njobs,
                                                      int64_t *__restrict__ rates, uint8_t *__restrict__ statesOut)
{
    constexpr int N = 1 << LOG2;
    __shared__ RateLds sh;
    const int lane = threadIdx.x, first = blockIdx.x * 64, j = first + lane;
    rateTables<LOG2>(sh, lane);
    RateJob job = RateJob();
    if (j < njobs) job = jobs[j];
    // a job the entry point excludes is not walked: its rates become -1 and its snapshot passes through
    const bool valid = j < njobs && job.count >= 1 && job.count <= 4 && job.c_idx <= 2 && job.scan_idx <= 2 && (job.scan_idx == 0 || LOG2 <= 3) && (job.c_idx == 0 || LOG2 <= 4);
    sh.ctxIndex[lane] = j < njobs ? job.ctx_index : -1;
    __syncthreads();
    loadStates(sh, lane, states);
    __syncthreads();
    const int blocks = valid ? job.count : 0;
    for (int blk = 0; blk < blocks; ++blk)
    {
        bool coded;
        rates[(long)job.rate_index + blk] = walkBlock<LOG2>(sh, lane, levels + (long)job.level_off + (long)blk * (N * N), job.c_idx, job.scan_idx, job.sdh, coded);
    }
    if (j < njobs && !valid)
    {
        const int c = job.count < 1 ? 1 : (job.count > 4 ? 4 : job.count);
        for (int blk = 0; blk < c; ++blk) rates[(long)job.rate_index + blk] = -1;
    }
    if (statesOut == nullptr) return;
    __syncthreads();
    storeStates(sh, lane, first, njobs, statesOut);
}

// k_intra_rate: what EstimateRateLuma measures for one refined intra candidate "since the partition began" (Search.hpp:199, 242-246; Syntax<IntraPartition>,
// SyntaxCtu.hpp:704-722), one candidate per lane in k_residual_rate's form: prev_intra_luma_pred_flag (Binarization.h:395-452, ctxInc 0), mpm_idx (TR, cMax 2,
// bypass: 1 or 2 bits) or rem_intra_luma_pred_mode (5 bypass bits), split_transform_flag = 0 where transform_tree codes it (ctxInc = 5 - log2,
// Binarization.h:617-634), cbf_luma (ctxInc = trafoDepth == 0, :637-651; cbf_cb / cbf_cr are priced as nothing, EstimateRate.h:114-119) and the block's
// residual_coding.  The two syntax contexts outside the 128-byte snapshot travel in 4 bytes of their own per job.  cbf_luma is priced AFTER the walk, which tells
// whether the block has a level without a second pass over it: no bin of the walk reads cbf_luma's context or the other way round, so the sum and every state are
// those of the syntax's order.
struct IntraRateLds
{
    RateLds r;
    uint8_t syn[HAVOC_INTRA_SYNTAX_CTX_BYTES][64];      // [context][lane]
};

template <int LOG2>
__global__ __launch_bounds__(64) void k_intra_rate(const int16_t *__restrict__ levels, const uint8_t *__restrict__ states, const uint8_t *__restrict__ syntaxStates,
                                                   const IntraRateJob *__restrict__ jobs, int njobs, int64_t *__restrict__ rates, uint8_t *__restrict__ statesOut,
                                                   uint8_t *__restrict__ syntaxOut)
{
    __shared__ IntraRateLds sh;
    const int lane = threadIdx.x, first = blockIdx.x * 64, j = first + lane;
    rateTables<LOG2>(sh.r, lane);
    IntraRateJob job = IntraRateJob();
    if (j < njobs) job = jobs[j];
    const bool splitCoded = (job.flags & HAVOC_INTRA_RATE_SPLIT_FLAG_CODED) != 0;
    // a job the entry point excludes is not walked: its rate becomes -1 and its snapshots pass through
    const bool valid = j < njobs && job.mpm_idx <= 3 && job.scan_idx <= 2 && (job.scan_idx == 0 || LOG2 <= 3) && !(splitCoded && LOG2 == 2);
    sh.r.ctxIndex[lane] = j < njobs ? job.ctx_index : -1;
    if (j < njobs)
        for (int b = 0; b < HAVOC_INTRA_SYNTAX_CTX_BYTES; ++b) sh.syn[b][lane] = syntaxStates[(long)job.ctx_index * HAVOC_INTRA_SYNTAX_CTX_BYTES + b];
    __syncthreads();
    loadStates(sh.r, lane, states);
    __syncthreads();
    if (valid)
    {
        auto priceSyntax = [&](int ctx, int bin) -> int {
            const int e = sh.r.bins[2 * sh.syn[ctx][lane] + bin];
            sh.syn[ctx][lane] = (uint8_t)e;
            return e >> 8;
        };
        const bool mpm = job.mpm_idx < 3;
        int64_t rate = priceSyntax(HAVOC_INTRA_SYNTAX_CTX_PREV_INTRA_LUMA_PRED_FLAG, mpm);
        rate += (int64_t)(mpm ? (job.mpm_idx == 0 ? 1 : 2) : 5) << 16;
        if (splitCoded) rate += priceSyntax(HAVOC_INTRA_SYNTAX_CTX_SPLIT_TRANSFORM_FLAG + 5 - LOG2, 0);
        bool coded;
        rate += walkBlock<LOG2>(sh.r, lane, levels + (long)job.level_off, 0, job.scan_idx, job.sdh, coded);
        rate += priceBin(sh.r, lane, HAVOC_RDOQ_CTX_CBF_LUMA + ((job.flags & HAVOC_INTRA_RATE_DEPTH_NONZERO) ? 0 : 1), coded);
        rates[job.rate_index] = rate;
    }
    else if (j < njobs)
        rates[job.rate_index] = -1;
    if (syntaxOut != nullptr && j < njobs)
        for (int b = 0; b < HAVOC_INTRA_SYNTAX_CTX_BYTES; ++b) syntaxOut[(long)j * HAVOC_INTRA_SYNTAX_CTX_BYTES + b] = sh.syn[b][lane];
    if (statesOut == nullptr) return;
    __syncthreads();
    storeStates(sh.r, lane, first, njobs, statesOut);
}

// k_tree_rate: what the inter transform-tree decision measures per depth (turing/Reconstruct.cpp:1296-1428: EstimateRate<void> over `if (rqt_root_cbf) transform_tree`),
// one candidate tree of one unit per lane in the form of the two kernels above; one launch per (log2CbSize L, depth), so that every lane of a launch walks the same
// sequence of block sizes.  Syntax<transform_tree> (turing/SyntaxCtu.hpp:329-379) and Syntax<transform_unit> (:411-502) with MaxTrafoDepth 1, 4:2:0, scanIdx 0:
//   depth 0: split_transform_flag = 0, cbf_cb, cbf_cr (both ctxInc 0), cbf_luma (ctxInc 1) only when cbf_cb || cbf_cr, then Y (log2 L), Cb, Cr (log2 max(L - 1, 2));
//   depth 1: split_transform_flag = 1, the parent's cbf_cb, cbf_cr (ctxInc 0: the OR of the children's), then per child in z-order cbf_cb / cbf_cr (ctxInc 1, L > 3 and
//            the parent's flag set), cbf_luma (ctxInc 0, always), Y (log2 L - 1), and Cb, Cr (log2 L - 2) -- for L == 3 the parent's one 4x4 Cb and Cr after child 3.
// The residual blocks are walked FIRST, in the syntax's order (Cb and Cr share the chroma residual contexts: Cb0 Cr0 Cb1 Cr1 ...), which tells every cbf without a
// second pass; the flag bins are priced after them, in the syntax's order among themselves (cbf_cb and cbf_cr share contexts).  The flag contexts, the luma and the
// chroma residual contexts are pairwise disjoint, so the sum and every state are those of the interleaved syntax.  A tree without a level is not coded at all
// (rqt_root_cbf = 0, itself not priced): rate 0, nothing moved.  The alternative form -- luma chain, chroma chain and flags on separate lanes, summed -- was not built.
// L == 6 exists at depth 1 only: a 64x64 unit lies above MaxTbLog2SizeY, so its split is inferred (Reconstruct.cpp:1300-1310) and the walk is depth 1's without the
// split_transform_flag bin -- four 32x32 Y and four 16x16 Cb and Cr blocks.  A job of it that claims the bin is coded names an impossible flag value and is refused.
template <int L, int DEPTH>
__global__ __launch_bounds__(64) void k_tree_rate(const int16_t *__restrict__ lumaLevels, const int16_t *__restrict__ chromaLevels, const uint8_t *__restrict__ states,
                                                  const uint8_t *__restrict__ syntaxStates, const TreeRateJob *__restrict__ jobs, int njobs, int64_t *__restrict__ rates,
                                                  uint32_t *__restrict__ cbfMasks, uint8_t *__restrict__ statesOut, uint8_t *__restrict__ syntaxOut)
{
    constexpr int LY = L - DEPTH, LC = (L == 3 ? 2 : L - 1 - DEPTH);      // the luma and chroma transform sizes of the depth
    constexpr int NY = DEPTH ? 4 : 1, NC = (DEPTH && L > 3) ? 4 : 1;      // how many blocks of each
    __shared__ IntraRateLds sh;
    const int lane = threadIdx.x, first = blockIdx.x * 64, j = first + lane;
    rateTables<LY>(sh.r, lane);
    subBlockScan<LC>(sh.r, lane);
    TreeRateJob job = TreeRateJob();
    if (j < njobs) job = jobs[j];
    // a job with a flag bit this kernel does not know is not walked: its rate becomes -1, its mask 0 and its snapshots pass through
    // (for L == 6, whose split is inferred, HAVOC_TREE_RATE_SPLIT_FLAG_CODED is such a bit)
    const bool valid = j < njobs && (job.flags & ~(L <= 5 ? HAVOC_TREE_RATE_SPLIT_FLAG_CODED : 0)) == 0;
    sh.r.ctxIndex[lane] = j < njobs ? job.ctx_index : -1;
    if (j < njobs)
        for (int b = 0; b < HAVOC_INTRA_SYNTAX_CTX_BYTES; ++b) sh.syn[b][lane] = syntaxStates[(long)job.ctx_index * HAVOC_INTRA_SYNTAX_CTX_BYTES + b];
    __syncthreads();
    loadStates(sh.r, lane, states);
    __syncthreads();
    if (valid)
    {
        int64_t rate = 0;
        uint32_t mask = 0;
        bool coded;
#pragma unroll 1
        for (int k = 0; k < NY; ++k)
        {
            rate += walkBlock<LY>(sh.r, lane, lumaLevels + (long)job.luma_off + (long)k * (1 << 2 * LY), 0, 0, job.sdh, coded);
            mask |= (uint32_t)coded << k;
            if (NC == NY || k == NY - 1)
            {
                const int kc = NC == NY ? k : 0;
                rate += walkBlock<LC>(sh.r, lane, chromaLevels + (long)job.cb_off + (long)kc * (1 << 2 * LC), 1, 0, job.sdh, coded);
                mask |= (uint32_t)coded << (4 + kc);
                rate += walkBlock<LC>(sh.r, lane, chromaLevels + (long)job.cr_off + (long)kc * (1 << 2 * LC), 2, 0, job.sdh, coded);
                mask |= (uint32_t)coded << (8 + kc);
            }
        }
        if (mask != 0)
        {
            const int cb = (mask & 0x0f0) != 0, cr = (mask & 0xf00) != 0;
            if (L <= 5 && (job.flags & HAVOC_TREE_RATE_SPLIT_FLAG_CODED))
            {
                const int ctx = HAVOC_INTRA_SYNTAX_CTX_SPLIT_TRANSFORM_FLAG + (L <= 5 ? 5 - L : 0), e = sh.r.bins[2 * sh.syn[ctx][lane] + DEPTH];
                sh.syn[ctx][lane] = (uint8_t)e;
                rate += e >> 8;
            }
            rate += priceBin(sh.r, lane, HAVOC_RDOQ_CTX_CBF_CHROMA, cb);
            rate += priceBin(sh.r, lane, HAVOC_RDOQ_CTX_CBF_CHROMA, cr);
            if (DEPTH == 0)
            {
                if (cb || cr) rate += priceBin(sh.r, lane, HAVOC_RDOQ_CTX_CBF_LUMA + 1, (int)(mask & 1));
            }
            else
                for (int k = 0; k < 4; ++k)
                {
                    if (NC == 4 && cb) rate += priceBin(sh.r, lane, HAVOC_RDOQ_CTX_CBF_CHROMA + 1, (int)(mask >> (4 + k)) & 1);
                    if (NC == 4 && cr) rate += priceBin(sh.r, lane, HAVOC_RDOQ_CTX_CBF_CHROMA + 1, (int)(mask >> (8 + k)) & 1);
                    rate += priceBin(sh.r, lane, HAVOC_RDOQ_CTX_CBF_LUMA, (int)(mask >> k) & 1);
                }
        }
        rates[job.out_index] = rate;
        cbfMasks[job.out_index] = mask;
    }
    else if (j < njobs)
    {
        rates[job.out_index] = -1;
        cbfMasks[job.out_index] = 0;
    }
    if (syntaxOut != nullptr && j < njobs)
        for (int b = 0; b < HAVOC_INTRA_SYNTAX_CTX_BYTES; ++b) syntaxOut[(long)j * HAVOC_INTRA_SYNTAX_CTX_BYTES + b] = sh.syn[b][lane];
    if (statesOut == nullptr) return;
    __syncthreads();
    storeStates(sh.r, lane, first, njobs, statesOut);
}

} // namespace

hipError_t launch_tree_rate(hipStream_t st, int log2Cb, int depth, const int16_t *lumaLevels, const int16_t *chromaLevels, const uint8_t *states, const uint8_t *syntaxStates,
                            const TreeRateJob *j, int njobs, int64_t *rates, uint32_t *cbf, uint8_t *statesOut, uint8_t *syntaxOut)
{
    if (njobs <= 0) return hipSuccess;
    const dim3 grid((njobs + 63) / 64), wg(64);
#define TREE_RATE(L, D) hipLaunchKernelGGL((k_tree_rate<L, D>), grid, wg, 0, st, lumaLevels, chromaLevels, states, syntaxStates, j, njobs, rates, cbf, statesOut, syntaxOut)
    if (log2Cb == 3 && depth == 0) TREE_RATE(3, 0);
    else if (log2Cb == 3 && depth == 1) TREE_RATE(3, 1);
    else if (log2Cb == 4 && depth == 0) TREE_RATE(4, 0);
    else if (log2Cb == 4 && depth == 1) TREE_RATE(4, 1);
    else if (log2Cb == 5 && depth == 0) TREE_RATE(5, 0);
    else if (log2Cb == 5 && depth == 1) TREE_RATE(5, 1);
    else if (log2Cb == 6 && depth == 1) TREE_RATE(6, 1);
    else return hipErrorInvalidValue;
#undef TREE_RATE
    return hipGetLastError();
}

hipError_t launch_intra_rate(hipStream_t st, int log2, const int16_t *levels, const uint8_t *states, const uint8_t *syntaxStates, const IntraRateJob *j, int njobs,
                             int64_t *rates, uint8_t *statesOut, uint8_t *syntaxOut)
{
    if (njobs <= 0) return hipSuccess;
    const dim3 grid((njobs + 63) / 64), wg(64);
    if (log2 == 2) hipLaunchKernelGGL(k_intra_rate<2>, grid, wg, 0, st, levels, states, syntaxStates, j, njobs, rates, statesOut, syntaxOut);
    else if (log2 == 3) hipLaunchKernelGGL(k_intra_rate<3>, grid, wg, 0, st, levels, states, syntaxStates, j, njobs, rates, statesOut, syntaxOut);
    else if (log2 == 4) hipLaunchKernelGGL(k_intra_rate<4>, grid, wg, 0, st, levels, states, syntaxStates, j, njobs, rates, statesOut, syntaxOut);
    else if (log2 == 5) hipLaunchKernelGGL(k_intra_rate<5>, grid, wg, 0, st, levels, states, syntaxStates, j, njobs, rates, statesOut, syntaxOut);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_residual_rate(hipStream_t st, int log2, const int16_t *levels, const uint8_t *states, const RateJob *j, int njobs, int64_t *rates, uint8_t *statesOut)
{
    if (njobs <= 0) return hipSuccess;
    const dim3 grid((njobs + 63) / 64), wg(64);
    if (log2 == 2) hipLaunchKernelGGL(k_residual_rate<2>, grid, wg, 0, st, levels, states, j, njobs, rates, statesOut);
    else if (log2 == 3) hipLaunchKernelGGL(k_residual_rate<3>, grid, wg, 0, st, levels, states, j, njobs, rates, statesOut);
    else if (log2 == 4) hipLaunchKernelGGL(k_residual_rate<4>, grid, wg, 0, st, levels, states, j, njobs, rates, statesOut);
    else if (log2 == 5) hipLaunchKernelGGL(k_residual_rate<5>, grid, wg, 0, st, levels, states, j, njobs, rates, statesOut);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

} // namespace havoc_gpu
