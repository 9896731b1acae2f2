// Inter prediction written to memory: HEVC 8-tap (luma) / 4-tap (chroma) fractional-sample interpolation, uni and bi
// (havoc/pred_inter.h:35,63; C reference havoc/pred_inter.cpp:76-202, 1207-1252), and the bi-search helper SubtractBi.
//
// Same two-phase structure as the sub-pel candidate kernel (kernels_subpel.hip):
//   1. horizontal pass straight from HBM/L2 with dot4 / dot2 (interp.h, hfilter4), transposed into LDS (tmp[x][y]);
//      bi-prediction does it for both references;
//   2. one column of 8 outputs per lane: two ds_read_b128 fetch the column's intermediates, the vertical filter is
//      four v_dot2_i32_i16 per output; uni: round, shift, clip; bi: the two 14-bit intermediates are averaged with
//      rounding and clipped (havoc_pred_bi_mean_c_ref).  The column goes to an LDS output tile;
//   3. the output tile is written row-wise, 4 samples per lane (coalesced, exactly w x h samples: the reference JIT's
//      licence to write to the right of the block, havoc/pred_inter.h:27, is not used).
// All phase combinations take the two-pass route (zero phase = the {..,64,..} filter), bit-identical to the
// reference's copy / one-pass forms for bit depths 8..10.  A launch is uniform in a size class (max_w x max_h), as
// the reference's table is indexed by width class: G = 8 / 32 / 128 / 256 lanes per block, 256 / G blocks per
// workgroup.
//
// That is the FULL form, kept for widths that are no multiple of four and as the other arm of HAVOC_PRED_LEAN=0.  Every other job takes the LEAN form
// (pred_workgroup_lean): a lane of the horizontal pass owns a quad of columns and walks its rows two at a time (no division, one 32-bit LDS store per column
// and row pair), the vertical pass hands its column's eight results to the quad's lanes through DPP and stores whole rows straight to the destination (no
// output tile, no second barrier, no third phase), and in the classes where a wavefront serves one job (32, 64) a zero phase is not filtered.  A workgroup
// takes one form for all its jobs, so that no barrier sits under a divergent branch.
#include <stdlib.h>

#include "common.h"
#include "launch.h"
#include "interp.h"

namespace havoc_gpu {

// LDS of one workgroup of a size class: intermediates [JPW][NREF][MAXW * TH + 8] int16, then the output tiles [JPW][MAXH * OS + 2] uint16
template <int MAXW, int MAXH, int G, bool BI>
struct PredLds
{
    static constexpr int JPW = 256 / G, NREF = BI ? 2 : 1, TH = MAXH + 8, OS = MAXW + 2;
    static constexpr int tmpElems = MAXW * TH + 8, outElems = MAXH * OS + 2;
    static constexpr int tmpBytes = ((JPW * NREF * tmpElems * 2) + 15) & ~15;
    static constexpr int bytes = tmpBytes + ((JPW * outElems * 2 + 15) & ~15);
};

// one workgroup's share of a size class: workgroup `wg` of `wgs`, job table of `njobs` jobs of that class
template <int S, int TAPS, int MAXW, int MAXH, int G, bool BI>
__device__ __forceinline__ void pred_workgroup_full(char *lds, char *__restrict__ dst, long stride_dst, const char *__restrict__ ref, long stride_ref,
                                                    const int32_t *__restrict__ jobs, int njobs, int bitDepth, int wg, int wgs)
{
    typedef typename Sample<S>::T T;
    typedef PredLds<MAXW, MAXH, G, BI> L;
    constexpr int JPW = 256 / G;
    constexpr int NREF = BI ? 2 : 1;
    constexpr int AB = TAPS / 2 - 1;
    constexpr int TH = MAXH + 8;     // intermediate column: h + TAPS - 1 <= MAXH + 7, rounded up to 8
    constexpr int OS = MAXW + 2;     // output tile row stride (samples), skewed against bank conflicts
    int16_t (*s_tmp)[NREF][L::tmpElems] = reinterpret_cast<int16_t (*)[NREF][L::tmpElems]>(lds);
    uint16_t (*s_out)[L::outElems] = reinterpret_cast<uint16_t (*)[L::outElems]>(lds + L::tmpBytes);

    const int sub = threadIdx.x / G, l = threadIdx.x - sub * G;
    const int job = xcd_block(wg, wgs) * JPW + sub;
    const bool live = job < njobs;
    // havoc_mi355x_pred_uni_job: dst, ref, w, h, xFrac, yFrac | havoc_mi355x_pred_bi_job: dst, ref0, ref1, w, h, 4 fracs
    const int32_t *j = jobs + (long)(live ? job : 0) * (BI ? 12 : 8);
    const int w = BI ? j[3] : j[2], h = BI ? j[4] : j[3];
    const long dsb = stride_dst * S, rsb = stride_ref * S;
    const int maxv = (1 << bitDepth) - 1;
    const int shift1 = min(4, bitDepth - 8);
    const int shift3 = max(2, 14 - bitDepth);
    const int qpr = (w + 3) >> 2, wh = h + TAPS - 1;
    const FastDiv fq(qpr);

    // ---- phase 1: horizontal pass(es)
#pragma unroll
    for (int r = 0; r < NREF; ++r)
    {
        const char *r0 = ref + (long)j[1 + r] * S;
        int cx[TAPS];
        taps_of<TAPS>(BI ? j[5 + 2 * r] : j[4], cx);
        int16_t *tmp = s_tmp[sub][r];
        for (int i = l; i < wh * qpr; i += G)
        {
            const int y = fq.div(i), x0 = (i - y * qpr) * 4;
            int a[4];
            hfilter4<S, TAPS>(r0 + (y - AB) * rsb + (x0 - AB) * S, cx, a);
#pragma unroll
            for (int o = 0; o < 4; ++o)
                if (x0 + o < w) tmp[(x0 + o) * TH + y] = (int16_t)(a[o] >> shift1);
        }
    }
    __syncthreads();

    // ---- phase 2: vertical pass, one column of 8 rows per lane
    {
        uint32_t cp[NREF][TAPS / 2];
#pragma unroll
        for (int r = 0; r < NREF; ++r)
        {
            int cy[TAPS];
            taps_of<TAPS>(BI ? j[6 + 2 * r] : j[5], cy);
#pragma unroll
            for (int k = 0; k < TAPS / 2; ++k) cp[r][k] = pack_i16(cy[2 * k], cy[2 * k + 1]);
        }
        const int groups = (h + 7) >> 3;
        const FastDiv fw(w);
        uint16_t *ot = s_out[sub];
        for (int it = l; it < (live ? w * groups : 0); it += G)
        {
            const int gy = fw.div(it), x = it - gy * w;
            const int y0 = gy * 8;
            int acc[8];
#pragma unroll
            for (int r = 0; r < NREF; ++r)
            {
                const int16_t *col = &s_tmp[sub][r][x * TH + y0];
                const u32x4 q0 = *reinterpret_cast<const u32x4 *>(col), q1 = *reinterpret_cast<const u32x4 *>(col + 8);
                const uint32_t e[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
                uint32_t od[7];
#pragma unroll
                for (int k = 0; k < 7; ++k) od[k] = __builtin_amdgcn_alignbit(e[k + 1], e[k], 16);
#pragma unroll
                for (int jj = 0; jj < 8; ++jj)
                {
                    int a = 0;
#pragma unroll
                    for (int k = 0; k < TAPS / 2; ++k) a = sdot2((jj & 1) ? od[(jj >> 1) + k] : e[(jj >> 1) + k], cp[r][k], a);
                    if (!BI) acc[jj] = a;
                    else if (r == 0) acc[jj] = a >> 6;
                    else acc[jj] += a >> 6;
                }
            }
#pragma unroll
            for (int jj = 0; jj < 8; ++jj)
            {
                const int v = BI ? (acc[jj] + (1 << shift3)) >> (shift3 + 1) : (acc[jj] + (1 << (5 + shift3))) >> (6 + shift3);
                if (y0 + jj < h) ot[(y0 + jj) * OS + x] = (uint16_t)clip3(0, maxv, v);
            }
        }
    }
    __syncthreads();

    // ---- phase 3: coalesced row-wise write of exactly w x h samples
    if (!live) return;
    char *d = dst + (long)j[0] * S;
    const uint16_t *ot = s_out[sub];
    for (int i = l; i < h * qpr; i += G)
    {
        const int y = fq.div(i), x0 = (i - y * qpr) * 4;
        const uint16_t *p = ot + y * OS + x0;
        char *q = d + y * dsb + x0 * S;
        if (x0 + 4 <= w)
        {
            if (S == 1) st4(q, (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
            else st8(q, u32x2{(uint32_t)p[0] | ((uint32_t)p[1] << 16), (uint32_t)p[2] | ((uint32_t)p[3] << 16)});
        }
        else
            for (int o = 0; x0 + o < w; ++o) reinterpret_cast<T *>(q)[o] = (T)p[o];
    }
}

// ---- the lean form (w % 4 == 0) ----------------------------------------------------------------------------------------------------------------------------

// LDS of one workgroup: the transposed intermediates [JPW][NREF] of tileElems int16.  Column x starts at x * TH + (x / 4) * QSKEW: the horizontal pass stores
// one dword per column and row pair, lanes of one store are a quad of columns apart, and 4 * TH / 2 dwords is 0 or 16 mod 32 banks in every class; the 16
// bytes of skew per quad spread them (odd multiples of 4 dwords) and keep the vertical pass's 16-byte column reads aligned.  No output tile.
template <int MAXW, int MAXH, int G, bool BI>
struct PredLeanLds
{
    static constexpr int JPW = 256 / G, NREF = BI ? 2 : 1, TH = MAXH + 8, QSKEW = 8;
    static constexpr int tileElems = MAXW * TH + (MAXW / 4) * QSKEW;
    static constexpr int bytes = JPW * NREF * tileElems * 2;
    static_assert(bytes <= PredLds<MAXW, MAXH, G, BI>::bytes, "the lean form lives in the full form's LDS");
};

constexpr int kDppXor2 = 0x4E;        // quad_perm [2,3,0,1]

// The lanes c = 0..3 of a quad hold columns x0 + c of one block, v[] = rows y0 .. y0 + 7 of that column (clipped samples).  Two byte (S = 1) / halfword
// (S = 2) transposes across the quad turn them into whole rows: lane c gets rows y0 + c and y0 + 4 + c of the four columns and stores them, one dword /
// one 8-byte store each.  q: the lane's destination, row y0 + c, column x0; rowsLeft = h - y0.
template <int S>
__device__ __forceinline__ void store_quad_rows(char *q, long dsb, const int (&v)[8], int c, int rowsLeft)
{
    if (S == 1)
    {
        const uint32_t selA = (c & 1) ? 0x03070105u : 0x06020400u, selB = (c & 2) ? 0x03020706u : 0x05040100u;
#pragma unroll
        for (int half = 0; half < 2; ++half)
        {
            const int *u = v + 4 * half;
            uint32_t d = (uint32_t)u[0] | ((uint32_t)u[1] << 8) | ((uint32_t)u[2] << 16) | ((uint32_t)u[3] << 24);      // this column, rows 0..3 of the half
            d = __builtin_amdgcn_perm((uint32_t)dpp_mov<kDppXor1>((int)d), d, selA);      // even lanes: rows 0, 2 of columns c, c + 1; odd lanes: rows 1, 3 of columns c - 1, c
            d = __builtin_amdgcn_perm((uint32_t)dpp_mov<kDppXor2>((int)d), d, selB);      // row c of columns 0..3
            if (c + 4 * half < rowsLeft) st4(q + 4 * half * dsb, d);
        }
    }
    else
    {
        const uint32_t selA = (c & 1) ? 0x03020706u : 0x05040100u;
        const bool hi = (c & 2) != 0;
#pragma unroll
        for (int half = 0; half < 2; ++half)
        {
            const int *u = v + 4 * half;
            uint32_t e0 = (uint32_t)u[0] | ((uint32_t)u[1] << 16), e1 = (uint32_t)u[2] | ((uint32_t)u[3] << 16);      // this column, rows (0, 1) and (2, 3) of the half
            e0 = __builtin_amdgcn_perm((uint32_t)dpp_mov<kDppXor1>((int)e0), e0, selA);      // row (c & 1) of the lane pair's two columns
            e1 = __builtin_amdgcn_perm((uint32_t)dpp_mov<kDppXor1>((int)e1), e1, selA);      // row 2 + (c & 1) of them
            const uint32_t t = (uint32_t)dpp_mov<kDppXor2>((int)(hi ? e0 : e1));             // lanes 0, 1 need the other pair's e0, lanes 2, 3 its e1
            if (c + 4 * half < rowsLeft) st8(q + 4 * half * dsb, u32x2{hi ? t : e0, hi ? e1 : t});
        }
    }
}

// true when every job of workgroup `wg` has a width that is a multiple of four; the same value in every wavefront of the workgroup
template <int JPW, bool BI>
__device__ __forceinline__ bool widths_are_quads(const int32_t *__restrict__ jobs, int njobs, int wg, int wgs)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int job = xcd_block(wg, wgs) * JPW + lane;
    int w = 0;
    if (lane < JPW && job < njobs) w = jobs[(long)job * (BI ? 12 : 8) + (BI ? 3 : 2)];
    return __ballot(w & 3) == 0;
}

template <int S, int TAPS, int MAXW, int MAXH, int G, bool BI>
__device__ __forceinline__ void pred_workgroup_lean(char *lds, char *__restrict__ dst, long stride_dst, const char *__restrict__ ref, long stride_ref,
                                                    const int32_t *__restrict__ jobs, int njobs, int bitDepth, int wg, int wgs)
{
    typedef PredLeanLds<MAXW, MAXH, G, BI> L;
    constexpr int JPW = 256 / G;
    constexpr int NREF = BI ? 2 : 1;
    constexpr int AB = TAPS / 2 - 1;
    constexpr int TH = L::TH;
    constexpr bool ZP = G >= kWave;      // a wavefront serves one job: its phases are uniform, and a zero phase is not filtered
    int16_t *s_tile = reinterpret_cast<int16_t *>(lds);

    const int sub = ZP ? __builtin_amdgcn_readfirstlane((int)threadIdx.x / G) : (int)threadIdx.x / G;
    const int l = threadIdx.x - sub * G;
    const int job = xcd_block(wg, wgs) * JPW + sub;
    const bool live = job < njobs;
    const int32_t *j = jobs + (long)(live ? job : 0) * (BI ? 12 : 8);
    const int w = BI ? j[3] : j[2], h = BI ? j[4] : j[3];
    const long dsb = stride_dst * S, rsb = stride_ref * S;
    const int maxv = (1 << bitDepth) - 1;
    const int shift1 = min(4, bitDepth - 8);
    const int shift3 = max(2, 14 - bitDepth);
    const int qpr = w >> 2, wh = h + TAPS - 1;

    // ---- phase 1: horizontal pass(es).  Lane l owns quad q = l % qpr of the columns and walks the row pairs l / qpr, + G / qpr, ...
    {
        const FastDiv fq(qpr);
        const int rp0 = fq.div(l), q = l - rp0 * qpr, rstep = fq.div(G);
        if (live && rp0 < rstep)
        {
#pragma unroll
            for (int r = 0; r < NREF; ++r)
            {
                const int xf = BI ? j[5 + 2 * r] : j[4], yf = BI ? j[6 + 2 * r] : j[5];
                const bool xz = ZP && xf == 0, yz = ZP && yf == 0;
                const int rows = yz ? h : wh;      // yFrac == 0: only the block's own rows, tile row y = block row y
                const char *p = ref + ((long)j[1 + r] + q * 4) * S + (long)(2 * rp0 - (yz ? 0 : AB)) * rsb;      // sample (4 q, first row of the pair)
                const long step = 2L * rstep * rsb;
                uint32_t *cw = reinterpret_cast<uint32_t *>(s_tile + (sub * NREF + r) * L::tileElems + q * (4 * TH + L::QSKEW)) + rp0;
                if (xz)
                {
                    // xFrac == 0: the intermediate is (sample << 6) >> shift1 = sample << (6 - shift1), no bit is lost
                    const int sh = 6 - shift1;
                    for (int y = 2 * rp0; y < rows; y += 2 * rstep, p += step, cw += rstep)
                    {
                        const char *p1 = p + (y + 1 < rows ? rsb : 0);      // the pad row of an odd count repeats the last one: written, never read
                        if (S == 1)
                        {
                            const uint32_t a = ld4(p), b = ld4(p1);
#pragma unroll
                            for (int o = 0; o < 4; ++o) cw[o * (TH / 2)] = __builtin_amdgcn_perm(b, a, 0x0c000c00u | ((4u + o) << 16) | o) << sh;
                        }
                        else
                        {
                            const u32x2 a = ld8(p), b = ld8(p1);
                            cw[0 * (TH / 2)] = __builtin_amdgcn_perm(b.x, a.x, 0x05040100u) << sh;
                            cw[1 * (TH / 2)] = __builtin_amdgcn_perm(b.x, a.x, 0x07060302u) << sh;
                            cw[2 * (TH / 2)] = __builtin_amdgcn_perm(b.y, a.y, 0x05040100u) << sh;
                            cw[3 * (TH / 2)] = __builtin_amdgcn_perm(b.y, a.y, 0x07060302u) << sh;
                        }
                    }
                }
                else
                {
                    int cx[TAPS];
                    taps_of<TAPS>(xf, cx);
                    p -= AB * S;
                    for (int y = 2 * rp0; y < rows; y += 2 * rstep, p += step, cw += rstep)
                    {
                        HRaw<S, TAPS> ra, rb;
                        hfilter4_load<S, TAPS>(p, ra);
                        hfilter4_load<S, TAPS>(p + (y + 1 < rows ? rsb : 0), rb);
                        int a[4], b[4];
                        hfilter4_eval<S, TAPS>(ra, cx, a);
                        hfilter4_eval<S, TAPS>(rb, cx, b);
#pragma unroll
                        for (int o = 0; o < 4; ++o)
                            cw[o * (TH / 2)] = __builtin_amdgcn_perm((uint32_t)(b[o] >> shift1), (uint32_t)(a[o] >> shift1), 0x05040100u);      // two int16
                    }
                }
            }
        }
    }
    __syncthreads();
    if (!live) return;

    // ---- phase 2: vertical pass, one column of 8 rows per lane, and the write of whole rows by the quad
    uint32_t cp[NREF][TAPS / 2];
    bool yz[NREF];
#pragma unroll
    for (int r = 0; r < NREF; ++r)
    {
        const int yf = BI ? j[6 + 2 * r] : j[5];
        yz[r] = ZP && yf == 0;
        int cy[TAPS];
        taps_of<TAPS>(yf, cy);
#pragma unroll
        for (int k = 0; k < TAPS / 2; ++k) cp[r][k] = pack_i16(cy[2 * k], cy[2 * k + 1]);
    }
    const int groups = (h + 7) >> 3;
    const FastDiv fw(w);
    char *d = dst + (long)j[0] * S;
    const int c = l & 3;      // = x & 3: w and G are multiples of four
    for (int it = l; it < w * groups; it += G)
    {
        const int gy = fw.div(it), x = it - gy * w;
        const int y0 = gy * 8;
        int acc[8];
#pragma unroll
        for (int r = 0; r < NREF; ++r)
        {
            const int16_t *col = s_tile + (sub * NREF + r) * L::tileElems + x * TH + (x >> 2) * L::QSKEW + y0;
            const u32x4 q0 = *reinterpret_cast<const u32x4 *>(col);
            if (yz[r])
            {
                // yFrac == 0: the sum is 64 t, so a >> 6 = t (bi) and a = 64 t (uni)
                const uint32_t e[4] = {q0.x, q0.y, q0.z, q0.w};
#pragma unroll
                for (int jj = 0; jj < 8; ++jj)
                {
                    const int t = (jj & 1) ? (int)e[jj >> 1] >> 16 : (int)(e[jj >> 1] << 16) >> 16;
                    if (!BI) acc[jj] = t * 64;
                    else if (r == 0) acc[jj] = t;
                    else acc[jj] += t;
                }
            }
            else
            {
                const u32x4 q1 = *reinterpret_cast<const u32x4 *>(col + 8);
                const uint32_t e[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
                uint32_t od[7];
#pragma unroll
                for (int k = 0; k < 7; ++k) od[k] = __builtin_amdgcn_alignbit(e[k + 1], e[k], 16);
#pragma unroll
                for (int jj = 0; jj < 8; ++jj)
                {
                    int a = 0;
#pragma unroll
                    for (int k = 0; k < TAPS / 2; ++k) a = sdot2((jj & 1) ? od[(jj >> 1) + k] : e[(jj >> 1) + k], cp[r][k], a);
                    if (!BI) acc[jj] = a;
                    else if (r == 0) acc[jj] = a >> 6;
                    else acc[jj] += a >> 6;
                }
            }
        }
#pragma unroll
        for (int jj = 0; jj < 8; ++jj)
        {
            const int v = BI ? (acc[jj] + (1 << shift3)) >> (shift3 + 1) : (acc[jj] + (1 << (5 + shift3))) >> (6 + shift3);
            acc[jj] = clip3(0, maxv, v);
        }
        store_quad_rows<S>(d + (y0 + c) * dsb + (x - c) * S, dsb, acc, c, h - y0);
    }
}

// one workgroup's share of a size class, in the lean form where every job of the workgroup allows it (`lean`: the launch's HAVOC_PRED_LEAN)
template <int S, int TAPS, int MAXW, int MAXH, int G, bool BI>
__device__ __forceinline__ void pred_workgroup(char *lds, char *__restrict__ dst, long stride_dst, const char *__restrict__ ref, long stride_ref,
                                               const int32_t *__restrict__ jobs, int njobs, int bitDepth, int wg, int wgs, int lean)
{
    if (lean && widths_are_quads<256 / G, BI>(jobs, njobs, wg, wgs))
        pred_workgroup_lean<S, TAPS, MAXW, MAXH, G, BI>(lds, dst, stride_dst, ref, stride_ref, jobs, njobs, bitDepth, wg, wgs);
    else
        pred_workgroup_full<S, TAPS, MAXW, MAXH, G, BI>(lds, dst, stride_dst, ref, stride_ref, jobs, njobs, bitDepth, wg, wgs);
}

template <int S, int TAPS, int MAXW, int MAXH, int G, bool BI>
__global__ __launch_bounds__(256) void k_pred(char *__restrict__ dst, long stride_dst, const char *__restrict__ ref, long stride_ref,
                                              const int32_t *__restrict__ jobs, int njobs, int bitDepth, int lean)
{
    __shared__ __attribute__((aligned(16))) char lds[PredLds<MAXW, MAXH, G, BI>::bytes];
    pred_workgroup<S, TAPS, MAXW, MAXH, G, BI>(lds, dst, stride_dst, ref, stride_ref, jobs, njobs, bitDepth, blockIdx.x, gridDim.x, lean);
}

// ALL FOUR size classes of a job table in one launch (the width class stays a property of the job, the launch no longer is):
// the table is sorted by class -- count[c] jobs whose larger side is <= 8, 16, 32, 64 -- and a workgroup finds its class from the prefix of
// workgroups per class.  LDS is the largest class's (27 KB for bi-prediction), which still leaves 5 workgroups per CU.
struct PredClasses { int count[4], firstWg[5]; };

template <int S, int TAPS, bool BI>
__global__ __launch_bounds__(256) void k_pred_classes(char *__restrict__ dst, long stride_dst, const char *__restrict__ ref, long stride_ref,
                                                      const int32_t *__restrict__ jobs, PredClasses pc, int bitDepth, int lean)
{
    __shared__ __attribute__((aligned(16))) char lds[PredLds<64, 64, 256, BI>::bytes];
    constexpr int words = BI ? 12 : 8;
    const int wg = blockIdx.x;
    if (wg < pc.firstWg[1])
        pred_workgroup<S, TAPS, 8, 8, 8, BI>(lds, dst, stride_dst, ref, stride_ref, jobs, pc.count[0], bitDepth, wg, pc.firstWg[1], lean);
    else if (wg < pc.firstWg[2])
        pred_workgroup<S, TAPS, 16, 16, 32, BI>(lds, dst, stride_dst, ref, stride_ref, jobs + (long)pc.count[0] * words, pc.count[1], bitDepth, wg - pc.firstWg[1],
                                                pc.firstWg[2] - pc.firstWg[1], lean);
    else if (wg < pc.firstWg[3])
        pred_workgroup<S, TAPS, 32, 32, 128, BI>(lds, dst, stride_dst, ref, stride_ref, jobs + (long)(pc.count[0] + pc.count[1]) * words, pc.count[2], bitDepth,
                                                 wg - pc.firstWg[2], pc.firstWg[3] - pc.firstWg[2], lean);
    else
        pred_workgroup<S, TAPS, 64, 64, 256, BI>(lds, dst, stride_dst, ref, stride_ref, jobs + (long)(pc.count[0] + pc.count[1] + pc.count[2]) * words, pc.count[3],
                                                 bitDepth, wg - pc.firstWg[3], pc.firstWg[4] - pc.firstWg[3], lean);
}

// havoc::SubtractBi (havoc/pred_inter.h:87; havoc/pred_inter.cpp:2063-2080): dst = clip(2*src - pred)
template <int S>
__global__ __launch_bounds__(256) void k_subtract_bi(char *__restrict__ dst, long stride_dst, const char *__restrict__ pred, long stride_pred,
                                                     const char *__restrict__ src, long stride_src, const int32_t *__restrict__ jobs, int njobs,
                                                     int bitDepth, int lean)
{
    typedef typename Sample<S>::T T;
    const int job = xcd_block(blockIdx.x, gridDim.x) * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (job >= njobs) return;
    const int32_t *j = jobs + job * 8;   // havoc_mi355x_subtract_bi_job
    const int w = j[3], h = j[4];
    T *d = reinterpret_cast<T *>(dst) + j[0];
    const T *p = reinterpret_cast<const T *>(pred) + j[1];
    const T *s = reinterpret_cast<const T *>(src) + j[2];
    const int maxv = (1 << bitDepth) - 1;
    if (lean && (w & 3) == 0 && w <= 4 * kWave)      // at least one row per pass of the wavefront: wider blocks keep the sample loop
    {
        // four samples per lane: lane owns quad lane % (w / 4) of the columns and walks the rows lane / (w / 4), + 64 / (w / 4), ...; packed 16-bit arithmetic
        const int qpr = w >> 2;
        const FastDiv fq(qpr);
        const int y0 = fq.div(lane), q = lane - y0 * qpr, ystep = fq.div(kWave);
        if (y0 >= ystep) return;
        const long db = stride_dst * S, pb = stride_pred * S, sb = stride_src * S;
        char *dd = reinterpret_cast<char *>(d + 4 * q) + y0 * db;
        const char *pp = reinterpret_cast<const char *>(p + 4 * q) + y0 * pb, *ss = reinterpret_cast<const char *>(s + 4 * q) + y0 * sb;
        const s16x2 zero = {0, 0}, top = {(short)maxv, (short)maxv};
        auto sub_clip = [&](uint32_t sv, uint32_t pv) {
            const s16x2 a = __builtin_bit_cast(s16x2, sv), b = __builtin_bit_cast(s16x2, pv);
            return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_elementwise_max(a + a - b, zero), top));
        };
        for (int y = y0; y < h; y += ystep, dd += ystep * db, pp += ystep * pb, ss += ystep * sb)
        {
            if (S == 1)
            {
                const uint32_t sv = ld4(ss), pv = ld4(pp);
                const uint32_t lo = sub_clip(__builtin_amdgcn_perm(0u, sv, 0x0c010c00u), __builtin_amdgcn_perm(0u, pv, 0x0c010c00u));
                const uint32_t hi = sub_clip(__builtin_amdgcn_perm(0u, sv, 0x0c030c02u), __builtin_amdgcn_perm(0u, pv, 0x0c030c02u));
                st4(dd, __builtin_amdgcn_perm(hi, lo, 0x06040200u));
            }
            else
            {
                const u32x2 sv = ld8(ss), pv = ld8(pp);
                st8(dd, u32x2{sub_clip(sv.x, pv.x), sub_clip(sv.y, pv.y)});
            }
        }
        return;
    }
    const FastDiv fd(w);
    for (int i = lane; i < w * h; i += kWave)
    {
        const int y = fd.div(i), x = i - y * w;
        d[y * stride_dst + x] = (T)clip3(0, maxv, 2 * (int)s[y * stride_src + x] - (int)p[y * stride_pred + x]);
    }
}

// HAVOC_PRED_LEAN=0: every job takes the full form of the kernels above (diagnostic A/B switch, read once)
static int pred_lean()
{
    static const int on = !(getenv("HAVOC_PRED_LEAN") && atoi(getenv("HAVOC_PRED_LEAN")) == 0);
    return on;
}

template <int S, int TAPS, bool BI>
static hipError_t launch_pred_st(hipStream_t st, int bd, int maxw, int maxh, char *dst, long sd, const char *ref, long sr, const int32_t *jobs, int n)
{
    const dim3 b(256);
    if (maxw <= 8 && maxh <= 8)
        hipLaunchKernelGGL((k_pred<S, TAPS, 8, 8, 8, BI>), dim3((n + 31) / 32), b, 0, st, dst, sd, ref, sr, jobs, n, bd, pred_lean());
    else if (maxw <= 16 && maxh <= 16)
        hipLaunchKernelGGL((k_pred<S, TAPS, 16, 16, 32, BI>), dim3((n + 7) / 8), b, 0, st, dst, sd, ref, sr, jobs, n, bd, pred_lean());
    else if (maxw <= 32 && maxh <= 32)
        hipLaunchKernelGGL((k_pred<S, TAPS, 32, 32, 128, BI>), dim3((n + 1) / 2), b, 0, st, dst, sd, ref, sr, jobs, n, bd, pred_lean());
    else
        hipLaunchKernelGGL((k_pred<S, TAPS, 64, 64, 256, BI>), dim3(n), b, 0, st, dst, sd, ref, sr, jobs, n, bd, pred_lean());
    return hipGetLastError();
}

template <bool BI>
static hipError_t launch_pred(hipStream_t st, int S, int taps, int bd, int maxw, int maxh, void *dst, long sd, const void *ref, long sr,
                              const int32_t *j, int n)
{
    if (n <= 0) return hipSuccess;
    char *d = (char *)dst;
    const char *r = (const char *)ref;
    if (S == 1 && taps == 8) return launch_pred_st<1, 8, BI>(st, bd, maxw, maxh, d, sd, r, sr, j, n);
    if (S == 1 && taps == 4) return launch_pred_st<1, 4, BI>(st, bd, maxw, maxh, d, sd, r, sr, j, n);
    if (S == 2 && taps == 8) return launch_pred_st<2, 8, BI>(st, bd, maxw, maxh, d, sd, r, sr, j, n);
    if (S == 2 && taps == 4) return launch_pred_st<2, 4, BI>(st, bd, maxw, maxh, d, sd, r, sr, j, n);
    return hipErrorInvalidValue;
}

hipError_t launch_pred_uni(hipStream_t st, int S, int taps, int bd, int maxw, int maxh, void *dst, long sd, const void *ref, long sr,
                           const havoc_mi355x_pred_uni_job *jobs, int n)
{
    return launch_pred<false>(st, S, taps, bd, maxw, maxh, dst, sd, ref, sr, (const int32_t *)jobs, n);
}

hipError_t launch_pred_bi(hipStream_t st, int S, int taps, int bd, int maxw, int maxh, void *dst, long sd, const void *ref, long sr,
                          const havoc_mi355x_pred_bi_job *jobs, int n)
{
    return launch_pred<true>(st, S, taps, bd, maxw, maxh, dst, sd, ref, sr, (const int32_t *)jobs, n);
}

template <bool BI>
static hipError_t launch_pred_classes_t(hipStream_t st, int S, int taps, int bd, void *dst, long sd, const void *ref, long sr, const int32_t *j, const int count[4])
{
    PredClasses pc;
    static const int jpw[4] = {32, 8, 2, 1};
    pc.firstWg[0] = 0;
    for (int c = 0; c < 4; ++c)
    {
        if (count[c] < 0) return hipErrorInvalidValue;
        pc.count[c] = count[c];
        pc.firstWg[c + 1] = pc.firstWg[c] + (count[c] + jpw[c] - 1) / jpw[c];
    }
    if (pc.firstWg[4] == 0) return hipSuccess;
    char *d = (char *)dst;
    const char *r = (const char *)ref;
    const dim3 g(pc.firstWg[4]), b(256);
    if (S == 1 && taps == 8) hipLaunchKernelGGL((k_pred_classes<1, 8, BI>), g, b, 0, st, d, sd, r, sr, j, pc, bd, pred_lean());
    else if (S == 1 && taps == 4) hipLaunchKernelGGL((k_pred_classes<1, 4, BI>), g, b, 0, st, d, sd, r, sr, j, pc, bd, pred_lean());
    else if (S == 2 && taps == 8) hipLaunchKernelGGL((k_pred_classes<2, 8, BI>), g, b, 0, st, d, sd, r, sr, j, pc, bd, pred_lean());
    else if (S == 2 && taps == 4) hipLaunchKernelGGL((k_pred_classes<2, 4, BI>), g, b, 0, st, d, sd, r, sr, j, pc, bd, pred_lean());
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_pred_bi_classes(hipStream_t st, int S, int taps, int bd, void *dst, long sd, const void *ref, long sr, const havoc_mi355x_pred_bi_job *jobs, const int count[4])
{
    return launch_pred_classes_t<true>(st, S, taps, bd, dst, sd, ref, sr, (const int32_t *)jobs, count);
}

hipError_t launch_pred_uni_classes(hipStream_t st, int S, int taps, int bd, void *dst, long sd, const void *ref, long sr, const havoc_mi355x_pred_uni_job *jobs, const int count[4])
{
    return launch_pred_classes_t<false>(st, S, taps, bd, dst, sd, ref, sr, (const int32_t *)jobs, count);
}

hipError_t launch_subtract_bi(hipStream_t st, int S, int bitDepth, void *dst, long sd, const void *pred, long sp, const void *src, long ss,
                              const havoc_mi355x_subtract_bi_job *jobs, int n)
{
    if (n <= 0) return hipSuccess;
    if (S == 1)
        hipLaunchKernelGGL((k_subtract_bi<1>), dim3((n + 3) / 4), dim3(256), 0, st, (char *)dst, sd, (const char *)pred, sp, (const char *)src, ss,
                           (const int32_t *)jobs, n, bitDepth, pred_lean());
    else
        hipLaunchKernelGGL((k_subtract_bi<2>), dim3((n + 3) / 4), dim3(256), 0, st, (char *)dst, sd, (const char *)pred, sp, (const char *)src, ss,
                           (const int32_t *)jobs, n, bitDepth, pred_lean());
    return hipGetLastError();
}

} // namespace havoc_gpu
