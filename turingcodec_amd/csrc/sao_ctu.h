// One CTU filtered with one set of SAO parameters, and EncSao::ssd of the result against the source (turing/EncSao.h:861-945), by a
// workgroup of 256 threads.  Shared by kernels_sao_decide.hip (the estimated parameters) and kernels_sao_merge.hip (the merge
// candidates of rdSao and the final parameters).
#pragma once

#include "common.h"

namespace havoc_gpu {

namespace {

using SaoCtu = havoc_mi355x_sao_ctu;
using SaoComp = havoc_mi355x_sao_component;
using SaoParams = havoc_mi355x_sao_params;

// a CTU the kernels can measure: luma 8..64 even (chroma 4..32); any other record is reported off and left alone
__device__ __forceinline__ bool ctu_ok(const SaoCtu &c) { return c.w >= 8 && c.h >= 8 && c.w <= 64 && c.h <= 64 && !(c.w & 1) && !(c.h & 1); }

__device__ __forceinline__ int sign3(int v) { return (v > 0) - (v < 0); }

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
    for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}

// LoopFilter.h:134-160 SaoOffsetVal (edge signs + + - -, band signs from sao_offset_sign) and the 32-entry band table of
// EncSao.h:866-877, for luma and chroma: threads 0..63 each write one entry of table[2][32]
__device__ __forceinline__ void sao_offset_table(int16_t (*table)[32], const SaoComp *comp, int tid, int bd)
{
    if (tid >= 64) return;
    const int k = tid & 31, ci = tid >> 5;
    const SaoComp &p = comp[ci];
    const int sh = bd - min(bd, 10);
    int v = 0;
    if (p.type == 1)
    {
        const int j = (k - p.band_position) & 31;
        if (j < 4) v = (p.offset_sign[j] ? -1 : 1) * p.offset_abs[j] << sh;
    }
    else if (p.type == 2 && k >= 1 && k <= 4)
        v = (k <= 2 ? 1 : -1) * p.offset_abs[k - 1] << sh;
    table[ci][k] = (int16_t)v;
}

// The CTU's Y, Cb and Cr filtered with comp / table (EncSao.h:861-945): every thread of the workgroup takes samples at stride 256.
// acc[2 p] += the squared error of plane p after the filter, acc[2 p + 1] without it (EncSao::ssd accumulates in uint32).  kWrite:
// the filtered samples go to the destination; without it nothing is stored.
template <typename T, bool kWrite>
__device__ __forceinline__ void sao_filter_ctu(const SaoCtu &c, const SaoComp *comp, const int16_t (*table)[32], int bd, const char *srcY,
                                               const char *srcC, long ssy, long ssc, const char *recY, const char *recC, long rsy, long rsc,
                                               char *dstY, char *dstC, long dsy, long dsc, uint32_t acc[6])
{
    const int tid = threadIdx.x, mx = (1 << bd) - 1;
    for (int plane = 0; plane < 3; ++plane)
    {
        const int ci = plane ? 1 : 0, type = comp[ci].type, e = comp[ci].eo_class & 3;
        const int bw = plane ? c.w >> 1 : c.w, bh = plane ? c.h >> 1 : c.h;
        const long ss = plane ? ssc : ssy, rs = plane ? rsc : rsy, ds = plane ? dsc : dsy;
        const T *src = reinterpret_cast<const T *>(plane ? srcC : srcY) + (plane == 0 ? c.src_y : plane == 1 ? c.src_cb : c.src_cr);
        const T *rec = reinterpret_cast<const T *>(plane ? recC : recY) + (plane == 0 ? c.rec_y : plane == 1 ? c.rec_cb : c.rec_cr);
        T *dst = kWrite ? reinterpret_cast<T *>(plane ? dstC : dstY) + (plane == 0 ? c.dst_y : plane == 1 ? c.dst_cb : c.dst_cr) : nullptr;
        // neighbours of the edge class (sao.cpp:63-73): horizontal, vertical, 135 degrees, 45 degrees
        const long n0 = (e == 0 ? 0 : -1) * rs + (e == 1 ? 0 : (e == 3 ? 1 : -1));
        const int16_t *tb = table[ci];
        // (unrolled: a thread's samples are independent, so their loads are in flight together -- the walk of kernels_sao_merge.hip
        // measures a CTU with one workgroup while nothing else runs beside it)
#pragma unroll 4
        for (int k = tid; k < bw * bh; k += 256)
        {
            const int y = k / bw, x = k - y * bw;
            const T *r = rec + y * rs + x;
            const int cv = r[0];
            int v = cv;
            if (type == 1)
                v = cv + tb[cv >> (bd - 5)];
            else if (type == 2)
            {
                int idx = 2 + sign3(cv - (int)r[n0]) + sign3(cv - (int)r[-n0]);
                idx = idx > 2 ? idx : (idx == 2 ? 0 : idx + 1);
                v = cv + tb[idx];
            }
            v = min(max(v, 0), mx);
            if (kWrite) dst[y * ds + x] = (T)v;
            const int s = src[y * ss + x], d1 = s - v, d0 = s - cv;
            acc[2 * plane] += (uint32_t)(d1 * d1);
            acc[2 * plane + 1] += (uint32_t)(d0 * d0);
        }
    }
}

} // namespace

} // namespace havoc_gpu
