// The SAO parameter estimation of one picture's CTUs: turing/EncSao.h:286-797
// (saoRdEstimateLuma / saoRdEstimateChroma) and the distortion the encoder weighs the result with, EncSao.h:800-947
// (computeSaoDistortion), in one call on the context's stream -- no host synchronisation, no allocation: capturable.
//
//   k_sao_est_jobs : the CTU records -> job records of the statistics kernels (kernels_sao.hip) in the workspace
//   k_sao_stats    : Y per CTU, Cb and Cr per CTU (one launch), k_sao_band_chroma: the joint Cb + Cr band histogram
//   k_sao_decide   : one workgroup per CTU.  Wavefront 0 decides luma, wavefront 1 chroma: lanes 0..15 take the 4 edge classes x
//                    4 categories (the offset loop of EncSao.h:340-350), lanes 16..45 the band positions 0..29 (EncSao.h:480-503,
//                    the four bands summed in order), then one lane walks the candidates in the reference's order (classes 0..3,
//                    then band positions from startBand down to 0) with its strict `<`.  All four wavefronts then filter the CTU's
//                    Y, Cb and Cr blocks into the destination and measure EncSao::ssd against the source with and without SAO.
//
// The double arithmetic must round where the reference's x86-64 build rounds: no fused multiply-add (`deltaD + lambda * rate` is
// two roundings there), sums in the reference's order, divisions in double (v_div_scale/fmas/fixup: IEEE).
#include "launch.h"
#include "sao_ctu.h"

#pragma clang fp contract(off)

namespace havoc_gpu {

namespace {

using StatsJob = havoc_mi355x_sao_stats_job;
using ChromaJob = havoc_mi355x_sao_chroma_job;

// the workspace: per CTU the statistics rows of kernels_sao.hip (Y 105, Cb 105, Cr 105, joint chroma bands 65 int64) and the jobs
struct Work
{
    long long *statY, *statC, *bandC;
    StatsJob *jobY, *jobC;
    ChromaJob *jobB;
};
__host__ __device__ inline Work work_of(void *base, int n)
{
    Work w;
    char *p = static_cast<char *>(base);
    w.statY = reinterpret_cast<long long *>(p);
    w.statC = w.statY + 105L * n;
    w.bandC = w.statC + 210L * n;
    w.jobY = reinterpret_cast<StatsJob *>(w.bandC + 65L * n);
    w.jobC = w.jobY + n;
    w.jobB = reinterpret_cast<ChromaJob *>(w.jobC + 2L * n);
    return w;
}

__global__ __launch_bounds__(256) void k_sao_est_jobs(const SaoCtu *__restrict__ ctus, int n, Work wk)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const SaoCtu c = ctus[i];
    const bool ok = ctu_ok(c);
    const int w = ok ? c.w : 2, h = ok ? c.h : 2, cw = ok ? c.w >> 1 : 2, ch = ok ? c.h >> 1 : 2;   // 2 x 2: an empty interior
    wk.jobY[i] = StatsJob{ c.src_y, c.rec_y, w, h };
    wk.jobC[i] = StatsJob{ c.stat_src_cb, c.stat_rec_cb, cw, ch };
    wk.jobC[n + i] = StatsJob{ c.stat_src_cr, c.stat_rec_cr, cw, ch };
    wk.jobB[i] = ChromaJob{ c.stat_src_cb, c.stat_src_cr, c.stat_rec_cb, c.stat_rec_cr, cw, ch, { 0, 0 } };
}

// EncSao::roundSao (EncSao.h:42-48); x >= 0 here
__device__ __forceinline__ int round_sao(int bd, double x)
{
    if (bd == 8) return x >= 0 ? (int)(x + 0.5) : (int)(x - 0.5);
    return x > 0 ? ((int)x + (1 << (bd - 9))) / (1 << (bd - 8)) : ((int)x - (1 << (bd - 9))) / (1 << (bd - 8));
}

// EncSao::estSaoDist (EncSao.h:49-59)
__device__ __forceinline__ long long est_dist(long long n, long long off, long long diff, int shift)
{
    const long long d = n * off * off - 2 * off * diff;
    if (shift == 0) return d;
    return d >= 0 ? d >> (2 * shift) : -((-d) >> (2 * shift));
}

struct DecideLds
{
    long long E[4][5], N[4][5], bE[32], bN[32];
    int start;
    double dj[16], bj[30];
    int eoff[16], boff[30][4];
};

// one component's search by one wavefront (EncSao.h:325-506 luma, :578-770 chroma with scale = distScale 4)
__device__ void decide(DecideLds &L, SaoComp &out, int lane, int bd, double lambda, int scale)
{
#pragma clang fp contract(off)
    const int shift = bd - 8, lim = (1 << (min(bd, 10) - 5)) - 1;
    if (lane < 16)
    {
        const int c = lane >> 2, k = (lane & 3) + 1, sign = k <= 2 ? 1 : -1;
        const long long n = L.N[c][k], e = L.E[c][k], ae = e < 0 ? -e : e;
        int q = 0;
        if (n != 0) q = c == 1 ? round_sao(bd, (double)(ae / n)) : round_sao(bd, (double)ae / (double)n);   // class 1: EncSao.h:369
        long long os = (q < 0 ? -q : q) + 1;
        os = os < lim ? os : lim;
        double dj = (double)(est_dist(n, sign * os, e, shift) * scale) + lambda * (double)(os + 1);
        long long off = sign * os;
        for (long long o = os - 1; o >= 0; --o)
        {
            const double cj = (double)(est_dist(n, sign * o, e, shift) * scale) + lambda * (double)(o + 1);
            if (cj < dj)
            {
                dj = cj;
                off = sign * o;
            }
        }
        L.dj[lane] = dj;
        L.eoff[lane] = (int)off;
    }
    else if (lane < 46 && lane - 16 <= L.start)
    {
        const int p = lane - 16;
        double tot = 0.0;
        for (int b = 0; b < 4; ++b)
        {
            // band 32 (position 29) is one past the reference's int64[32] arrays (EncSao.h:485): taken as an empty band
            const int i = p + b;
            const long long n = i < 32 ? L.bN[i] : 0, e = i < 32 ? L.bE[i] : 0, ae = e < 0 ? -e : e;
            const int q = n == 0 ? 0 : round_sao(bd, (double)ae / (double)n), aq = q < 0 ? -q : q;
            const int o = (e >= 0 ? 1 : -1) * (aq < lim ? aq : lim);
            tot = tot + ((double)(est_dist(n, o, e, shift) * scale) + lambda * (double)((o < 0 ? -o : o) + 2));
            L.boff[p][b] = o;
        }
        L.bj[p] = tot;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (lane == 0)
    {
        // the reference's sequential order and strict comparisons: classes 0..3, then band positions startBand .. 0
        double best = 0.0;
        int type = 0, cls = 0, band = 0, off[4] = { 0, 0, 0, 0 };
        for (int c = 0; c < 4; ++c)
        {
            double t = 0.0;
            for (int k = 0; k < 4; ++k) t += L.dj[4 * c + k];
            if (t < best)
            {
                best = t;
                type = 2;
                cls = c;
                for (int k = 0; k < 4; ++k) off[k] = L.eoff[4 * c + k];
            }
        }
        for (int p = L.start; p >= 0; --p)
            if (L.bj[p] < best)
            {
                best = L.bj[p];
                type = 1;
                band = p;
                for (int k = 0; k < 4; ++k) off[k] = L.boff[p][k];
            }
        if (abs(off[0]) + abs(off[1]) + abs(off[2]) + abs(off[3]) == 0) type = 0;
        out.type = type;
        out.eo_class = type == 2 ? cls : 0;
        out.band_position = type == 1 ? band : 0;
        for (int k = 0; k < 4; ++k)
        {
            out.offset_abs[k] = abs(off[k]);
            out.offset_sign[k] = type == 1 && off[k] < 0;
        }
    }
}

template <int S>
__global__ __launch_bounds__(256) void k_sao_decide(const SaoCtu *__restrict__ ctus, Work wk, int bd, double lambda, int flags,
                                                    const char *__restrict__ srcY, const char *__restrict__ srcC, long ssy, long ssc,
                                                    const char *__restrict__ recY, const char *__restrict__ recC, long rsy, long rsc,
                                                    char *__restrict__ dstY, char *__restrict__ dstC, long dsy, long dsc, SaoParams *__restrict__ params)
{
    typedef typename Sample<S>::T T;
    __shared__ DecideLds L[2];
    __shared__ SaoComp comp[2];
    __shared__ int16_t table[2][32];      // per component: the band table of EncSao.h:866-877 / SaoOffsetVal[5] of the edge filter
    __shared__ uint32_t part[4][6];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = blockIdx.x;
    const SaoCtu c = ctus[i];
    if (!ctu_ok(c))
    {
        if (tid < 32) reinterpret_cast<int32_t *>(params + i)[tid] = 0;
        return;
    }
    if (tid < 2 * 11) reinterpret_cast<int32_t *>(comp)[tid] = 0;
    const bool active = wave < 2 && (flags >> wave & 1);
    if (active)
    {
        DecideLds &D = L[wave];
        if (wave == 0)
        {
            const long long *st = wk.statY + 105L * i;
            if (lane < 40) (lane % 10 < 5 ? D.E[lane / 10][lane % 10] : D.N[lane / 10][lane % 10 - 5]) = st[lane];
            if (lane < 32)
            {
                D.bE[lane] = st[40 + lane];
                D.bN[lane] = st[72 + lane];
            }
            if (lane == 0) D.start = (int)st[104];
        }
        else
        {
            // EncSao.h:586-587: the Cb and Cr statistics summed per class and category; the band histogram is already joint
            const long long *a = wk.statC + 105L * i, *b = wk.statC + 105L * (i + (int)gridDim.x), *bc = wk.bandC + 65L * i;
            if (lane < 40) (lane % 10 < 5 ? D.E[lane / 10][lane % 10] : D.N[lane / 10][lane % 10 - 5]) = a[lane] + b[lane];
            if (lane < 32)
            {
                D.bE[lane] = bc[lane];
                D.bN[lane] = bc[32 + lane];
            }
            if (lane == 0) D.start = (int)bc[64];
        }
    }
    __syncthreads();
    if (active) decide(L[wave], comp[wave], lane, bd, lambda, wave ? 4 : 1);
    __syncthreads();
    sao_offset_table(table, comp, tid, bd);
    __syncthreads();
    // apply and measure (EncSao.h:861-945): Y, Cb, Cr; EncSao::ssd accumulates in uint32
    uint32_t acc[6] = { 0, 0, 0, 0, 0, 0 };
    sao_filter_ctu<T, true>(c, comp, table, bd, srcY, srcC, ssy, ssc, recY, recC, rsy, rsc, dstY, dstC, dsy, dsc, acc);
#pragma unroll
    for (int k = 0; k < 6; ++k)
    {
        const uint32_t t = wave_sum_u32(acc[k]);
        if (lane == 0) part[wave][k] = t;
    }
    __syncthreads();
    if (tid < 32)
    {
        SaoParams *o = params + i;
        if (tid < 22) reinterpret_cast<int32_t *>(o)[tid] = reinterpret_cast<const int32_t *>(comp)[tid];
        if (tid == 0)
        {
            uint32_t sao[3], off[3];
            for (int p = 0; p < 3; ++p)
            {
                sao[p] = part[0][2 * p] + part[1][2 * p] + part[2][2 * p] + part[3][2 * p];
                off[p] = part[0][2 * p + 1] + part[1][2 * p + 1] + part[2][2 * p + 1] + part[3][2 * p + 1];
                if (S == 2)
                {
                    sao[p] >>= 4;
                    off[p] >>= 4;
                }
                o->ssd_sao[p] = sao[p];
                o->ssd_off[p] = off[p];
            }
            // computeSaoDistortion's int total: chroma x distScale 4, all of it modulo 2^32
            o->dist_sao = (int32_t)(sao[0] + sao[1] * 4u + sao[2] * 4u);
            o->dist_off = (int32_t)(off[0] + off[1] * 4u + off[2] * 4u);
            o->reserved[0] = o->reserved[1] = 0;
        }
    }
}

} // namespace

size_t sao_workspace_bytes(int nctus) { return nctus <= 0 ? 0 : (size_t)nctus * ((105 * 3 + 65) * 8 + 3 * sizeof(StatsJob) + sizeof(ChromaJob)); }

hipError_t launch_sao_estimate(hipStream_t st, int S, int bd, double lambda, int flags, const void *srcY, const void *srcC, long ssy, long ssc, const void *recY,
                               const void *recC, long rsy, long rsc, void *dstY, void *dstC, long dsy, long dsc, const SaoCtu *c, int n, void *work, SaoParams *p)
{
    if (n <= 0) return hipSuccess;
    const Work wk = work_of(work, n);
    hipLaunchKernelGGL(k_sao_est_jobs, dim3((n + 255) / 256), dim3(256), 0, st, c, n, wk);
    hipError_t e;
    if ((flags & 1) && (e = launch_sao_stats(st, S, bd, srcY, ssy, recY, rsy, wk.jobY, n, (int64_t *)wk.statY)) != hipSuccess) return e;
    if ((flags & 2) && ((e = launch_sao_stats(st, S, bd, srcC, ssc, recC, rsc, wk.jobC, 2 * n, (int64_t *)wk.statC)) != hipSuccess ||
                        (e = launch_sao_band_chroma(st, S, bd, srcC, ssc, recC, rsc, wk.jobB, n, (int64_t *)wk.bandC)) != hipSuccess))
        return e;
    if (S == 1)
        hipLaunchKernelGGL(k_sao_decide<1>, dim3(n), dim3(256), 0, st, c, wk, bd, lambda, flags, (const char *)srcY, (const char *)srcC, ssy, ssc, (const char *)recY,
                           (const char *)recC, rsy, rsc, (char *)dstY, (char *)dstC, dsy, dsc, p);
    else
        hipLaunchKernelGGL(k_sao_decide<2>, dim3(n), dim3(256), 0, st, c, wk, bd, lambda, flags, (const char *)srcY, (const char *)srcC, ssy, ssc, (const char *)recY,
                           (const char *)recC, rsy, rsc, (char *)dstY, (char *)dstC, dsy, dsc, p);
    return hipGetLastError();
}

} // namespace havoc_gpu
