// The last step of EncSao::rdSao (turing/EncSao.h:1017-1120): per CTU, the estimate of kernels_sao_decide.hip against
// "all off", merge-up and merge-left, each priced with CABAC rates (Search<sao>::go, Search.hpp:641-705) plus its distortion times the
// reciprocal lambda, in one call on the context's stream -- no host synchronisation, no allocation: capturable.
//
//   k_sao_merge_pre   one workgroup per CTU: the CTU filtered with its left and with its upper neighbour's ESTIMATED parameters, and
//                     computeSaoDistortion of each (sao_ctu.h); it also clears the hand-off words of the call.
//   k_sao_merge_rows  the raster dependency: a merge copies the neighbour's FINAL parameters, and the two SAO contexts flow from CTU to
//                     CTU.  One workgroup per CTU row, rows taken by ticket in the order workgroups start (so a row only waits for
//                     running workgroups); without WPP one workgroup walks the whole picture.  Per CTU, thread 0 prices the four
//                     candidates with integer rates; the distortion of a merge is dist_off when the neighbour's final parameters are
//                     off, the pre-pass value when they are the immediate neighbour's estimate, and -- only for a merge chain of two or
//                     more steps -- a fresh filter and SSD by the whole workgroup.  A finished CTU publishes ONE 64-bit word (done bit,
//                     its final source, its context states after its SAO syntax) with an agent-scope atomic store; the row below polls
//                     it with agent-scope atomic loads.  The payload travels inside the word, so no fence is needed.  Every wait is
//                     bounded: one that gives up raises a word the apply pass turns into records with `decided` = 0.
//   k_sao_merge_apply one workgroup per CTU: the decision record, and the CTU filtered again with its final parameters wherever they
//                     differ from its estimate.
#include "cabac_tables.h"
#include "launch.h"
#include "sao_ctu.h"

namespace havoc_gpu {

namespace {

constexpr int kMaxRow = 512;          // CTUs per row the decision pass holds in LDS (havoc_mi355x_sao_decide checks ctus_x against it)
constexpr int kSpinLimit = 1 << 22;   // polls of a hand-off word before a wait gives up

// the workspace: per CTU the decision (source, merge flags, distortion, context states), the published word and the two pre-pass
// distortions; then the row ticket and the give-up word
struct MergeWork
{
    int4 *dec;
    unsigned long long *pub;
    int32_t *distL, *distU, *ticket, *gaveUp;
};
__host__ __device__ inline MergeWork merge_work_of(void *base, int n)
{
    MergeWork w;
    char *p = static_cast<char *>(base);
    w.dec = reinterpret_cast<int4 *>(p);
    w.pub = reinterpret_cast<unsigned long long *>(w.dec + n);
    w.distL = reinterpret_cast<int32_t *>(w.pub + n);
    w.distU = w.distL + n;
    w.ticket = w.distU + n;
    w.gaveUp = w.ticket + 1;
    return w;
}

struct Planes
{
    const char *srcY, *srcC, *recY, *recC;
    char *dstY, *dstC;
    long ssy, ssc, rsy, rsc, dsy, dsc;
};

struct FilterLds
{
    SaoComp comp[2];
    int16_t table[2][32];
    uint32_t part[4][3];
};

// computeSaoDistortion (EncSao.h:815-947) of CTU c filtered with the parameters gcomp[2] (global memory), by the whole workgroup;
// every thread returns it.  EncSao::ssd: uint32 sums that wrap, >> 4 for 16-bit samples; chroma x distScale 4, an int total.
template <int S>
__device__ int ctu_dist(const SaoCtu &c, const SaoComp *gcomp, FilterLds &F, const Planes &P, int bd)
{
    typedef typename Sample<S>::T T;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    __syncthreads();      // the previous user of F is done
    if (tid < 22) reinterpret_cast<int32_t *>(F.comp)[tid] = reinterpret_cast<const int32_t *>(gcomp)[tid];
    __syncthreads();
    sao_offset_table(F.table, F.comp, tid, bd);
    __syncthreads();
    uint32_t acc[6] = { 0, 0, 0, 0, 0, 0 };
    sao_filter_ctu<T, false>(c, F.comp, F.table, bd, P.srcY, P.srcC, P.ssy, P.ssc, P.recY, P.recC, P.rsy, P.rsc, nullptr, nullptr, 0, 0, acc);
#pragma unroll
    for (int p = 0; p < 3; ++p)
    {
        const uint32_t t = wave_sum_u32(acc[2 * p]);
        if (lane == 0) F.part[wave][p] = t;
    }
    __syncthreads();
    uint32_t s[3];
    for (int p = 0; p < 3; ++p)
    {
        s[p] = F.part[0][p] + F.part[1][p] + F.part[2][p] + F.part[3][p];
        if (S == 2) s[p] >>= 4;
    }
    return (int32_t)(s[0] + s[1] * 4u + s[2] * 4u);
}

template <int S>
__global__ __launch_bounds__(256) void k_sao_merge_pre(const SaoCtu *__restrict__ ctus, const SaoParams *__restrict__ params, int cx, MergeWork wk,
                                                       int bd, Planes P)
{
    __shared__ FilterLds F;
    const int tid = threadIdx.x, i = blockIdx.x;
    if (tid == 0)
    {
        wk.pub[i] = 0;
        if (i == 0) *wk.ticket = *wk.gaveUp = 0;
    }
    const SaoCtu c = ctus[i];
    for (int k = 0; k < 2; ++k)
    {
        const int nb = k == 0 ? (i % cx > 0 ? i - 1 : -1) : (i >= cx ? i - cx : -1);
        int d = 0;
        // a neighbour whose estimate is all off is published as "off" by the decision pass, which then takes dist_off
        if (nb >= 0 && ctu_ok(c) && (params[nb].comp[0].type | params[nb].comp[1].type)) d = ctu_dist<S>(c, params[nb].comp, F, P, bd);
        if (tid == 0) (k ? wk.distU : wk.distL)[i] = d;
    }
}

struct RowLds
{
    int types[kMaxRow];     // the estimate's types: luma | chroma << 2
    int bypass[kMaxRow];    // bypass bins of the estimate's SAO syntax as Search<sao>::go prices it
    int dsao[kMaxRow], doff[kMaxRow], dleft[kMaxRow], dup[kMaxRow];
    int src[kMaxRow];       // this row's final sources (-1: off)
    int upSrc[kMaxRow];     // the row above's final sources and context states after their SAO syntax, as far as they are known
    int upCtx[kMaxRow];
};

template <int S>
__global__ __launch_bounds__(256) void k_sao_merge_rows(const SaoCtu *__restrict__ ctus, const SaoParams *__restrict__ params, int n, int cx, MergeWork wk,
                                                        int bd, int flags, long long lambda, int ctxMerge, int ctxType, Planes P)
{
    __shared__ RowLds R;
    __shared__ FilterLds F;
    __shared__ int sh[4];     // row ticket, the two fresh sources, "a wait gave up"
    __shared__ int bins[256];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    bins[tid] = bin_entry(tid >> 1, tid & 1);
    const int rows = n / cx, wpp = flags >> 2 & 1, cmax = (1 << (min(bd, 10) - 5)) - 1;
    int m = ctxMerge, t = ctxType;      // thread 0: the states of sao_merge_X_flag and sao_type_idx_X
    for (;;)
    {
        __syncthreads();
        if (tid == 0)
        {
            sh[0] = atomicAdd(wk.ticket, 1);
            sh[3] = 0;
        }
        __syncthreads();
        const int r = sh[0];
        if (r >= rows) return;
        for (int x = tid; x < cx; x += 256)
        {
            const int i = r * cx + x;
            const SaoParams &p = params[i];
            int ty = 0, nb = 0;
            for (int ci = 0; ci < 2; ++ci)
            {
                const SaoComp &q = p.comp[ci];
                ty |= q.type << (2 * ci);
                if (q.type == 0) continue;
                // sao_type_idx's second bin; sao_offset_abs truncated unary with cMax; then signs of the non-zero band offsets and
                // sao_band_position (5 bins), or sao_eo_class (2 bins) -- all bypass (Binarization.h:126-257).  Search<sao>::go prices
                // cIdx 0 and 1 only, never Cr (Search.hpp:674-703): the rate under-counts Cr as the reference does.
                nb += 1;
                for (int k = 0; k < 4; ++k) nb += min(q.offset_abs[k] + 1, cmax);
                if (q.type == 1)
                {
                    for (int k = 0; k < 4; ++k) nb += q.offset_abs[k] != 0;
                    nb += 5;
                }
                else
                    nb += 2;
            }
            R.types[x] = ty;
            R.bypass[x] = nb;
            R.dsao[x] = p.dist_sao;
            R.doff[x] = p.dist_off;
            R.dleft[x] = wk.distL[i];
            R.dup[x] = wk.distU[i];
        }
        int known = 0;      // wave 0: CTUs of the row above in upSrc / upCtx
        __syncthreads();
        for (int x = 0; x < cx; ++x)
        {
            const int i = r * cx + x;
            if (wave == 0 && r > 0)
            {
                // the upper CTU's final parameters; at the row start the contexts: after CTU (1, r - 1) with WPP (StatePictures.h:1058-1067),
                // else after the row above
                const int need = x > 0 ? x + 1 : (wpp ? min(2, cx) : cx);
                int spins = 0;
                while (known < need)
                {
                    const int j = known + lane;
                    unsigned long long w = 0;
                    if (j < cx) w = __hip_atomic_load(wk.pub + (long)(r - 1) * cx + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const unsigned long long done = __ballot(j < cx && (w >> 63));
                    const int run = done == ~0ull ? 64 : __builtin_ctzll(~done);
                    if (lane < run)
                    {
                        R.upSrc[j] = (int)(uint32_t)w - 1;
                        R.upCtx[j] = (int)(w >> 32) & 0xffff;
                    }
                    known += run;
                    if (run == 0)
                    {
                        __builtin_amdgcn_s_sleep(8);
                        if (++spins > kSpinLimit || __hip_atomic_load(wk.gaveUp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                        {
                            if (lane == 0) sh[3] = 1;
                            break;
                        }
                    }
                }
            }
            __syncthreads();
            if (sh[3])
            {   // the row gives up: the rows below are let through (they see the word too); the apply pass writes no decision
                if (tid == 0) atomicOr(wk.gaveUp, 1);
                for (int k = x + tid; k < cx; k += 256)
                    __hip_atomic_store(wk.pub + (long)r * cx + k, 1ull << 63, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
            if (tid == 0)
            {
                if (x == 0 && r > 0 && (!wpp || cx >= 2))
                {
                    const int s = R.upCtx[wpp ? 1 : cx - 1];
                    m = s & 0xff;
                    t = s >> 8;
                }
                else if (x == 0)
                {   // slice start, or a WPP row whose CTU (1, r - 1) does not exist: the slice's initial states
                    m = ctxMerge;
                    t = ctxType;
                }
                int f0 = -1, f1 = -1;
                if (flags & 3)
                {
                    const int su = r > 0 ? R.upSrc[x] : -1, sl = x > 0 ? R.src[x - 1] : -1;
                    if (su >= 0 && su != i - cx) f0 = su;
                    if (sl >= 0 && sl != i - 1) f1 = sl;
                }
                sh[1] = f0;
                sh[2] = f1;
            }
            __syncthreads();
            const int f0 = sh[1], f1 = sh[2];
            int fresh0 = 0, fresh1 = 0;
            if (f0 >= 0 || f1 >= 0)
            {
                const SaoCtu c = ctus[i];
                if (ctu_ok(c))
                {
                    if (f0 >= 0) fresh0 = ctu_dist<S>(c, params[f0].comp, F, P, bd);
                    if (f1 >= 0) fresh1 = f1 == f0 ? fresh0 : ctu_dist<S>(c, params[f1].comp, F, P, bd);
                }
            }
            if (tid == 0)
            {
                const int ty = R.types[x], t0 = ty & 3, t1 = ty >> 2, mBefore = m, tBefore = t;
                int src = -1, ml = 0, mu = 0, dist = R.doff[x];
                if (flags & 3)
                {
                    // the distortion of a merge whose final source is s: off, the neighbour's own estimate (the pre-pass value; with one CTU
                    // per row the left index is the upper one, so each merge checks its own neighbour only), or further up the chain
                    auto merged = [&](int s, int neighbour, int pre, int fresh) { return s < 0 ? R.doff[x] : s == neighbour ? pre : fresh; };
                    // 1. the estimate (EncSao.h:1029-1037).  sao_merge_left_flag = 0 is coded when rx > 0, then sao_merge_up_flag = 0
                    //    when ry > 0 (one slice, one tile: both neighbours are available); the shared context moves between them.
                    int mm = m, tt = t;
                    long long rate = (long long)R.bypass[x] << 16;
                    if (x > 0) rate += ctx_bin(bins, mm, 0);
                    if (r > 0) rate += ctx_bin(bins, mm, 0);
                    if (flags & 1) rate += ctx_bin(bins, tt, t0 != 0);
                    if (flags & 2) rate += ctx_bin(bins, tt, t1 != 0);
                    long long best = rate + (long long)R.dsao[x] * lambda;
                    src = ty ? i : -1;
                    dist = R.dsao[x];
                    // 2. all off, tried only when the luma or the chroma estimate is not type 0 (EncSao.h:1044); strict `<` throughout
                    if (t0 || t1)
                    {
                        mm = m;
                        tt = t;
                        rate = 0;
                        if (x > 0) rate += ctx_bin(bins, mm, 0);
                        if (r > 0) rate += ctx_bin(bins, mm, 0);
                        if (flags & 1) rate += ctx_bin(bins, tt, 0);
                        if (flags & 2) rate += ctx_bin(bins, tt, 0);
                        const long long cost = rate + (long long)R.doff[x] * lambda;
                        if (cost < best)
                        {
                            best = cost;
                            src = -1;
                            dist = R.doff[x];
                        }
                    }
                    // 3. merge-up (EncSao.h:1061-1076): sao_merge_left_flag = 0 first when rx > 0, then sao_merge_up_flag = 1
                    if (r > 0)
                    {
                        mm = m;
                        rate = 0;
                        if (x > 0) rate += ctx_bin(bins, mm, 0);
                        rate += ctx_bin(bins, mm, 1);
                        const int d = merged(R.upSrc[x], i - cx, R.dup[x], fresh0);
                        const long long cost = rate + (long long)d * lambda;
                        if (cost < best)
                        {
                            best = cost;
                            src = R.upSrc[x];
                            dist = d;
                            mu = 1;
                        }
                    }
                    // 4. merge-left (EncSao.h:1078-1093): the reference does not update bestCost here -- it is the last candidate
                    if (x > 0)
                    {
                        mm = m;
                        rate = ctx_bin(bins, mm, 1);
                        const int d = merged(R.src[x - 1], i - 1, R.dleft[x], fresh1);
                        if (rate + (long long)d * lambda < best)
                        {
                            src = R.src[x - 1];
                            dist = d;
                            ml = 1;
                            mu = 0;
                        }
                    }
                    // the bins Write codes for the choice (SyntaxCtu.hpp:46-72) move the contexts; Cr's bins are bypass.  rdSao itself
                    // leaves them as they were (EncSao.h:1119): the SAO contexts a CTU's rdSao sees are those at its start (Write.h:921-926).
                    if (x > 0) ctx_bin(bins, m, ml);
                    if (r > 0 && !ml) ctx_bin(bins, m, mu);
                    if (!ml && !mu)
                    {
                        if (flags & 1) ctx_bin(bins, t, src == i && t0 != 0);
                        if (flags & 2) ctx_bin(bins, t, src == i && t1 != 0);
                    }
                }
                // (flags & 3 == 0: no sao() is coded, SyntaxCtu.hpp:40 -- all off, the states unchanged)
                R.src[x] = src;
                wk.dec[i] = int4{ src, ml | mu << 1, dist, mBefore | tBefore << 8 | m << 16 | t << 24 };
                const unsigned long long word = 1ull << 63 | (unsigned long long)(m | t << 8) << 32 | (uint32_t)(src + 1);
                __hip_atomic_store(wk.pub + i, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

template <int S>
__global__ __launch_bounds__(256) void k_sao_merge_apply(const SaoCtu *__restrict__ ctus, const SaoParams *__restrict__ params, MergeWork wk, int bd, Planes P,
                                                         havoc_mi355x_sao_decision *__restrict__ out)
{
    typedef typename Sample<S>::T T;
    __shared__ SaoComp comp[2];
    __shared__ int16_t table[2][32];
    const int tid = threadIdx.x, i = blockIdx.x;
    int32_t *o = reinterpret_cast<int32_t *>(out + i);
    if (*wk.gaveUp)
    {   // a wait gave up: no record of the call is a decision
        if (tid < 32) o[tid] = 0;
        return;
    }
    const int4 d = wk.dec[i];
    const int src = d.x;
    if (tid < 22) reinterpret_cast<int32_t *>(comp)[tid] = src >= 0 ? reinterpret_cast<const int32_t *>(params[src].comp)[tid] : 0;
    __syncthreads();
    if (tid < 22)
        // a type-0 component is all zeros; the reference's SaoCtuData keeps the estimate's stale offsets, class and band there after
        // "all off" wins (EncSao.h:1046-1048 zero only SaoTypeIdx), which nothing reads
        o[tid] = comp[tid / 11].type ? reinterpret_cast<const int32_t *>(comp)[tid] : 0;
    else if (tid < 32)
        o[tid] = tid == 22 ? d.y & 1 : tid == 23 ? d.y >> 1 : tid == 24 ? d.z : tid == 25 ? src : tid == 26 ? d.w : tid == 27 ? 1 : 0;
    // the destination holds the CTU filtered with its estimate (havoc_mi355x_sao_estimate): filter it again where the final differs
    const SaoCtu c = ctus[i];
    const int estimate = (params[i].comp[0].type | params[i].comp[1].type) ? i : -1;
    if (src == estimate || !ctu_ok(c)) return;
    sao_offset_table(table, comp, tid, bd);
    __syncthreads();
    uint32_t acc[6] = { 0, 0, 0, 0, 0, 0 };
    sao_filter_ctu<T, true>(c, comp, table, bd, P.srcY, P.srcC, P.ssy, P.ssc, P.recY, P.recC, P.rsy, P.rsc, P.dstY, P.dstC, P.dsy, P.dsc, acc);
}

} // namespace

size_t sao_decide_workspace_bytes(int nctus) { return nctus <= 0 ? 0 : (size_t)nctus * (sizeof(int4) + 8 + 8) + 16; }

int sao_decide_max_row() { return kMaxRow; }

hipError_t launch_sao_decide(hipStream_t st, int S, int bd, long long lambda, int flags, const void *srcY, const void *srcC, long ssy, long ssc, const void *recY,
                             const void *recC, long rsy, long rsc, void *dstY, void *dstC, long dsy, long dsc, const SaoCtu *c, int n, int cx, const SaoParams *p,
                             int ctxMerge, int ctxType, void *work, havoc_mi355x_sao_decision *d)
{
    if (n <= 0) return hipSuccess;
    const MergeWork wk = merge_work_of(work, n);
    const Planes P{ (const char *)srcY, (const char *)srcC, (const char *)recY, (const char *)recC, (char *)dstY, (char *)dstC, ssy, ssc, rsy, rsc, dsy, dsc };
    // rows by ticket: at most one workgroup per CU (cdna_hip_programming 1: the grid stays resident); without WPP the rows are a chain
    const int rows = n / cx, grid = (flags & 4) ? (rows < 256 ? rows : 256) : 1;
    if (S == 1)
    {
        hipLaunchKernelGGL(k_sao_merge_pre<1>, dim3(n), dim3(256), 0, st, c, p, cx, wk, bd, P);
        hipLaunchKernelGGL(k_sao_merge_rows<1>, dim3(grid), dim3(256), 0, st, c, p, n, cx, wk, bd, flags, lambda, ctxMerge, ctxType, P);
        hipLaunchKernelGGL(k_sao_merge_apply<1>, dim3(n), dim3(256), 0, st, c, p, wk, bd, P, d);
    }
    else
    {
        hipLaunchKernelGGL(k_sao_merge_pre<2>, dim3(n), dim3(256), 0, st, c, p, cx, wk, bd, P);
        hipLaunchKernelGGL(k_sao_merge_rows<2>, dim3(grid), dim3(256), 0, st, c, p, n, cx, wk, bd, flags, lambda, ctxMerge, ctxType, P);
        hipLaunchKernelGGL(k_sao_merge_apply<2>, dim3(n), dim3(256), 0, st, c, p, wk, bd, P, d);
    }
    return hipGetLastError();
}

} // namespace havoc_gpu
