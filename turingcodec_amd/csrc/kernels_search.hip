// A picture's motion searches ENTIRELY ON THE DEVICE (round 3): the reference's decision loops (turing/Search.hpp:1252-1482, 1498-1657,
// 2060-2358, restated once in ../search/decision.hpp and compiled here for gfx950) run inside the kernels with the primitives they call --
// havoc_sad / havoc_sad_multiref (havoc/sad.h), HavocPredUni at a quarter-sample vector (read from the 16 fractional-sample planes of the
// reference picture, havoc_mi355x_interp_planes) + measureSatd (turing/Measure.h:97-135), SubtractBi (havoc/pred_inter.h:87) -- computed by the
// workgroup's own wavefronts.  No SAD surface, no job table and no host replay: what the batch client (../search/picture_search.cpp) obtains in
// launch + replay rounds over the link is here a function call.
//
//   k_search_rows   the uni-directional searches of a picture in ONE launch.  Dependencies are ../search/picture_order.hpp's (VERDICT r2 missing #2):
//                   a PU's two predictors are derived from the vectors decided for its left and upper neighbours, mvPreviousInteger2Nx2N is
//                   handed along the CTU row, CTU (x, y) starts when (x + 1, y - 1) is done (turing/TaskEncodeSubstream.cpp:71-95).  A workgroup
//                   per (CTU row, reference list) -- the two lists' searches of a PU read and write nothing of each other (Search.hpp:1883-1884)
//                   -- walks its row and waits, inside the kernel, for the row above to be two CTUs ahead.
//   k_search_step   the same CTU code, one launch per wavefront step s (the CTUs with x + 2y == s); stream order is the dependency.
//   k_search_bi     the bi-directional refinement of every PU (searchBi, Search.hpp:1796-1827), which feeds nothing back into the walk: a
//                   workgroup per PU, one launch per list after the walk.
//
// Inside a workgroup (4 wavefronts) every wavefront runs the same decision code on the same values, in SCALAR registers:
//   sad    (one position):    every wavefront computes it (nothing to exchange);
//   sad4   (four positions):  wavefront k computes position k, the four sums go through LDS (one barrier) -- or, where the positions were announced
//                             (hintSadRect: the 11 x 14 grid of a bi-directional refinement), four look-ups in a table computed in one pass;
//   satd   (8 or 9 sub-sample positions of a refinement step, announced by decision.hpp's hintSatd): a position per lane group (small blocks)
//          or per wavefront, read back into scalar registers once.
// The source block (or the bi-directional "ideal" block), a window of the reference picture around the start candidates and the decided
// vectors of the CTU and its neighbours live in LDS.  Exchange buffers alternate between two halves, so one barrier per exchange is enough.
#include "common.h"
#include "launch.h"

#include "../search/search_abi.h"
#include "../search/decision.hpp"
#include "../search/picture_order.hpp"

namespace havoc_gpu {

using havoc_search::Cost;
using havoc_search::Mv;

namespace {

struct SearchArgs
{
    havoc_search::SearchParams sp;
    Cost mvpRate[2];
    const char *src, *ref[2], *phase[2];      // sample (0, 0) of the source picture, of the two reference pictures, of their phase planes 0
    long srcStride, refStride, planeElems;    // samples
    const havoc_picture_pu *pus;
    const int32_t *ctuFirst;
    int ctusX, ctusY, cw, ch;
    havoc_search_result *out;
    havoc_search_result *outBi;               // bi-directional refinements (nullptr: none); until k_search_bi runs, the predictors of the searches
    int32_t *field;                           // [2][ch][cw]: x | y << 16
    uint8_t *valid;                           // [2][ch][cw]
    int32_t *rowPrev;                         // [ctusY][2]: mvPreviousInteger2Nx2N at the end of the row's last finished CTU
    int *progress;                            // [ctusY][2]: CTUs of the row done (the one-launch form)
    int *ticket, *gaveUp;                     // rows are handed out in the order workgroups start; a wait that gave up
    int rowLag;                               // CTUs the row above must be ahead: 2 = the reference's wavefront rule (TaskEncodeSubstream.cpp:71-95); 1 = diagnostic
    const int *rowsReady;                     // [2] or nullptr: luma rows (from picture row 0) of reference list l that are final in ref[l] AND in all of phase[l], raised
                                              // by another stream while this kernel runs (havoc_mi355x_search_gate): a CTU row waits for what its vectors can reach
};
// ... and with the units' temporal candidates (havoc_mi355x_search_temporal).  A record of its own, the argument of the <S, true> kernels alone: the kernels without a
// table keep the argument block, and with it the code, they had
struct SearchArgsTemporal : SearchArgs
{
    const havoc_search::TemporalCand *temporal;      // [2 * pu + list]
};
template <bool T> struct SearchArgsOf { typedef SearchArgs type; };
template <> struct SearchArgsOf<true> { typedef SearchArgsTemporal type; };
__device__ __forceinline__ const havoc_search::TemporalCand *temporalOf(const SearchArgs &) { return nullptr; }
__device__ __forceinline__ const havoc_search::TemporalCand *temporalOf(const SearchArgsTemporal &a) { return a.temporal; }

// LDS operands are named by address-space-3 pointers so that they are read with ds_read (a generic pointer would be a flat load)
typedef const __attribute__((address_space(3))) char *LdsPtr;
typedef __attribute__((address_space(3))) u32u lds_u32u;
typedef __attribute__((address_space(3))) u32x2u lds_u32x2u;
typedef __attribute__((address_space(3))) u32x4u lds_u32x4u;
using havoc_gpu::ld4;
using havoc_gpu::ld8;
using havoc_gpu::ld16;
__device__ __forceinline__ uint32_t ld4(LdsPtr p) { return *reinterpret_cast<const lds_u32u *>(p); }
__device__ __forceinline__ u32x2 ld8(LdsPtr p)
{
    const u32x2u v = *reinterpret_cast<const lds_u32x2u *>(p);
    return u32x2{v.x, v.y};
}
__device__ __forceinline__ u32x4 ld16(LdsPtr p)
{
    const u32x4u v = *reinterpret_cast<const lds_u32x4u *>(p);
    return u32x4{v.x, v.y, v.z, v.w};
}
template <class T>
__device__ __forceinline__ LdsPtr ldsPtr(T *p) { return (LdsPtr)p; }

// the wavefront's share `part` of `parts` of the block's row segments; the sum is NOT yet the table's value for 16-bit samples (sadShift)
template <int S, class PA, class PB>
__device__ __forceinline__ int wave_sad(PA a, long sab, PB b, long sbb, int w, int h, int lane, int part = 0, int parts = 1)
{
    uint32_t acc = 0;
    lane += kWave * part;
    const int stride = kWave * parts;
    if ((w & 7) == 0)
    {   // 8 samples per lane and row segment
        const int tw = w >> 3;
        const FastDiv fd(tw);
        for (int it = lane; it < tw * h; it += stride)
        {
            const int y = fd.div(it), x = it - y * tw;
            const PA pa = a + y * sab + x * 8 * S;
            const PB pb = b + y * sbb + x * 8 * S;
            if (S == 1)
            {
                const u32x2 va = ld8(pa), vb = ld8(pb);
                acc = __builtin_amdgcn_sad_u8(va.x, vb.x, acc);
                acc = __builtin_amdgcn_sad_u8(va.y, vb.y, acc);
            }
            else
            {
                const u32x4 va = ld16(pa), vb = ld16(pb);
                acc = __builtin_amdgcn_sad_u16(va.x, vb.x, acc);
                acc = __builtin_amdgcn_sad_u16(va.y, vb.y, acc);
                acc = __builtin_amdgcn_sad_u16(va.z, vb.z, acc);
                acc = __builtin_amdgcn_sad_u16(va.w, vb.w, acc);
            }
        }
    }
    else
    {   // 4 samples
        const int tw = w >> 2;
        const FastDiv fd(tw);
        for (int it = lane; it < tw * h; it += stride)
        {
            const int y = fd.div(it), x = it - y * tw;
            const PA pa = a + y * sab + x * 4 * S;
            const PB pb = b + y * sbb + x * 4 * S;
            if (S == 1)
                acc = __builtin_amdgcn_sad_u8(ld4(pa), ld4(pb), acc);
            else
            {
                const u32x2 va = ld8(pa), vb = ld8(pb);
                acc = __builtin_amdgcn_sad_u16(va.x, vb.x, acc);
                acc = __builtin_amdgcn_sad_u16(va.y, vb.y, acc);
            }
        }
    }
    return wave_sum((int)acc);
}
template <int S>
__device__ __forceinline__ int sadShift(int t) { return S == 2 ? t >> 2 : t; }      // havoc/sad.cpp: the 16-bit tables return sad >> 2

// measureSatd of a w x h block (w, h multiples of 4), one tile row per lane as k_satd (kernels_metric.hip) with a whole wavefront on the block
template <int S, class PA, class PB>
__device__ __forceinline__ int wave_satd(PA a, long sab, PB b, long sbb, int w, int h, int lane)
{
    int acc = 0;
    if (((w | h) & 7) == 0)
    {
        const int tw = w >> 3, n = tw * (h >> 3) * 8;
        const FastDiv fd(tw);
        for (int base = 0; base < n; base += kWave)      // every lane goes through satd_rows (its DPP steps read the neighbours' registers)
        {
            const int it = base + lane, r = it & 7;
            const bool on = it < n;
            const int tile = on ? it >> 3 : 0;
            const int ty = fd.div(tile), tx = tile - ty * tw;
            const PA pa8 = a + (long)(ty * 8 + r) * sab + tx * 8 * S;
            const PB pb8 = b + (long)(ty * 8 + r) * sbb + tx * 8 * S;
            if (S == 1)
            {
                u32x2 va = {0, 0}, vb = {0, 0};
                if (on)
                {
                    va = ld8(pa8);
                    vb = ld8(pb8);
                }
                const uint32_t m = 0x00ff00ffu;
                uint32_t p[4] = {pk_sub(va.x & m, vb.x & m), pk_sub((va.x >> 8) & m, (vb.x >> 8) & m), pk_sub(va.y & m, vb.y & m), pk_sub((va.y >> 8) & m, (vb.y >> 8) & m)};
                acc += satd_rows_pk<8>(p, r);
            }
            else
            {
                int d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                if (on)
                {
                    const u32x4 va = ld16(pa8), vb = ld16(pb8);
                    const uint32_t wa[4] = {va.x, va.y, va.z, va.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
                    for (int x = 0; x < 4; ++x)
                    {
                        d[2 * x] = (int)(wa[x] & 0xffff) - (int)(wb[x] & 0xffff);
                        d[2 * x + 1] = (int)(wa[x] >> 16) - (int)(wb[x] >> 16);
                    }
                }
                acc += satd_rows<S, 8>(d, r);
            }
        }
    }
    else
    {
        const int tw = w >> 2, n = tw * (h >> 2) * 4;
        const FastDiv fd(tw);
        for (int base = 0; base < n; base += kWave)
        {
            const int it = base + lane, r = it & 3;
            const bool on = it < n;
            const int tile = on ? it >> 2 : 0;
            const int ty = fd.div(tile), tx = tile - ty * tw;
            const PA pa4 = a + (long)(ty * 4 + r) * sab + tx * 4 * S;
            const PB pb4 = b + (long)(ty * 4 + r) * sbb + tx * 4 * S;
            if (S == 1)
            {
                const uint32_t va = on ? ld4(pa4) : 0u, vb = on ? ld4(pb4) : 0u, m = 0x00ff00ffu;
                uint32_t p[2] = {pk_sub(va & m, vb & m), pk_sub((va >> 8) & m, (vb >> 8) & m)};
                acc += satd_rows_pk<4>(p, r);
            }
            else
            {
                int d[4] = {0, 0, 0, 0};
                if (on)
                {
                    const u32x2 va = ld8(pa4), vb = ld8(pb4);
                    d[0] = (int)(va.x & 0xffff) - (int)(vb.x & 0xffff);
                    d[1] = (int)(va.x >> 16) - (int)(vb.x >> 16);
                    d[2] = (int)(va.y & 0xffff) - (int)(vb.y & 0xffff);
                    d[3] = (int)(va.y >> 16) - (int)(vb.y >> 16);
                }
                acc += satd_rows<S, 4>(d, r);
            }
        }
    }
    return wave_sum(acc);
}

constexpr int kWinBytes = 12 * 1024;      // per byte of sample size: the staged reference window of a search
constexpr int kWinMargin = 8;             // full samples around the start candidates: the probes after an improving start (+-2), star distances 1..8

// wavefronts of a workgroup: 4, 8 or 16 (a multiple of the four positions of a sad4; with more than 4, several wavefronts share a position's rows and a
// big block's (position, pass) SATD items spread wider).  Measured on the 1080p clip, one picture alone (profiles/r03/gpu_call_s.sh): 4 -> 14.4 ms,
// 8 -> 17.1 ms, 16 -> 26.7 ms: the barriers and the replicated scalar code cost more than the wider arithmetic saves, so 4.
#ifndef HAVOC_SEARCH_WAVES
#define HAVOC_SEARCH_WAVES 4
#endif
constexpr int kWaves = HAVOC_SEARCH_WAVES;
constexpr int kThreads = kWave * kWaves;
static_assert(kWaves % 4 == 0 && kWaves >= 4 && kWaves <= 16, "wavefronts per workgroup");

template <int S>
struct Lds      // of a workgroup
{
    int32_t sad[2][kWaves];
    int32_t ring[2][16];         // the SADs of a whole pattern call (4, 8 or 16 candidates)
    int32_t raster[704];         // ... of the raster refinement's 700 (208) positions
    int32_t satd[2][12];
    int32_t table[16 * 12];      // SADs of a rectangle of full-sample displacements (the grid of a bi-directional refinement)
    int32_t mv[256 + 36];        // the CTU's own 16 x 16 cells, the 16 cells left of it, the 16 cells above it, the cell above-left (288) and the cell above-right (289):
    uint8_t valid[256 + 36];     // where the five spatial candidates of a PU of this CTU can lie (search/picture_order.hpp: derivePredictors)
    alignas(16) uint8_t src[64 * 64 * S];
    alignas(16) uint8_t win[kWinBytes * S];
};

// What a CTU's searches share, staged ONCE per CTU (and list) by the picture kernels instead of once per search (round 4): the CTU's 64 x 64 source block and a
// window of the reference picture around the CTU, shifted by the first search's first start candidate.  A search whose start candidates (+ margin) lie inside
// reads both from here and stages nothing (staging was 2.1 of a search's 14.4 us: a dependent global round trip per search); one whose vectors point elsewhere
// stages its own window as before.  Which of the two serves a position changes no value.
constexpr int kCtuMargin = 56;
constexpr int kCtuWinW = 64 + 2 * kCtuMargin;      // 176 samples square: 31 KB (8-bit), 62 KB (16-bit)
constexpr int kPlaneReach = 84;                     // samples beyond the picture every plane is good for (havoc_search_picture_uni_device: ref_pad >= 96)
template <int S>
struct CtuStage
{
    alignas(16) uint8_t win[kCtuWinW * S * kCtuWinW];      // row pitch kCtuWinW * S bytes: a multiple of 16
    alignas(16) uint8_t src[64 * 64 * S];
};
struct CtuBox { int X0 = 0, Y0 = 0, X1 = -1, Y1 = -1; bool valid = false; };      // the staged window in picture coordinates (wave-uniform)

// the per-call interface decision.hpp's loops are written against (its `View`), answered by the workgroup itself
template <int S>
struct DeviceView
{
    const char *ref, *phase;      // the PU's position (x0, y0) in the reference picture and in its phase plane 0
    long sbb, planeBytes;
    int w, h, wave, lane, tid;
    Lds<S> *x;
    int bx0, by0, bx1, by1, wsB;      // displacements [bx0, bx1] x [by0, by1] are answered from the staged window (row pitch wsB bytes)
    LdsPtr winBase, srcBase;          // where displacement (bx0, by0) and the source block start in LDS (the search's own staging, or the CTU's)
    int srcPitch;                     // bytes per source row there: w * S, or 64 * S inside the CTU's block
    int sadTurn = 0, satdTurn = 0, satdCount = 0;
    int tx0 = 0, ty0 = 0, tw = 0, th = 0;      // displacements [tx0, tx0 + tw) x [ty0, ty0 + th) are in x->table (tw = 0: nothing is)
    int32_t satdKey[9], satdValue[9];      // the announced positions and their SATDs, read back once (scalar registers)
#ifdef HAVOC_SEARCH_TIMING
    long tHint = 0, acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tExit = 0;
#define GAP_IN() { if (tExit) { acc[6] += clock64() - tExit; acc[7] += 1; } }
#define GAP_OUT() { tExit = clock64(); }
#define TICK(k, expr) { const long t_ = clock64(); expr; acc[k] += clock64() - t_; }
#else
#define TICK(k, expr) { expr; }
#define GAP_IN()
#define GAP_OUT()
#endif

    __device__ __forceinline__ int sadOne(int dx, int dy, int part, int parts) const
    {
        if (dx >= bx0 && dx <= bx1 && dy >= by0 && dy <= by1)
            return wave_sad<S>(srcBase, srcPitch, winBase + (dy - by0) * wsB + (dx - bx0) * S, wsB, w, h, lane, part, parts);
        return wave_sad<S>(srcBase, srcPitch, ref + dy * sbb + (long)dx * S, sbb, w, h, lane, part, parts);
    }

    __device__ __forceinline__ int sad(int dx, int dy)
    {
        int v;
        GAP_IN();
        TICK(0, v = sadShift<S>(sadOne(dx, dy, 0, 1)));      // every wavefront, whole block: nothing to exchange
        GAP_OUT();
        return v;
    }

    __device__ __forceinline__ void sad4(const Mv d[4], int32_t out[4])
    {
        GAP_IN();
        if (tw)
        {   // announced (hintSadRect): four look-ups, no exchange
            bool all = true;
#pragma unroll
            for (int i = 0; i < 4; ++i) all &= d[i].x >= tx0 && d[i].x < tx0 + tw && d[i].y >= ty0 && d[i].y < ty0 + th;
            if (all)
            {
#pragma unroll
                for (int i = 0; i < 4; ++i) out[i] = __builtin_amdgcn_readfirstlane(x->table[(d[i].y - ty0) * tw + d[i].x - tx0]);
                GAP_OUT();
                return;
            }
        }
        // this wavefront's position, picked with masks: a choice between d[0..3] by address would keep the caller's array in (per-lane) private
        // memory, and whatever is read from there counts as divergent -- the whole decision state would leave the scalar registers
        const int k = wave & 3;
        const int s0 = -(k == 0), s1 = -(k == 1), s2 = -(k == 2), s3 = -(k == 3);
        const int mx = (d[0].x & s0) | (d[1].x & s1) | (d[2].x & s2) | (d[3].x & s3), my = (d[0].y & s0) | (d[1].y & s1) | (d[2].y & s2) | (d[3].y & s3);
        int v;
        TICK(0, v = sadOne(mx, my, wave >> 2, kWaves / 4));      // kWaves / 4 wavefronts share a position's row segments
        sadTurn ^= 1;
#ifdef HAVOC_SEARCH_TIMING
        const long c0 = clock64();
#endif
        if (lane == 0) x->sad[sadTurn][wave] = v;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i)
        {
            int t = 0;
#pragma unroll
            for (int p = 0; p < kWaves / 4; ++p) t += __builtin_amdgcn_readfirstlane(x->sad[sadTurn][i + 4 * p]);
            out[i] = sadShift<S>(t);
        }
#ifdef HAVOC_SEARCH_TIMING
        acc[1] += clock64() - c0;
#endif
        GAP_OUT();
    }

    // the SADs of every full-sample displacement of a rectangle (inside the staged window), a displacement per lane group (small blocks: up to
    // 16 per wavefront) or per wavefront; sad4 then answers from the table
    __device__ __forceinline__ void hintSadRect(int x0, int y0, int x1, int y1)
    {
        x0 = max(x0, bx0); y0 = max(y0, by0); x1 = min(x1, bx1); y1 = min(y1, by1);
        tw = 0;
        const int gw = x1 - x0 + 1, gh = y1 - y0 + 1, count = gw * gh;
        if (gw <= 0 || gh <= 0 || count > 16 * 12) return;
        const LdsPtr src = srcBase, win = winBase;
        const int seg = (w & 7) ? 4 : 8, segs = (w & 7) ? w >> 2 : w >> 3, rows = segs * h;      // row segments of seg samples per displacement
        const FastDiv fg(gw);
        if (rows > 32)
        {
            for (int j = wave; j < count; j += kWaves)
            {
                const int gy = fg.div(j), gx = j - gy * gw;
                const int v = wave_sad<S>(src, srcPitch, win + (y0 + gy - by0) * wsB + (x0 + gx - bx0) * S, wsB, w, h, lane);
                if (lane == 0) x->table[j] = sadShift<S>(v);
            }
        }
        else
        {
            const int Lsh = rows <= 4 ? 2 : (rows <= 8 ? 3 : (rows <= 16 ? 4 : 5)), L = 1 << Lsh, G = kWave >> Lsh;      // shifts: no division by a variable
            const int l = lane & (L - 1), g = lane >> Lsh;
            const FastDiv fs(segs);
            const int row = fs.div(l), col = l - row * segs;
            for (int base = 0; base < count; base += kWaves * G)
            {
                const int j = base + wave * G + g;
                const bool on = j < count && l < rows;
                const int jj = j < count ? j : 0;
                const int gy = fg.div(jj), gx = jj - gy * gw;
                const LdsPtr pa = src + (on ? row * srcPitch + col * seg * S : 0);
                const LdsPtr pb = win + (y0 + gy - by0 + (on ? row : 0)) * wsB + (x0 + gx - bx0) * S + (on ? col * seg * S : 0);
                uint32_t acc = 0;
                if (seg == 8)
                {
                    if (S == 1)
                    {
                        const u32x2 va = ld8(pa), vb = ld8(pb);
                        acc = __builtin_amdgcn_sad_u8(va.x, vb.x, acc);
                        acc = __builtin_amdgcn_sad_u8(va.y, vb.y, acc);
                    }
                    else
                    {
                        const u32x4 va = ld16(pa), vb = ld16(pb);
                        acc = __builtin_amdgcn_sad_u16(va.x, vb.x, acc);
                        acc = __builtin_amdgcn_sad_u16(va.y, vb.y, acc);
                        acc = __builtin_amdgcn_sad_u16(va.z, vb.z, acc);
                        acc = __builtin_amdgcn_sad_u16(va.w, vb.w, acc);
                    }
                }
                else if (S == 1)
                    acc = __builtin_amdgcn_sad_u8(ld4(pa), ld4(pb), acc);
                else
                {
                    const u32x2 va = ld8(pa), vb = ld8(pb);
                    acc = __builtin_amdgcn_sad_u16(va.x, vb.x, acc);
                    acc = __builtin_amdgcn_sad_u16(va.y, vb.y, acc);
                }
                int v = on ? (int)acc : 0;
                // sum over the group's lanes with row operations: after k steps the last lane of every aligned group of 2^k lanes holds its sum
                v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);                    // row_shr:1
                v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);                    // row_shr:2
                if (L >= 8) v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xe, true);        // row_shr:4
                if (L >= 16) v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xc, true);       // row_shr:8
                if (L >= 32) v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, true);       // row_bcast:15 into rows 1 and 3
                if (j < count && l == L - 1) x->table[j] = sadShift<S>(v);
            }
        }
        __syncthreads();
        tx0 = x0; ty0 = y0; tw = gw; th = gh;
    }

    __device__ __forceinline__ const char *predAt(Mv mv) const
    {
        return phase + (long)(4 * (mv.y & 3) + (mv.x & 3)) * planeBytes + (mv.y >> 2) * sbb + (long)(mv.x >> 2) * S;
    }

    // the positions the next costMv calls will ask for: small blocks several per wavefront (a position takes as many lanes as it has tile rows)
    __device__ __forceinline__ void hintSatd(const Mv *positions, int n)
    {
        GAP_IN();
        int32_t packed[9];
        satdTurn ^= 1;
        satdCount = n;
        computeSatds(positions, n, packed);
        {   // lane i reads position i, then the nine values move to scalar registers
            const int v = x->satd[satdTurn][lane < 9 ? lane : 0];
#pragma unroll
            for (int j = 0; j < 9; ++j)
            {
                satdKey[j] = packed[j];
                satdValue[j] = __builtin_amdgcn_readlane(v, j);
            }
        }
        GAP_OUT();
    }

    // the SATDs of n <= 9 sub-sample positions into x->satd[satdTurn][0 .. n), a position per lane group (small blocks) or per wavefront; ends with the barrier
    __device__ __forceinline__ void computeSatds(const Mv *positions, int n, int32_t (&packed)[9])
    {
#ifdef HAVOC_SEARCH_TIMING
        if (!tHint) tHint = wall_clock64();
        const long c0 = clock64();
#endif
        const LdsPtr src = srcBase;
        const int tsh = ((w | h) & 7) ? 2 : 3, ts = 1 << tsh, tw = w >> tsh;
        const int rows = tw * (h >> tsh) * ts;
        // the positions stay in registers: position `j` of a lane (group) or wavefront is picked with compares, not by address (an indexed array
        // would live in private memory), and nothing goes through LDS before the SATDs do
#pragma unroll
        for (int i = 0; i < 9; ++i) packed[i] = havoc_search::MotionField::pack(positions[i < n ? i : 0]);
        auto pick = [&](int j) {
            int32_t k = packed[0];
#pragma unroll
            for (int i = 1; i < 9; ++i) k = j == i ? packed[i] : k;
            return havoc_search::MotionField::unpack(k);
        };
#ifdef HAVOC_SEARCH_TIMING
        const long c1 = clock64();
#endif
        if (rows > 32)
        {   // a whole position per wavefront.  (Dealing its 64-row passes round the wavefronts was measured: the same latency for one picture
            // alone, but a third less throughput with 8 - 16 pictures in flight -- a reduction and an exchange per pass instead of per position)
            for (int i = wave; i < n; i += kWaves)
            {
                const int v = wave_satd<S>(src, srcPitch, predAt(pick(i)), sbb, w, h, lane);
                if (lane == 0) x->satd[satdTurn][i] = v;
            }
        }
        else
        {
            const int Lsh = rows <= 4 ? 2 : (rows <= 8 ? 3 : (rows <= 16 ? 4 : 5)), L = 1 << Lsh, G = kWave >> Lsh;      // shifts: no division by a variable
            const int l = lane & (L - 1), g = lane >> Lsh;
            const FastDiv fd(tw);
            for (int base = 0; base < n; base += kWaves * G)
            {
                const int j = base + wave * G + g;
                const bool on = j < n && l < rows;
                const char *pred = predAt(pick(j < n ? j : 0));
                int v;
                if (ts == 8)
                {
                    const int tile = on ? l >> 3 : 0, r = l & 7;
                    const int ty = fd.div(tile), tx = tile - ty * tw;
                    const LdsPtr pa = src + (ty * 8 + r) * srcPitch + tx * 8 * S;
                    const char *pb = pred + (long)(ty * 8 + r) * sbb + tx * 8 * S;
                    if (S == 1)
                    {
                        u32x2 va = {0, 0}, vb = {0, 0};
                        if (on)
                        {
                            va = ld8(pa);
                            vb = ld8(pb);
                        }
                        const uint32_t m = 0x00ff00ffu;
                        uint32_t p[4] = {pk_sub(va.x & m, vb.x & m), pk_sub((va.x >> 8) & m, (vb.x >> 8) & m), pk_sub(va.y & m, vb.y & m), pk_sub((va.y >> 8) & m, (vb.y >> 8) & m)};
                        v = satd_rows_pk<8>(p, r);
                    }
                    else
                    {
                        int d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                        if (on)
                        {
                            const u32x4 va = ld16(pa), vb = ld16(pb);
                            const uint32_t wa[4] = {va.x, va.y, va.z, va.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
                            for (int k = 0; k < 4; ++k)
                            {
                                d[2 * k] = (int)(wa[k] & 0xffff) - (int)(wb[k] & 0xffff);
                                d[2 * k + 1] = (int)(wa[k] >> 16) - (int)(wb[k] >> 16);
                            }
                        }
                        v = satd_rows<S, 8>(d, r);
                    }
                }
                else
                {
                    const int tile = on ? l >> 2 : 0, r = l & 3;
                    const int ty = fd.div(tile), tx = tile - ty * tw;
                    const LdsPtr pa = src + (ty * 4 + r) * srcPitch + tx * 4 * S;
                    const char *pb = pred + (long)(ty * 4 + r) * sbb + tx * 4 * S;
                    if (S == 1)
                    {
                        const uint32_t va = on ? ld4(pa) : 0u, vb = on ? ld4(pb) : 0u, m = 0x00ff00ffu;
                        uint32_t p[2] = {pk_sub(va & m, vb & m), pk_sub((va >> 8) & m, (vb >> 8) & m)};
                        v = satd_rows_pk<4>(p, r);
                    }
                    else
                    {
                        int d[4] = {0, 0, 0, 0};
                        if (on)
                        {
                            const u32x2 va = ld8(pa), vb = ld8(pb);
                            d[0] = (int)(va.x & 0xffff) - (int)(vb.x & 0xffff);
                            d[1] = (int)(va.x >> 16) - (int)(vb.x >> 16);
                            d[2] = (int)(va.y & 0xffff) - (int)(vb.y & 0xffff);
                            d[3] = (int)(va.y >> 16) - (int)(vb.y >> 16);
                        }
                        v = satd_rows<S, 4>(d, r);
                    }
                }
                for (int o = ts; o < L; o <<= 1) v += __shfl_xor(v, o, kWave);      // the tiles' costs (in their first lanes) to the position's total
                if (j < n && l == 0) x->satd[satdTurn][j] = v;
            }
        }
#ifdef HAVOC_SEARCH_TIMING
        const long c2 = clock64();
#endif
        __syncthreads();
#ifdef HAVOC_SEARCH_TIMING
        const long c3 = clock64();
        acc[2] += c1 - c0; acc[3] += c2 - c1; acc[4] += c3 - c2;
#endif
    }

    // ---- whole steps of decision.hpp's loops with a candidate per LANE (decision.hpp: foldPatternStep / foldSubpelStep) ----
    __device__ __forceinline__ static uint64_t quadMin(uint64_t key)
    {   // the smallest key of each aligned group of four lanes, in all four (two quad permutations: lane ^ 1, lane ^ 2)
        {
            const int lo = (int)(uint32_t)key, hi = (int)(uint32_t)(key >> 32);
            const uint32_t olo = (uint32_t)__builtin_amdgcn_update_dpp(0, lo, 0xB1, 0xf, 0xf, false), ohi = (uint32_t)__builtin_amdgcn_update_dpp(0, hi, 0xB1, 0xf, 0xf, false);
            const uint64_t other = ((uint64_t)ohi << 32) | olo;
            key = other < key ? other : key;
        }
        {
            const int lo = (int)(uint32_t)key, hi = (int)(uint32_t)(key >> 32);
            const uint32_t olo = (uint32_t)__builtin_amdgcn_update_dpp(0, lo, 0x4E, 0xf, 0xf, false), ohi = (uint32_t)__builtin_amdgcn_update_dpp(0, hi, 0x4E, 0xf, 0xf, false);
            const uint64_t other = ((uint64_t)ohi << 32) | olo;
            key = other < key ? other : key;
        }
        return key;
    }

#ifndef HAVOC_NO_PATTERN_LANES
    // sad4 + the four best.consider() of StateMeFullPel::considerPattern (Search.hpp:1447-1482): lane i of every quad costs candidate i; the winner is the
    // first of the cheapest (what considering them in order leaves in `best`), taken if it beats `best` strictly
    __device__ __forceinline__ bool patternStep(const Mv d0, const Mv d1, const Mv d2, const Mv d3, const havoc_search::PuContext &pu, const havoc_search::Lambda lambda,
                                                havoc_search::MvCandidate &best)
    {
        GAP_IN();
        const int i = lane & 3;
        const int px = i == 0 ? d0.x : (i == 1 ? d1.x : (i == 2 ? d2.x : d3.x));
        const int py = i == 0 ? d0.y : (i == 1 ? d1.y : (i == 2 ? d2.y : d3.y));
        auto inTable = [&](Mv m) { return m.x >= tx0 && m.x < tx0 + tw && m.y >= ty0 && m.y < ty0 + th; };
        const bool all = tw != 0 && inTable(d0) && inTable(d1) && inTable(d2) && inTable(d3);
        int sadv;
        if (all)
            sadv = x->table[(py - ty0) * tw + px - tx0];      // announced (hintSadRect): a look-up per lane
        else
        {
            const int k = wave & 3;
            const int s0 = -(k == 0), s1 = -(k == 1), s2 = -(k == 2), s3 = -(k == 3);
            const int mx = (d0.x & s0) | (d1.x & s1) | (d2.x & s2) | (d3.x & s3), my = (d0.y & s0) | (d1.y & s1) | (d2.y & s2) | (d3.y & s3);
            int v;
            TICK(0, v = sadOne(mx, my, wave >> 2, kWaves / 4));
            sadTurn ^= 1;
            if (lane == 0) x->sad[sadTurn][wave] = v;
            __syncthreads();
            int t = 0;
#pragma unroll
            for (int p = 0; p < kWaves / 4; ++p) t += x->sad[sadTurn][i + 4 * p];
            sadv = sadShift<S>(t);
        }
        const Mv mv(int16_t(px << 2), int16_t(py << 2));
        const Mv m0 = mv - pu.mvp[0], m1 = mv - pu.mvp[1];
        const Cost c0 = havoc_search::rateOf(m0) + pu.mvpRate[0], c1 = havoc_search::rateOf(m1) + pu.mvpRate[1];
        const bool second = c1 < c0;      // MvCandidate's constructor: the second predictor replaces the first on strictly smaller cost
        const Cost c = (second ? c1 : c0) + lambda * sadv;
        const int32_t mvdPacked = havoc_search::MotionField::pack(second ? m1 : m0);
        const uint64_t key = quadMin(((uint64_t)c << 2) | (uint32_t)i);
        const uint32_t klo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)key), khi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(key >> 32));
        const int w = klo & 3;
        const Cost cw = (Cost)((((uint64_t)khi << 32) | klo) >> 2);
        const bool improved = havoc_search::costLess(cw, best.cost);
        if (improved)
        {
            const int s0 = -(w == 0), s1 = -(w == 1), s2 = -(w == 2), s3 = -(w == 3);
            best.cost = cw;
            best.mv = havoc_search::shl2(Mv(int16_t((d0.x & s0) | (d1.x & s1) | (d2.x & s2) | (d3.x & s3)), int16_t((d0.y & s0) | (d1.y & s1) | (d2.y & s2) | (d3.y & s3))));
            best.mvd = havoc_search::MotionField::unpack(__builtin_amdgcn_readlane(mvdPacked, w));
            best.mvpFlag = __builtin_amdgcn_readlane((int)second, w);
        }
        GAP_OUT();
        return improved;
    }

#endif
    // a candidate's cost in its lane: the cheaper predictor (the second on strictly smaller cost, as MvCandidate's constructor), rate + lambda * sad
    __device__ __forceinline__ static Cost laneCost(int px, int py, const havoc_search::PuContext &pu, const havoc_search::Lambda lambda, int sadv, int32_t &mvdPacked, int &second)
    {
        const Mv mv(int16_t(px << 2), int16_t(py << 2));
        const Mv m0 = mv - pu.mvp[0], m1 = mv - pu.mvp[1];
        const Cost c0 = havoc_search::rateOf(m0) + pu.mvpRate[0], c1 = havoc_search::rateOf(m1) + pu.mvpRate[1];
        second = c1 < c0;
        mvdPacked = havoc_search::MotionField::pack(second ? m1 : m0);
        return (second ? c1 : c0) + lambda * sadv;
    }
    __device__ __forceinline__ static uint64_t read64(uint64_t v, int l)
    {
        return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    }
    __device__ __forceinline__ static uint64_t scalarMin(uint64_t a, uint64_t b) { return havoc_search::costLess((Cost)b, (Cost)a) ? b : a; }      // non-negative keys

    // A WHOLE considerPattern call (Search.hpp:1447-1482): its 4, 8 or 16 candidates one per lane, their SADs dealt round the wavefronts, ONE exchange.  The
    // reference folds the candidates into `best` four at a time in order; the first of the cheapest, taken on strictly smaller cost, is what that leaves.
    __device__ __forceinline__ int patternRing(Mv origin, const Mv *pattern, int n, int step, int dist, const havoc_search::LimitFullPelMv &limit, const havoc_search::PuContext &pu,
                                               const havoc_search::Lambda lambda, havoc_search::MvCandidate &best)
    {
        static_assert(kWaves == 4, "a candidate group per wavefront");
        GAP_IN();
        const int count = step == 1 ? n : (step == 2 ? n >> 1 : n / step), c = lane & 15;
        const Mv p = pattern[(c < count ? c : 0) * step];
        int px = (origin.x + dist * p.x) / 4, py = (origin.y + dist * p.y) / 4;
        px = min(max(px, (int)limit.lo.x), (int)limit.hi.x);
        py = min(max(py, (int)limit.lo.y), (int)limit.hi.y);
        sadTurn ^= 1;
        for (int q = 0; 4 * q < count; ++q)
        {
            const int cc = (wave & 3) + 4 * q;
            const int mx = __builtin_amdgcn_readlane(px, cc), my = __builtin_amdgcn_readlane(py, cc);
            int v;
            TICK(0, v = sadOne(mx, my, 0, 1));
            if (lane == 0) x->ring[sadTurn][cc] = v;
        }
        __syncthreads();
        const int sadv = sadShift<S>(x->ring[sadTurn][c < count ? c : 0]);
        int32_t mvdPacked;
        int second;
        const Cost cost = laneCost(px, py, pu, lambda, sadv, mvdPacked, second);
        const uint64_t key = quadMin(c < count ? (((uint64_t)cost << 4) | (uint32_t)c) : ~0ull);
        uint64_t k = read64(key, 0);
        if (count > 4) k = scalarMin(k, read64(key, 4));
        if (count > 8) k = scalarMin(scalarMin(k, read64(key, 8)), read64(key, 12));
        const int w = (int)(k & 15);
        const Cost cw = (Cost)(k >> 4);
        const bool improved = havoc_search::costLess(cw, best.cost);
        if (improved)
        {
            best.cost = cw;
            best.mv = havoc_search::shl2(Mv(int16_t(__builtin_amdgcn_readlane(px, w)), int16_t(__builtin_amdgcn_readlane(py, w))));
            best.mvd = havoc_search::MotionField::unpack(__builtin_amdgcn_readlane(mvdPacked, w));
            best.mvpFlag = __builtin_amdgcn_readlane(second, w);
        }
        GAP_OUT();
        return improved ? 1 : 0;
    }

#ifdef HAVOC_SEARCH_START_PROBE      // measured, no gain (1080p picture alone 16.9 ms either way; with the hexagon's eight measured speculatively as well: 17.2 ms): off
    // A start candidate of fullPelMotionEstimation AND the early-termination probe around it (Search.hpp:2100-2196, the diamond and hexagon of :2112-2124): the
    // candidate's SAD, the diamond's four and (coding units of 32 and more) the hexagon's eight measured TOGETHER -- the probe's positions depend only on the
    // candidate's -- in one exchange, then decided in the reference's order: the candidate against `best`; if it wins and early termination is on, the diamond
    // (any improvement: no termination), then the hexagon.  A typical search at reference distance 1 is this step and the two sub-sample steps.
    __device__ __forceinline__ int startProbe(Mv mvQ, int forcedFlag, bool met, bool hexagon, const havoc_search::LimitFullPelMv &limit, const havoc_search::PuContext &pu,
                                              const havoc_search::Lambda lambda, havoc_search::MvCandidate &best, Cost *costOut, int &calls)
    {
        static_assert(kWaves == 4, "a candidate group per wavefront");
        static constexpr Mv probe[16] = {{0, 0}, {-4, 0}, {0, 4}, {4, 0}, {0, -4}, {0, -8}, {8, -4}, {8, 4}, {0, 8}, {-8, 4}, {-8, -4}, {-8, 4}, {-8, -4}, {0, 0}, {0, 0}, {0, 0}};
        GAP_IN();
        const int count = met ? 5 : 1, c = lane & 15;      // (the hexagon's eight measured here as well was tried: slower -- 3-4 SADs per wavefront before the exchange)
        const Mv p = probe[c];
        int px = (mvQ.x + p.x) / 4, py = (mvQ.y + p.y) / 4;
        if (c)
        {   // the candidate itself is not limited here (the zero vector never is; the others were by the caller)
            px = min(max(px, (int)limit.lo.x), (int)limit.hi.x);
            py = min(max(py, (int)limit.lo.y), (int)limit.hi.y);
        }
        sadTurn ^= 1;
        for (int q = 0; 4 * q < count; ++q)
        {
            const int cc = (wave & 3) + 4 * q;
            if (cc < count)
            {
                const int mx = __builtin_amdgcn_readlane(px, cc), my = __builtin_amdgcn_readlane(py, cc);
                int v;
                TICK(0, v = sadOne(mx, my, 0, 1));
                if (lane == 0) x->ring[sadTurn][cc] = v;
            }
        }
        __syncthreads();
        const int sadv = sadShift<S>(x->ring[sadTurn][c < count ? c : 0]);
        int32_t mvdPacked;
        int second;
        Cost cost = laneCost(px, py, pu, lambda, sadv, mvdPacked, second);
        if (forcedFlag >= 0 && c == 0)
        {   // a predictor's own start candidate: costed with THAT predictor
            const Mv mvd = mvQ - pu.mvp[forcedFlag];
            cost = havoc_search::rateOf(mvd) + pu.mvpRate[forcedFlag] + lambda * sadv;
            mvdPacked = havoc_search::MotionField::pack(mvd);
            second = forcedFlag;
        }
        auto take = [&](int w, Cost cw) {
            best.cost = cw;
            best.mv = havoc_search::shl2(Mv(int16_t(__builtin_amdgcn_readlane(px, w)), int16_t(__builtin_amdgcn_readlane(py, w))));
            best.mvd = havoc_search::MotionField::unpack(__builtin_amdgcn_readlane(mvdPacked, w));
            best.mvpFlag = __builtin_amdgcn_readlane(second, w);
        };
        ++calls;
        const Cost c0 = (Cost)read64((uint64_t)cost, 0);
        if (costOut) *costOut = c0;
        int ends = 0;
        if (havoc_search::costLess(c0, best.cost))
        {
            take(0, c0);
            best.mv = mvQ;
            if (met)
            {
                ++calls;
                const uint64_t kd = quadMin(c >= 1 && c <= 4 ? (((uint64_t)cost << 4) | (uint32_t)c) : ~0ull);
                const uint64_t d = scalarMin(read64(kd, 0), read64(kd, 4));
                if (havoc_search::costLess((Cost)(d >> 4), best.cost))
                    take((int)(d & 15), (Cost)(d >> 4));
                else if (!hexagon)
                    ends = 1;
                else
                {   // the hexagon around the candidate as a step of its own (coding units of 32 and more whose diamond found nothing)
                    static constexpr Mv hexagonPattern[8] = {{0, -8}, {8, -4}, {8, 4}, {0, 8}, {-8, 4}, {-8, -4}, {-8, 4}, {-8, -4}};
                    calls += 2;
                    ends = patternRing(best.mv, hexagonPattern, 8, 1, 1, limit, pu, lambda, best) ? 0 : 1;
                }
            }
        }
        GAP_OUT();
        return ends;
    }
#endif

    // The raster refinement (Search.hpp:2268-2283): 25 x 28 (13 x 16 with the small window) positions five samples apart, all known before the first is
    // measured.  Every wavefront takes a quarter of the SADs, ONE exchange, then the candidates are costed 64 at a time and the first of the cheapest wins.
    __device__ __forceinline__ void rasterSweep(int rasterSearch, const havoc_search::LimitFullPelMv &limit, const havoc_search::PuContext &pu, const havoc_search::Lambda lambda,
                                                havoc_search::MvCandidate &best)
    {
        GAP_IN();
        const int rows = 2 * rasterSearch / 20 + 1, perRow = 4 * (2 * rasterSearch / 80 + 1), total = rows * perRow, first = -rasterSearch / 4;
        const FastDiv fr(perRow);
        for (int idx = wave; idx < total; idx += kWaves)
        {
            const int r = fr.div(idx), k = idx - r * perRow;
            const int mx = min(max(first + 5 * k, (int)limit.lo.x), (int)limit.hi.x), my = min(max(first + 5 * r, (int)limit.lo.y), (int)limit.hi.y);
            const int v = sadOne(mx, my, 0, 1);
            if (lane == 0) x->raster[idx] = v;
        }
        __syncthreads();
        uint64_t key = ~0ull;
        for (int idx = lane; idx < total; idx += kWave)
        {
            const int r = fr.div(idx), k = idx - r * perRow;
            const int px = min(max(first + 5 * k, (int)limit.lo.x), (int)limit.hi.x), py = min(max(first + 5 * r, (int)limit.lo.y), (int)limit.hi.y);
            int32_t mvdPacked;
            int second;
            const Cost cost = laneCost(px, py, pu, lambda, sadShift<S>(x->raster[idx]), mvdPacked, second);
            const uint64_t kk = ((uint64_t)cost << 10) | (uint32_t)idx;
            key = kk < key ? kk : key;
        }
        key = quadMin(key);
        uint64_t k = read64(key, 0);
#pragma unroll
        for (int l = 4; l < kWave; l += 4) k = scalarMin(k, read64(key, l));
        const Cost cw = (Cost)(k >> 10);
        if (havoc_search::costLess(cw, best.cost))
        {   // the winner's vector, predictor and difference again, in scalar registers (once)
            const int idx = (int)(k & 1023), r = fr.div(idx), kx = idx - r * perRow;
            Mv full(int16_t(first + 5 * kx), int16_t(first + 5 * r));
            limit(full);
            const havoc_search::MvCandidate again(havoc_search::shl2(full), pu.mvp, pu.mvpRate);
            best.cost = cw;
            best.mv = again.mv;
            best.mvd = again.mvd;
            best.mvpFlag = again.mvpFlag;
        }
        __syncthreads();      // x->raster is free again before anyone writes it (the next raster sweep is a whole search away, but the barrier is cheap here)
        GAP_OUT();
    }
    // searchMotionBi's exhaustive grid (Search.hpp:1583-1623): (2 range + 1)^2 candidates in raster order, every SAD already in x->table (hintSadRect).  The reference takes
    // them four columns at a time: the candidate of column x is the limited position of ITS column, its SAD the one taken (x - first column) samples right of the group's
    // limited first position.  A candidate per lane (every wavefront the whole grid: nothing to exchange), the first of the cheapest wins on strictly smaller cost.
    __device__ __forceinline__ bool biGrid(Mv origin, int range, const havoc_search::LimitFullPelMv &limit, const havoc_search::PuContext &pu, const havoc_search::Lambda lambda,
                                           havoc_search::MvCandidate &best)
    {
        if (!tw) return false;
        GAP_IN();
        const int side = 2 * range + 1, total = side * side;
        const FastDiv fs(side);
        const int ox = origin.x >> 2, oy = origin.y >> 2;
        const int lox = limit.lo.x, hix = limit.hi.x, loy = limit.lo.y, hiy = limit.hi.y;
        uint64_t key = 0x7fffffffffffffffull;      // lanes without a candidate (the 3 x 3 grid of the small window): beyond every cost, and non-negative for scalarMin
        bool ok = true;
        for (int idx = lane; idx < total; idx += kWave)
        {
            const int yy = fs.div(idx), xx = idx - yy * side, i = xx & 3;
            const int fy = min(max(oy + yy - range, loy), hiy);
            const int fx = min(max(ox + xx - range - i, lox), hix);                      // the group's first position, limited
            const int sx = i ? min(max(fx + i, lox), hix) : fx;                         // where this column's SAD is taken
            const int cx = i ? min(max(ox + xx - range, lox), hix) : fx;                // the candidate itself
            const bool in = sx >= tx0 && sx < tx0 + tw && fy >= ty0 && fy < ty0 + th;
            ok &= in;
            const int sadv = in ? x->table[(fy - ty0) * tw + sx - tx0] : 0;
            int32_t mvdPacked;
            int second;
            const Cost cost = laneCost(cx, fy, pu, lambda, sadv, mvdPacked, second);
            const uint64_t kk = ((uint64_t)cost << 8) | (uint32_t)idx;
            key = kk < key ? kk : key;
        }
        if (__builtin_amdgcn_ballot_w64(!ok) != 0)
        {   // a position outside the announced rectangle: the generic loops answer (every wavefront decides the same)
            GAP_OUT();
            return false;
        }
        key = quadMin(key);
        uint64_t k = read64(key, 0);
#pragma unroll
        for (int l = 4; l < kWave; l += 4) k = scalarMin(k, read64(key, l));
        const Cost cw = (Cost)(k >> 8);
        if (havoc_search::costLess(cw, best.cost))
        {
            const int idx = (int)(k & 255), yy = fs.div(idx), xx = idx - yy * side, i = xx & 3;
            Mv full(int16_t(ox + xx - range - i), int16_t(oy + yy - range));
            limit(full);
            if (i)
            {
                full = Mv(int16_t(ox + xx - range), int16_t(oy + yy - range));
                limit(full);
            }
            const havoc_search::MvCandidate again(havoc_search::shl2(full), pu.mvp, pu.mvpRate);
            best.cost = cw;
            best.mv = again.mv;
            best.mvd = again.mvd;
            best.mvpFlag = again.mvpFlag;
        }
        GAP_OUT();
        return true;
    }
#ifndef HAVOC_NO_SUBPEL_LANES
    // patternSearchOnce's costMv calls (Search.hpp:2001-2061, one iteration): the eight neighbours of `mv` at `scale` quarter samples in raster order (and `mv`
    // itself first when tryOrigin), a position per lane; returns the first of the cheapest neighbours if it beats the cost so far strictly, else -1
    __device__ __forceinline__ int subpelStep(Mv mv, Mv mvd, int scale, bool tryOrigin, const havoc_search::Lambda lambda, Cost &bestCost)
    {
        GAP_IN();
        Mv ask[9];
#pragma unroll
        for (int j = 0; j < 8; ++j)
        {
            const int g = j < 4 ? j : j + 1;
            ask[j] = Mv(int16_t(mv.x + (g % 3 - 1) * scale), int16_t(mv.y + (g / 3 - 1) * scale));
        }
        ask[8] = mv;
        satdTurn ^= 1;
        satdCount = 0;      // nothing is kept for satdQpel: the values are consumed here
        int32_t packed[9];
        computeSatds(ask, tryOrigin ? 9 : 8, packed);
        const int j = lane & 15, g = j < 4 ? j : j + 1;
        const Mv off = j < 8 ? Mv(int16_t((g % 3 - 1) * scale), int16_t((g / 3 - 1) * scale)) : Mv(0, 0);
        const int satdv = x->satd[satdTurn][j < 9 ? j : 0];
        const Cost cj = havoc_search::rateOf(mvd + off) + lambda * satdv;
        Cost start = bestCost;
        if (tryOrigin)
        {
            const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)cj, 8), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)cj >> 32), 8);
            start = (Cost)(((uint64_t)hi << 32) | lo);
        }
        const uint64_t key = quadMin(j < 8 ? (((uint64_t)cj << 4) | (uint32_t)j) : ~0ull);
        // (the built-in returns int: without the casts a low word of 2^31 or more -- costs of 64x64 blocks -- would sign-extend over the high word)
        const uint64_t k0 = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(key >> 32), 0) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key, 0);
        const uint64_t k1 = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(key >> 32), 4) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key, 4);
        const uint64_t k = havoc_search::costLess((Cost)k1, (Cost)k0) ? k1 : k0;      // keys are non-negative and never equal (the index is part of them)
        const Cost cmin = (Cost)(k >> 4);
        int bestI = -1;
        if (havoc_search::costLess(cmin, start))
        {
            start = cmin;
            bestI = (int)(k & 15);
        }
        bestCost = start;
        GAP_OUT();
        return bestI;
    }
#endif

    __device__ __forceinline__ int satdQpel(Mv mv)
    {
        GAP_IN();
        const int32_t k = havoc_search::MotionField::pack(mv);
#ifdef HAVOC_SEARCH_TIMING
        const long c0 = clock64();
#endif
        int v = -1;
#pragma unroll
        for (int i = 8; i >= 0; --i)
            if (i < satdCount && satdKey[i] == k) v = satdValue[i];
#ifdef HAVOC_SEARCH_TIMING
        acc[5] += clock64() - c0;
#endif
        GAP_OUT();
        if (v >= 0) return v;
        return wave_satd<S>(srcBase, srcPitch, predAt(mv), sbb, w, h, lane);      // not announced: every wavefront computes it
    }
};

// what a uni-directional search needs before its loops run: the view of (PU, list), the source block and a window of the reference picture
// around the start candidates of fullPel in LDS.  The caller's barrier follows.
template <int S>
__device__ __forceinline__ void stage_uni(const SearchArgs &a, Lds<S> &x, DeviceView<S> &view, const havoc_search::PuContext &pu, const int list,
                                          CtuStage<S> *cs = nullptr, CtuBox *box = nullptr)
{
    const int tid = threadIdx.x;
    const long sbb = a.refStride * S;
    const long at = (long)pu.y0 * a.refStride + pu.x0;
    view.ref = a.ref[list] + at * S;
    view.phase = a.phase[list] + at * S;
    view.sbb = sbb;
    view.planeBytes = a.planeElems * S;
    view.w = pu.w;
    view.h = pu.h;
    view.wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    view.lane = tid & 63;
    view.tid = tid;
    view.x = &x;
    {   // the window: the start candidates of fullPel (zero, the two predictors, the previous 2Nx2N vector) and a margin around them
        const havoc_search::LimitFullPelMv limit(pu, a.sp);
        int x0 = 0, x1 = 0, y0 = 0, y1 = 0;
        Mv first0;
        for (int k = 0; k < 3; ++k)
        {
            if (k == 2 && pu.part2Nx2N && pu.cqtDepth == 0) break;
            Mv m = k < 2 ? havoc_search::shr2(Mv(int16_t(pu.mvp[k].x + 1), int16_t(pu.mvp[k].y + 1))) : havoc_search::shr2(pu.mvPrevious2Nx2N);
            limit(m);
            if (k == 0) first0 = m;
            x0 = min(x0, (int)m.x); x1 = max(x1, (int)m.x);
            y0 = min(y0, (int)m.y); y1 = max(y1, (int)m.y);
        }
        if (((x1 - x0 + 2 * kWinMargin + pu.w) * S + 3) / 4 * 4 * (y1 - y0 + 2 * kWinMargin + pu.h) > kWinBytes * S)
        {   // too far apart: the first predictor's surroundings
            x0 = x1 = first0.x;
            y0 = y1 = first0.y;
        }
        view.bx0 = x0 - kWinMargin; view.bx1 = x1 + kWinMargin;
        view.by0 = y0 - kWinMargin; view.by1 = y1 + kWinMargin;
        if (cs && box)
        {   // the picture kernels: the CTU's source block is staged; its window too -- made around the first search's first start candidate
            view.srcBase = ldsPtr(cs->src) + ((pu.y0 - pu.yCtb) * 64 + (pu.x0 - pu.xCtb)) * S;
            view.srcPitch = 64 * S;
            if (!box->valid)
            {
                const int W = a.sp.picWidth, H = a.sp.picHeight;
                int X0 = pu.xCtb + first0.x - kCtuMargin, Y0 = pu.yCtb + first0.y - kCtuMargin;
                X0 = min(max(X0, -kPlaneReach), W + kPlaneReach - kCtuWinW);      // inside what every plane holds (pictures narrower than the window: see `fits`)
                Y0 = min(max(Y0, -kPlaneReach), H + kPlaneReach - kCtuWinW);
                box->X0 = X0; box->Y0 = Y0; box->X1 = X0 + kCtuWinW - 1; box->Y1 = Y0 + kCtuWinW - 1;
                box->valid = X0 >= -kPlaneReach && Y0 >= -kPlaneReach;
                if (box->valid)
                {
                    constexpr int chunks = kCtuWinW * S / 16;
                    const char *g = a.ref[list] + ((long)Y0 * a.refStride + X0) * S;
                    const FastDiv fc(chunks);
                    for (int i = tid; i < chunks * kCtuWinW; i += kThreads)
                    {
                        const int y = fc.div(i), k = i - y * chunks;
                        *reinterpret_cast<u32x4 *>(&cs->win[y * (kCtuWinW * S) + 16 * k]) = ld16(g + y * sbb + 16 * k);
                    }
                }
            }
            const bool fits = box->valid && pu.x0 + view.bx0 >= box->X0 && pu.x0 + view.bx1 + pu.w - 1 <= box->X1 && pu.y0 + view.by0 >= box->Y0 &&
                              pu.y0 + view.by1 + pu.h - 1 <= box->Y1;
            if (fits)
            {   // every displacement that keeps the block inside the CTU's window is answered from it
                view.bx0 = box->X0 - pu.x0; view.bx1 = box->X1 - pu.x0 - pu.w + 1;
                view.by0 = box->Y0 - pu.y0; view.by1 = box->Y1 - pu.y0 - pu.h + 1;
                view.wsB = kCtuWinW * S;
                view.winBase = ldsPtr(cs->win);
                return;
            }
        }
        const int rowB = (view.bx1 - view.bx0 + pu.w) * S, rowDw = (rowB + 3) / 4, nRows = view.by1 - view.by0 + pu.h;
        view.wsB = rowDw * 4;
        view.winBase = ldsPtr(x.win);
        const FastDiv fd(rowDw);
        const char *g = view.ref + view.by0 * sbb + (long)view.bx0 * S;
        uint32_t *win = reinterpret_cast<uint32_t *>(x.win);
        for (int i = tid; i < rowDw * nRows; i += kThreads)      // the last dword of a row may read up to 3 bytes past it: still inside the padded row
        {
            const int y = rowDw <= 128 ? fd.div(i) : i / rowDw, k = i - y * rowDw;
            win[i] = ld4(g + y * sbb + 4 * k);
        }
        if (cs && box) return;      // the source block is the CTU's
        view.srcBase = ldsPtr(x.src);
        view.srcPitch = pu.w * S;
        const int srcDw = pu.w * S / 4;
        const FastDiv fs(srcDw);
        const char *gs = a.src + ((long)pu.y0 * a.srcStride + pu.x0) * S;
        uint32_t *src = reinterpret_cast<uint32_t *>(x.src);
        for (int i = tid; i < srcDw * pu.h; i += kThreads)
        {
            const int y = fs.div(i), k = i - y * srcDw;
            src[i] = ld4(gs + y * a.srcStride * S + 4 * k);
        }
    }
}

// one CTU's searches in one list.  x.mv / x.valid [256 ..]: the cells left of and above the CTU, put there by the caller.  T (a compile-time choice: the kernels
// without a table are the code they were): each derivation also receives temporal[2 * p + list]
template <int S, bool T>
__device__ __forceinline__ void search_ctu(const SearchArgs &a, Lds<S> &x, CtuStage<S> &cs, const int list, const int cx, const int cy, Mv &mvPrev,
                                           const havoc_search::TemporalCand *temporal)
{
    const int c = cy * a.ctusX + cx, tid = threadIdx.x;
    const int ctb = a.sp.ctbSize, xCtb = cx * ctb, yCtb = cy * ctb;
    CtuBox box;
    {   // the CTU's source block (rows below / right of the picture's edge come from the plane's border: nothing reads them)
        constexpr int chunks = 64 * S / 16;
        const char *gs = a.src + ((long)yCtb * a.srcStride + xCtb) * S;
        for (int i = tid; i < chunks * 64; i += kThreads)
        {
            const int y = i / chunks, k = i - y * chunks;
            *reinterpret_cast<u32x4 *>(&cs.src[y * (64 * S) + 16 * k]) = ld16(gs + (long)y * a.srcStride * S + 16 * k);
        }
    }
    int32_t *field = a.field + (long)list * a.cw * a.ch;
    uint8_t *valid = a.valid + (long)list * a.cw * a.ch;
    auto get = [&](int, int px, int py, Mv *v) {
        const int rx = px - xCtb, ry = py - yCtb;
        int i;
        if (rx >= 0 && ry >= 0 && rx < 64 && ry < 64) i = (ry >> 2) * 16 + (rx >> 2);
        else if (rx >= -4 && rx < 0 && ry >= 0 && ry < 64) i = 256 + (ry >> 2);
        else if (ry >= -4 && ry < 0 && rx >= 0 && rx < 64) i = 272 + (rx >> 2);
        else if (ry >= -4 && ry < 0 && rx >= -4 && rx < 0) i = 288;      // B2 of a PU in the CTU's top-left corner
        else if (ry >= -4 && ry < 0 && rx >= 64 && rx < 68) i = 289;     // B0 of a PU at the CTU's top-right corner: the CTU above-right (done: the wavefront's lag)
        else
            return false;      // not a position a predictor of this CTU is read from
        if (!__builtin_amdgcn_readfirstlane((int)x.valid[i])) return false;
        *v = havoc_search::MotionField::unpack(__builtin_amdgcn_readfirstlane(x.mv[i]));
        return true;
    };
    const int first = a.ctuFirst[c], last = a.ctuFirst[c + 1];
    for (int p = first; p < last; ++p)
    {
#ifdef HAVOC_SEARCH_TIMING
        const long tTop = wall_clock64(), cTop = clock64();
#endif
        const havoc_picture_pu q = a.pus[p];
        Mv mvp[2];
        if constexpr (T)
        {   // p and list are the workgroup's: one 8-byte record, the same for every lane, kept in scalar registers like the cells `get` reads (no LDS, nothing indexed)
            const u32x2 raw = *reinterpret_cast<const u32x2 *>(temporal + (2 * p + list));
            const uint32_t lo = __builtin_amdgcn_readfirstlane(raw.x), hi = __builtin_amdgcn_readfirstlane(raw.y);
            havoc_search::TemporalCand cand;
            cand.mv[0] = int16_t(lo & 0xffff);
            cand.mv[1] = int16_t(lo >> 16);
            cand.available = int16_t(hi & 0xffff);
            cand.source = int16_t(hi >> 16);
            havoc_search::derivePredictors(q, list, ctb, a.sp.picWidth, a.sp.picHeight, get, mvp, &cand);
        }
        else
            havoc_search::derivePredictors(q, list, ctb, a.sp.picWidth, a.sp.picHeight, get, mvp);
        const havoc_search::PuContext pu = havoc_search::contextOf(q, ctb, mvp, a.mvpRate, mvPrev);
        DeviceView<S> view;
        stage_uni<S>(a, x, view, pu, list, &cs, &box);
        __syncthreads();
#ifdef HAVOC_SEARCH_TIMING
        const long tStaged = wall_clock64();
#endif
        havoc_search::MotionSearch<DeviceView<S>> search(a.sp, pu, view);
        const havoc_search::UniResult r = search.run();
#ifdef HAVOC_SEARCH_TIMING
        const long tEnd = wall_clock64(), cEnd = clock64();
#endif
        if (tid == 0)
        {
            havoc_search_result o;
            o.mv[0] = r.mv.x; o.mv[1] = r.mv.y;
            o.mvd[0] = r.mvd.x; o.mvd[1] = r.mvd.y;
            o.mv_integer[0] = r.mvInteger.x; o.mv_integer[1] = r.mvInteger.y;
            o.mvp_flag = (int16_t)r.mvpFlag;
            o.wrote_2Nx2N = r.wrote2Nx2N;
            o.calls = r.calls;
            o.replays = 0;
#ifdef HAVOC_SEARCH_TIMING
            o.replays = HAVOC_SEARCH_TIMING == 1 ? int(tEnd - tTop) : (HAVOC_SEARCH_TIMING == 2 ? int(tStaged - tTop) : (HAVOC_SEARCH_TIMING == 3 ? int(view.tHint - tStaged) : int(tEnd - view.tHint)));
            if (HAVOC_SEARCH_TIMING >= 5 && HAVOC_SEARCH_TIMING <= 10) o.replays = int(view.acc[HAVOC_SEARCH_TIMING - 5]);
            if (HAVOC_SEARCH_TIMING == 12) o.replays = int(view.acc[6]);
            if (HAVOC_SEARCH_TIMING == 13) o.replays = int(view.acc[7]) * 100;
            if (HAVOC_SEARCH_TIMING == 11) o.replays = int(cEnd - cTop);
#endif
            o.cost_integer = r.costInteger;
            o.cost_subpel = r.costSubPel;
            o.cost_mvd_zero[0] = r.costMvdZero[0];
            o.cost_mvd_zero[1] = r.costMvdZero[1];
            a.out[2 * p + list] = o;
            if (a.outBi)
            {   // the predictors this search ran with, for the refinement launched after the walk (k_search_bi overwrites the record with its result)
                havoc_search_result stash = havoc_search_result();
                stash.mv[0] = mvp[0].x; stash.mv[1] = mvp[0].y;
                stash.mvd[0] = mvp[1].x; stash.mvd[1] = mvp[1].y;
                a.outBi[2 * p + list] = stash;
            }
        }
        // "last decision covers the area": the PU's cells, in LDS for this CTU's later PUs and in the picture's field for other CTUs' (later launches)
        const int cw4 = q.w >> 2, cells = cw4 * (q.h >> 2);
        __syncthreads();      // every wavefront is past its reads of the cells, the window and the source block before they change
        if (tid < cells)
        {
            const int yy = tid / cw4, xx = tid - yy * cw4;
            const int gx = (q.x0 >> 2) + xx, gy = (q.y0 >> 2) + yy;
            const int32_t packed = havoc_search::MotionField::pack(r.mv);
            const int li = (gy - (yCtb >> 2)) * 16 + gx - (xCtb >> 2);
            x.mv[li] = packed;
            x.valid[li] = 1;
            if (gx < a.cw && gy < a.ch)
            {
                field[(long)gy * a.cw + gx] = packed;
                valid[(long)gy * a.cw + gx] = 1;
            }
        }
        __syncthreads();      // ... and the next PU's predictors are read from these cells by every wavefront
        if (r.wrote2Nx2N) mvPrev = r.mvInteger;
    }
    __syncthreads();
}

// n INDEPENDENT (PU, list) searches whose predictors, rates and previous vector are inputs (havoc_search_pu, search_abi.h): no chain, a workgroup
// per search, one launch -- what the launch + replay client havoc_search_motion_uni does in rounds.  One reference picture:
// a.ref[0] / a.phase[0].
template <int S>
__global__ __launch_bounds__(kThreads) void k_search_list(const SearchArgs a, const havoc_search_pu *__restrict__ pus)
{
    __shared__ Lds<S> x;
    const int i = blockIdx.x, tid = threadIdx.x;
    const havoc_search_pu q = pus[i];
    havoc_search::PuContext pu;
    pu.x0 = q.x0; pu.y0 = q.y0; pu.w = q.w; pu.h = q.h;
    pu.cuLog2Size = q.cu_log2_size;
    pu.cqtDepth = q.cqt_depth;
    pu.part2Nx2N = q.part_2Nx2N != 0;
    pu.xCtb = q.x_ctb; pu.yCtb = q.y_ctb;
    for (int k = 0; k < 2; ++k)
    {
        pu.mvp[k] = Mv(q.mvp[k][0], q.mvp[k][1]);
        pu.mvpRate[k] = q.mvp_rate[k];
    }
    pu.mvPrevious2Nx2N = Mv(q.mv_previous_2Nx2N[0], q.mv_previous_2Nx2N[1]);
    DeviceView<S> view;
    stage_uni<S>(a, x, view, pu, 0);
    __syncthreads();
    havoc_search::MotionSearch<DeviceView<S>> search(a.sp, pu, view);
    const havoc_search::UniResult r = search.run();
    if (tid == 0)
    {
        havoc_search_result o = havoc_search_result();
        o.mv[0] = r.mv.x; o.mv[1] = r.mv.y;
        o.mvd[0] = r.mvd.x; o.mvd[1] = r.mvd.y;
        o.mv_integer[0] = r.mvInteger.x; o.mv_integer[1] = r.mvInteger.y;
        o.mvp_flag = (int16_t)r.mvpFlag;
        o.wrote_2Nx2N = r.wrote2Nx2N;
        o.calls = r.calls;
        o.cost_integer = r.costInteger;
        o.cost_subpel = r.costSubPel;
        o.cost_mvd_zero[0] = r.costMvdZero[0];
        o.cost_mvd_zero[1] = r.costMvdZero[1];
        a.out[i] = o;
    }
}

// The bi-directional refinement of every PU in `list` (searchBi, turing/Search.hpp:1796-1827, the branch without mvd_l1_zero_flag): nothing of it
// feeds the walk above (the motion field keeps the uni-directional vectors), so it is not a chain: ONE launch per list after the walk, a
// workgroup per PU -- list 0 against the prediction from list 1's vector, then (next launch) list 1 against list 0's refined vector.
// one refinement: the workgroup builds the "ideal" block and the window in LDS and runs searchMotionBi; q = the PU, pu = its context (predictors, rates),
// `other` = the other list's vector (the prediction is read from a.phase[1 - list]), `start` = the refined list's vector
template <int S>
__device__ __forceinline__ havoc_search::BiResult bi_refine(const SearchArgs &a, Lds<S> &x, const int list, const int x0, const int y0, const int w, const int h,
                                                            const havoc_search::PuContext &pu, const Mv other, const Mv start)
{
    const int tid = threadIdx.x;
    const long sbb = a.refStride * S;
    DeviceView<S> view;
    const long at = (long)y0 * a.refStride + x0;
    view.ref = a.ref[list] + at * S;
    view.phase = a.phase[list] + at * S;
    view.sbb = sbb;
    view.planeBytes = a.planeElems * S;
    view.w = w;
    view.h = h;
    view.wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    view.lane = tid & 63;
    view.tid = tid;
    view.x = &x;
    const havoc_search::LimitFullPelMv limit(pu, a.sp);
    {   // the "ideal" second predictor clip(2 * source - prediction from the other list) takes the source block's place (Search.hpp:1519-1546)
        Mv full = havoc_search::shr2(other);
        limit(full);
        const char *pred = a.phase[1 - list] + (long)(4 * (other.y & 3) + (other.x & 3)) * a.planeElems * S + (((long)y0 + full.y) * a.refStride + x0 + full.x) * S;
        const char *gs = a.src + ((long)y0 * a.srcStride + x0) * S;
        const int srcDw = w * S / 4;
        const FastDiv fs(srcDw);
        uint32_t *ideal = reinterpret_cast<uint32_t *>(x.src);
        for (int i = tid; i < srcDw * h; i += kThreads)
        {
            const int y = fs.div(i), k = i - y * srcDw;
            const uint32_t sv = ld4(gs + y * a.srcStride * S + 4 * k), pv = ld4(pred + y * sbb + 4 * k);
            uint32_t o;
            if (S == 1)
            {   // SubtractBi with bitDepth = 6 + 2 * sizeof(Sample) = 8
                o = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b)
                {
                    const int v = 2 * (int)((sv >> (8 * b)) & 0xff) - (int)((pv >> (8 * b)) & 0xff);
                    o |= (uint32_t)clip3(0, 255, v) << (8 * b);
                }
            }
            else
            {   // bitDepth = 10 whatever the picture's
                const int v0 = 2 * (int)(sv & 0xffff) - (int)(pv & 0xffff), v1 = 2 * (int)(sv >> 16) - (int)(pv >> 16);
                o = (uint32_t)clip3(0, 1023, v0) | ((uint32_t)clip3(0, 1023, v1) << 16);
            }
            ideal[i] = o;
        }
        // the window: the 11 x 11 grid around the rounded start vector (and the three positions right of each, Search.hpp:1583-1603)
        Mv o0 = havoc_search::shr2(Mv(int16_t(start.x + 1), int16_t(start.y + 1)));
        limit(o0);
        view.bx0 = o0.x - kWinMargin; view.bx1 = o0.x + kWinMargin;
        view.by0 = o0.y - kWinMargin; view.by1 = o0.y + kWinMargin;
        const int rowB = (view.bx1 - view.bx0 + w) * S, rowDw = (rowB + 3) / 4, nRows = view.by1 - view.by0 + h;
        view.wsB = rowDw * 4;
        view.winBase = ldsPtr(x.win);
        view.srcBase = ldsPtr(x.src);
        view.srcPitch = w * S;
        const FastDiv fd(rowDw);
        const char *g = view.ref + view.by0 * sbb + (long)view.bx0 * S;
        uint32_t *win = reinterpret_cast<uint32_t *>(x.win);
        for (int i = tid; i < rowDw * nRows; i += kThreads)
        {
            const int y = rowDw <= 128 ? fd.div(i) : i / rowDw, k = i - y * rowDw;
            win[i] = ld4(g + y * sbb + 4 * k);
        }
    }
    __syncthreads();
    return havoc_search::searchMotionBi(a.sp, pu, view, start);
}

__device__ __forceinline__ havoc_search_result biRecord(const havoc_search::BiResult &b)
{
    havoc_search_result o = havoc_search_result();
    o.mv[0] = b.mv.x; o.mv[1] = b.mv.y;
    o.mvd[0] = b.mvd.x; o.mvd[1] = b.mvd.y;
    o.mvp_flag = (int16_t)b.mvpFlag;
    o.calls = b.calls;
    o.cost_subpel = b.cost;
    return o;
}

template <int S>
__global__ __launch_bounds__(kThreads) void k_search_bi(const SearchArgs a, const int list)
{
    __shared__ Lds<S> x;
    const int p = blockIdx.x, tid = threadIdx.x;
    const havoc_picture_pu q = a.pus[p];
    if (!havoc_search::biRefined(q))
    {
        if (tid == 0) a.outBi[2 * p + list] = havoc_search_result();
        return;
    }
    const havoc_search_result uni = a.out[2 * p + list], stash = a.outBi[2 * p + list];
    const havoc_search_result from = list == 0 ? a.out[2 * p + 1] : a.outBi[2 * p];
    const Mv mvp[2] = {Mv(stash.mv[0], stash.mv[1]), Mv(stash.mvd[0], stash.mvd[1])};
    const Mv other(from.mv[0], from.mv[1]), start(uni.mv[0], uni.mv[1]);
    const havoc_search::PuContext pu = havoc_search::contextOf(q, a.sp.ctbSize, mvp, a.mvpRate, Mv(0, 0));
    const havoc_search::BiResult b = bi_refine<S>(a, x, list, q.x0, q.y0, q.w, q.h, pu, other, start);
    if (tid == 0) a.outBi[2 * p + list] = biRecord(b);
}

// n INDEPENDENT refinements whose predictors, rates, other-list vector (havoc_search_pu::mv_other) and start vector are inputs: the list form of
// k_search_bi, as k_search_list is of the walk.  a.ref[0] / a.phase[0] = the refined list's picture, a.phase[1] = the other list's phase planes.
template <int S>
__global__ __launch_bounds__(kThreads) void k_search_bi_list(const SearchArgs a, const havoc_search_pu *__restrict__ pus, const int16_t *__restrict__ start)
{
    __shared__ Lds<S> x;
    const int i = blockIdx.x, tid = threadIdx.x;
    const havoc_search_pu q = pus[i];
    havoc_search::PuContext pu;
    pu.x0 = q.x0; pu.y0 = q.y0; pu.w = q.w; pu.h = q.h;
    pu.cuLog2Size = q.cu_log2_size;
    pu.cqtDepth = q.cqt_depth;
    pu.part2Nx2N = q.part_2Nx2N != 0;
    pu.xCtb = q.x_ctb; pu.yCtb = q.y_ctb;
    for (int k = 0; k < 2; ++k)
    {
        pu.mvp[k] = Mv(q.mvp[k][0], q.mvp[k][1]);
        pu.mvpRate[k] = q.mvp_rate[k];
    }
    const havoc_search::BiResult b = bi_refine<S>(a, x, 0, q.x0, q.y0, q.w, q.h, pu, Mv(q.mv_other[0], q.mv_other[1]), Mv(start[2 * i], start[2 * i + 1]));
    if (tid == 0) a.out[i] = biRecord(b);
}

// the cells left of and above CTU (cx, cy) from the picture's field (decided by earlier launches / by workgroups whose progress was awaited)
template <int S>
__device__ __forceinline__ void load_neighbours(const SearchArgs &a, Lds<S> &x, int list, int cx, int cy, bool left, bool top)
{
    const int tid = threadIdx.x;
    const int32_t *field = a.field + (long)list * a.cw * a.ch;
    const uint8_t *valid = a.valid + (long)list * a.cw * a.ch;
    if (tid < 34)
    {   // 0 .. 15: left of the CTU; 16 .. 31: above it; 32: above-left; 33: above-right (all of the row above are final: the CTU above-right is done before this one starts)
        const int gx = tid < 16 ? cx * 16 - 1 : (tid < 32 ? cx * 16 + tid - 16 : (tid == 32 ? cx * 16 - 1 : cx * 16 + 16));
        const int gy = tid < 16 ? cy * 16 + tid : cy * 16 - 1;
        const bool want = tid < 16 ? left : top;      // (the cell above-left belongs to the row above: loaded with it, whether or not the left column is kept in LDS)
        const bool in = gx >= 0 && gy >= 0 && gx < a.cw && gy < a.ch;
        if (want)      // (cells not asked for keep what they hold: the row walk hands a CTU's right column on as the next one's left neighbours)
        {
            x.mv[256 + tid] = in ? field[(long)gy * a.cw + gx] : 0;
            x.valid[256 + tid] = in ? valid[(long)gy * a.cw + gx] : 0;
        }
    }
}

// (a) one launch per wavefront step: the CTUs with cx + 2 cy == step
template <int S, bool T>
__global__ __launch_bounds__(kThreads) void k_search_step(const typename SearchArgsOf<T>::type a, const int step, const int yLo)
{
    __shared__ Lds<S> x;
    __shared__ CtuStage<S> cs;
    const int list = blockIdx.x & 1, cy = yLo + (blockIdx.x >> 1), cx = step - 2 * cy, tid = threadIdx.x;
    if (tid < 256)
    {
        x.mv[tid] = 0;
        x.valid[tid] = 0;
    }
    load_neighbours<S>(a, x, list, cx, cy, true, true);
    __syncthreads();
    Mv mvPrev = cx ? havoc_search::MotionField::unpack(a.rowPrev[2 * cy + list]) : Mv(0, 0);
    search_ctu<S, T>(a, x, cs, list, cx, cy, mvPrev, temporalOf(a));
    if (tid == 0) a.rowPrev[2 * cy + list] = havoc_search::MotionField::pack(mvPrev);
}

// (b) one launch per picture: a workgroup per (CTU row, list) walks its row and waits for the row above to be two CTUs ahead (the WPP rule) on a
// progress counter in memory -- no barrier across the picture per step, so a heavy CTU delays only what depends on it.  Rows are handed out
// by a ticket in the order workgroups START, so a row only ever waits for workgroups that are already running.  A wait that does not end
// (it cannot, short of a fault elsewhere) gives up after kSpinLimit polls and raises a flag the host reads: nothing hangs.
constexpr int kSpinLimit = 1 << 22;

template <int S, bool T>
__global__ __launch_bounds__(kThreads) void k_search_rows(const typename SearchArgsOf<T>::type a)
{
    __shared__ Lds<S> x;
    __shared__ CtuStage<S> cs;
    __shared__ int shared;
    const int tid = threadIdx.x;
    if (tid == 0) shared = atomicAdd(a.ticket, 1);
    __syncthreads();
    const int t = shared, list = t & 1, cy = t >> 1;
    if (cy >= a.ctusY) return;
    int *progress = a.progress + 2 * cy + list;
    const int *above = a.progress + 2 * (cy - 1) + list;
    if (a.rowsReady)
    {   // The reference picture is still arriving (TaskEncodeSubstream.cpp:71-95: a CTU waits until its reference is reconstructed 3 rows below).  With frames encoded
        // concurrently the vectors of this CTU row are limited to blocks that end above row yCtb + 2 * ctb - 15 (decision.hpp: LimitFullPelMv, the reference's
        // howCloseDoYouDare), so rows [0, (cy + 2) * ctb) of the picture and of its 15 fractional planes are all this row reads; the last rows reach the bottom border.
        __syncthreads();      // (every thread has read its ticket from `shared`)
        if (tid == 0)
        {
            const int ctb = a.sp.ctbSize, need = min((cy + 2) * ctb, a.sp.picHeight + ctb + 8);
            int spins = 0, ok = 1;
            while (__hip_atomic_load(a.rowsReady + list, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < need)
            {
                __builtin_amdgcn_s_sleep(64);
                if (++spins > kSpinLimit || __hip_atomic_load(a.gaveUp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                {
                    ok = 0;
                    break;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            shared = ok;
        }
        __syncthreads();
        if (!shared)
        {
            if (tid == 0)
            {
                atomicOr(a.gaveUp, 1);
                __hip_atomic_store(progress, a.ctusX, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            }
            return;
        }
        __syncthreads();
    }
    Mv mvPrev(0, 0);
    if (tid < 256)
    {
        x.mv[tid] = 0;
        x.valid[tid] = 0;
    }
    if (tid < 36)
    {
        x.mv[256 + tid] = 0;
        x.valid[256 + tid] = 0;
    }
    __syncthreads();
    for (int cx = 0; cx < a.ctusX; ++cx)
    {
        if (cy > 0)
        {
            if (tid == 0)
            {
                const int need = cx + a.rowLag < a.ctusX ? cx + a.rowLag : a.ctusX;
                int spins = 0, ok = 1;
                // polled relaxed (an acquire per poll would invalidate this XCD's caches every quarter microsecond for as long as the row waits --
                // and rows wait most of the time); ONE acquire fence once the row above is far enough
                while (__hip_atomic_load(above, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < need)
                {
                    __builtin_amdgcn_s_sleep(32);
                    if (++spins > kSpinLimit || __hip_atomic_load(a.gaveUp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                    {
                        ok = 0;
                        break;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                shared = ok;
            }
            __syncthreads();
            if (!shared)
            {   // the whole workgroup leaves; the rows below are let through (their results mean nothing: the host sees the flag)
                if (tid == 0)
                {
                    atomicOr(a.gaveUp, 1);
                    __hip_atomic_store(progress, a.ctusX, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                }
                return;
            }
        }
        load_neighbours<S>(a, x, list, cx, cy, false, true);      // the cells above, now final; the cells to the left were kept below
        __syncthreads();
        search_ctu<S, T>(a, x, cs, list, cx, cy, mvPrev, temporalOf(a));
        // this CTU's right column becomes the next one's left neighbours; its own cells start undecided
        const int32_t keepMv = tid < 16 ? x.mv[tid * 16 + 15] : 0;
        const uint8_t keepValid = tid < 16 ? x.valid[tid * 16 + 15] : 0;
        __syncthreads();
        if (tid < 256)
        {
            x.mv[tid] = 0;
            x.valid[tid] = 0;
        }
        if (tid < 16)
        {
            x.mv[256 + tid] = keepMv;
            x.valid[256 + tid] = keepValid;
        }
#if HAVOC_SEARCH_FENCE_ALL
        __threadfence();
#endif
        // the field cells every wavefront wrote are ordered before the barrier (a workgroup-scope release / acquire), and the one agent-scope
        // release below is cumulative over them: one write-back of the L2 per CTU instead of one per wavefront
        __syncthreads();
        if (tid == 0) __hip_atomic_store(progress, cx + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the walk's launches: one (rows wait for each other in the kernel), or -- stepLaunches -- ctusX + 2 * (ctusY - 1) on the stream
template <bool T>
hipError_t launch_walk(hipStream_t st, int S, const typename SearchArgsOf<T>::type &a, int stepLaunches)
{
    const int ctusX = a.ctusX, ctusY = a.ctusY;
    if (!stepLaunches)
    {
        hipLaunchKernelGGL((S == 1 ? k_search_rows<1, T> : k_search_rows<2, T>), dim3(2 * ctusY), dim3(kThreads), 0, st, a);
        return hipGetLastError();
    }
    for (int step = 0; step <= ctusX - 1 + 2 * (ctusY - 1); ++step)
    {
        const int yLo = step > ctusX - 1 ? (step - (ctusX - 1) + 1) / 2 : 0, yHi = step / 2 < ctusY - 1 ? step / 2 : ctusY - 1;
        if (yHi < yLo) continue;
        const dim3 grid(2 * (yHi - yLo + 1));
        hipLaunchKernelGGL((S == 1 ? k_search_step<1, T> : k_search_step<2, T>), grid, dim3(kThreads), 0, st, a, step, yLo);
    }
    return hipGetLastError();
}

} // namespace

#ifdef HAVOC_SEARCH_TEMPORAL_UNIT
// kernels_search_temporal.hip: this file once more, for the walk kernels that read a table of temporal candidates and nothing else.  A translation unit of their own:
// compiled beside them, the kernels without a table came out of the compiler as different code (DESIGN.md f2^11) -- apart, they are the instructions they were.
hipError_t launch_search_walk_temporal(hipStream_t st, int S, const void *searchArgs, const void *temporal, int stepLaunches)
{
    SearchArgsTemporal at;
    static_cast<SearchArgs &>(at) = *static_cast<const SearchArgs *>(searchArgs);
    at.temporal = static_cast<const havoc_search::TemporalCand *>(temporal);
    return launch_walk<true>(st, S, at, stepLaunches);
}
#else

hipError_t launch_search_list(hipStream_t st, int S, const havoc_mi355x_search_params *sp, const void *src, long srcOrigin, long srcStride, const void *ref, long refOrigin,
                              long refStride, const void *phase, long planeElems, long phaseOrigin, const void *pus, int n, void *out)
{
    if (n <= 0) return hipSuccess;
    SearchArgs a = SearchArgs();
    a.sp.picWidth = sp->pic_width;
    a.sp.picHeight = sp->pic_height;
    a.sp.ctbSize = sp->ctb_size;
    a.sp.concurrentFrames = sp->concurrent_frames;
    a.sp.met = sp->met != 0;
    a.sp.smallSearchWindow = sp->small_search_window != 0;
    a.sp.biSmallSearchWindow = sp->bi_small_search_window != 0;
    a.sp.halfPel = sp->half_pel != 0;
    a.sp.quarterPel = sp->quarter_pel != 0;
    a.sp.reciprocalSqrtLambda = sp->reciprocal_sqrt_lambda;
    a.sp.bitDepth = sp->bit_depth;
    a.src = static_cast<const char *>(src) + srcOrigin * S;
    a.ref[0] = a.ref[1] = static_cast<const char *>(ref) + refOrigin * S;
    a.phase[0] = a.phase[1] = static_cast<const char *>(phase) + phaseOrigin * S;
    a.srcStride = srcStride;
    a.refStride = refStride;
    a.planeElems = planeElems;
    a.out = static_cast<havoc_search_result *>(out);
    if (S == 1)
        hipLaunchKernelGGL(k_search_list<1>, dim3(n), dim3(kThreads), 0, st, a, static_cast<const havoc_search_pu *>(pus));
    else
        hipLaunchKernelGGL(k_search_list<2>, dim3(n), dim3(kThreads), 0, st, a, static_cast<const havoc_search_pu *>(pus));
    return hipGetLastError();
}

hipError_t launch_search_bi_list(hipStream_t st, int S, const havoc_mi355x_search_params *sp, const void *src, long srcOrigin, long srcStride, const void *ref,
                                 long refOrigin, long refStride, const void *phase, long planeElems, long phaseOrigin, const void *phaseOther, long phaseOtherOrigin,
                                 const void *pus, const int16_t *start, int n, void *out)
{
    if (n <= 0) return hipSuccess;
    SearchArgs a = SearchArgs();
    a.sp.picWidth = sp->pic_width;
    a.sp.picHeight = sp->pic_height;
    a.sp.ctbSize = sp->ctb_size;
    a.sp.concurrentFrames = sp->concurrent_frames;
    a.sp.met = sp->met != 0;
    a.sp.smallSearchWindow = sp->small_search_window != 0;
    a.sp.biSmallSearchWindow = sp->bi_small_search_window != 0;
    a.sp.halfPel = sp->half_pel != 0;
    a.sp.quarterPel = sp->quarter_pel != 0;
    a.sp.reciprocalSqrtLambda = sp->reciprocal_sqrt_lambda;
    a.sp.bitDepth = sp->bit_depth;
    a.src = static_cast<const char *>(src) + srcOrigin * S;
    a.ref[0] = a.ref[1] = static_cast<const char *>(ref) + refOrigin * S;
    a.phase[0] = static_cast<const char *>(phase) + phaseOrigin * S;
    a.phase[1] = static_cast<const char *>(phaseOther) + phaseOtherOrigin * S;
    a.srcStride = srcStride;
    a.refStride = refStride;
    a.planeElems = planeElems;
    a.out = static_cast<havoc_search_result *>(out);
    if (S == 1)
        hipLaunchKernelGGL(k_search_bi_list<1>, dim3(n), dim3(kThreads), 0, st, a, static_cast<const havoc_search_pu *>(pus), start);
    else
        hipLaunchKernelGGL(k_search_bi_list<2>, dim3(n), dim3(kThreads), 0, st, a, static_cast<const havoc_search_pu *>(pus), start);
    return hipGetLastError();
}

size_t search_workspace_bytes(int width, int height)
{
    const size_t cells = (size_t)((width + 3) / 4) * ((height + 3) / 4);
    // validity of the two lists' cells | the rows' mvPreviousInteger2Nx2N, their progress | ticket, "a wait gave up" (the last 8 bytes)
    return ((2 * cells + 255) & ~(size_t)255) + 16 * (size_t)((height + 63) / 64) + 16;
}

// ---- a launch that ends when CTU rows 0 .. rowHi of BOTH lists of the picture search in `work` are done (k_search_rows' progress counters): what is queued behind it on
// its stream -- the band's merge candidates, predictions, transform trees, deblocking (decisions.py: step_banded) -- then runs while the rows below are still searched.
// The stream must not be the search's, nor share its hardware queue (another priority).
__global__ __launch_bounds__(64) void k_wait_rows(const int *progress, int rowHi, int ctusX, const int *searchGaveUp, int *gaveUp)
{
    if (threadIdx.x != 0) return;
    int spins = 0;
    for (int r = 0; r <= rowHi; ++r)
        for (int l = 0; l < 2; ++l)
            while (__hip_atomic_load(progress + 2 * r + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < ctusX)
            {
                __builtin_amdgcn_s_sleep(64);
                if (++spins > kSpinLimit || __hip_atomic_load(searchGaveUp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                {
                    atomicOr(gaveUp, 1);
                    return;
                }
            }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

hipError_t launch_search_wait_rows(hipStream_t st, const void *work, int width, int height, int rowHi, int *gaveUp)
{
    const size_t cells = (size_t)((width + 3) / 4) * ((height + 3) / 4);
    const int ctusX = (width + 63) / 64, ctusY = (height + 63) / 64;
    const int32_t *rowPrev = reinterpret_cast<const int32_t *>(static_cast<const char *>(work) + ((2 * cells + 255) & ~(size_t)255));      // (launch_search_picture_uni's layout)
    const int *progress = rowPrev + 2 * ctusY, *ticket = progress + 2 * ctusY + 2;
    hipLaunchKernelGGL(k_wait_rows, dim3(1), dim3(64), 0, st, progress, rowHi < ctusY - 1 ? rowHi : ctusY - 1, ctusX, ticket + 1, gaveUp);
    return hipGetLastError();
}

static hipError_t launch_bi(hipStream_t st, int S, const SearchArgs &a, int nPus)
{
    if (a.outBi && nPus > 0)
        for (int list = 0; list < 2; ++list)
        {
            if (S == 1)
                hipLaunchKernelGGL(k_search_bi<1>, dim3(nPus), dim3(kThreads), 0, st, a, list);
            else
                hipLaunchKernelGGL(k_search_bi<2>, dim3(nPus), dim3(kThreads), 0, st, a, list);
        }
    return hipGetLastError();
}

// the whole picture: the zeroed workspace and field, the walk (launch_walk), the refinement launches
static_assert(sizeof(havoc_mi355x_search_params) == sizeof(havoc_search_params) && sizeof(havoc_search_params) == 48, "search ABI");

hipError_t launch_search_picture_uni(hipStream_t st, int S, const havoc_mi355x_search_params *sp, const int64_t mvpRate[2], const void *src, long srcOrigin, long srcStride,
                                     const void *ref, const long refOrigin[2], long refStride, const void *phase, long planeElems, const long phaseOrigin[2], const void *pus,
                                     const int32_t *ctuFirst, int ctusX, int ctusY, int nPus, void *out, void *outBi, int16_t *field, void *work, int stepLaunches,
                                     const int32_t *rowsReady, const void *temporal)
{
    SearchArgs a;
    a.rowsReady = rowsReady;
    a.sp.picWidth = sp->pic_width;
    a.sp.picHeight = sp->pic_height;
    a.sp.ctbSize = sp->ctb_size;
    a.sp.concurrentFrames = sp->concurrent_frames;
    a.sp.met = sp->met != 0;
    a.sp.smallSearchWindow = sp->small_search_window != 0;
    a.sp.biSmallSearchWindow = sp->bi_small_search_window != 0;
    a.sp.halfPel = sp->half_pel != 0;
    a.sp.quarterPel = sp->quarter_pel != 0;
    a.sp.reciprocalSqrtLambda = sp->reciprocal_sqrt_lambda;
    a.sp.bitDepth = sp->bit_depth;
    a.mvpRate[0] = mvpRate[0];
    a.mvpRate[1] = mvpRate[1];
    a.src = static_cast<const char *>(src) + srcOrigin * S;
    for (int l = 0; l < 2; ++l)
    {
        a.ref[l] = static_cast<const char *>(ref) + refOrigin[l] * S;
        a.phase[l] = static_cast<const char *>(phase) + phaseOrigin[l] * S;
    }
    a.srcStride = srcStride;
    a.refStride = refStride;
    a.planeElems = planeElems;
    a.pus = static_cast<const havoc_picture_pu *>(pus);
    a.ctuFirst = ctuFirst;
    a.ctusX = ctusX;
    a.ctusY = ctusY;
    a.cw = (sp->pic_width + 3) / 4;
    a.ch = (sp->pic_height + 3) / 4;
    a.out = static_cast<havoc_search_result *>(out);
    a.outBi = static_cast<havoc_search_result *>(outBi);
    a.field = reinterpret_cast<int32_t *>(field);
    const size_t cells = (size_t)a.cw * a.ch;
    a.valid = static_cast<uint8_t *>(work);
    a.rowPrev = reinterpret_cast<int32_t *>(static_cast<char *>(work) + ((2 * cells + 255) & ~(size_t)255));
    a.progress = a.rowPrev + 2 * ctusY;
    a.ticket = a.progress + 2 * ctusY + 2;
    a.gaveUp = a.ticket + 1;
    // The reference's wavefront rule (TaskEncodeSubstream.cpp:71-95): since round 5 a REQUIREMENT of the data, not only of the rule -- the derivation of the predictors
    // (picture_order.hpp: the reference's five spatial candidates) reads the cell above-right of a CTU (B0).  (Round 4's derivation had no above-right candidate and
    // HAVOC_SEARCH_ROW_LAG=1 was a legal diagnostic: 13.5 -> 10.6 ms per 1080p picture, profiles/r04/row_lag_diagnostic.json; it no longer is and is ignored.)
    a.rowLag = 2;
    hipError_t e = hipMemsetAsync(work, 0, search_workspace_bytes(sp->pic_width, sp->pic_height), st);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(field, 0, 2 * cells * 4, st)) != hipSuccess) return e;
    // with a table of temporal candidates: the kernels that read it (kernels_search_temporal.hip); without one, the kernels that do not know of it
    e = temporal ? launch_search_walk_temporal(st, S, &a, temporal, stepLaunches) : launch_walk<false>(st, S, a, stepLaunches);
    if (e != hipSuccess) return e;
    return launch_bi(st, S, a, nPus);
}

#endif

} // namespace havoc_gpu
