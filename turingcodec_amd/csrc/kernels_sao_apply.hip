// In-loop SAO of a picture (the last step of the SAO third): what the encoder's TaskSao leaves in a picture before it
// is padded and becomes a reference (turing/TaskSao.cpp:96-121 -> LoopFilter::Picture::applySaoCTU -> filterBlockSao, LoopFilter.h:
// 795-811, 886-1008), with the parameters havoc_mi355x_sao_decide chose.  Unlike the measuring filter of sao_ctu.h (computeSaoDistortion's
// form), this one keeps the reference's availability rules: an edge-offset sample whose neighbour CTU is not available (picture edge,
// slice edge without slice_loop_filter_across_slices_enabled_flag) goes back to the deblocked value through filterBlockSao's
// undoT / undoL / undoR / undoB counters, and restoreUnfilteredRegions copies back the regions where the loop filter is disabled.
//
// One 256-thread workgroup per CTU does Y, Cb and Cr.  The CTU's decision record and bounds are read once (wave-uniform), the offset
// tables of sao_ctu.h go to LDS; a lane takes 4 horizontally adjacent samples, loaded and stored as one dword / 8 bytes when the plane
// allows it, and its neighbours through L1 (row above and below, one sample either side, clamped into the picture: only samples the
// reference restores ever see a clamped neighbour).  The restore decision is a predicate of the lane's position and the CTU's uniform
// counters.  Nothing outside the picture is read or written.
#include "launch.h"
#include "sao_ctu.h"

namespace havoc_gpu {

namespace {

struct SaoApplyArgs
{
    const char *rec[3];
    char *dst[3];
    long rs[2], ds[2];                       // row strides in samples: [0] luma, [1] chroma
    const havoc_mi355x_sao_decision *decisions;
    const havoc_mi355x_sao_bounds *bounds;                 // null: one slice, one tile
    const int8_t *block_data;                // null: no disabled regions
    long block_stride;
    int width, height, log2, ctus_x, nctus, bd, flags;
};

template <typename T>
__device__ __forceinline__ void load4(const T *p, bool vec, int v[4])
{
    if (vec && sizeof(T) == 1)
    {
        const uint32_t w = *reinterpret_cast<const uint32_t *>(p);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (w >> (8 * k)) & 0xff;
    }
    else if (vec)
    {
        const uint2 w = *reinterpret_cast<const uint2 *>(p);
        v[0] = w.x & 0xffff, v[1] = w.x >> 16, v[2] = w.y & 0xffff, v[3] = w.y >> 16;
    }
    else
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = p[k];
}

template <typename T>
__device__ __forceinline__ void store4(T *p, bool vec, const int v[4])
{
    if (vec && sizeof(T) == 1)
        *reinterpret_cast<uint32_t *>(p) = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
    else if (vec)
        *reinterpret_cast<uint2 *>(p) = make_uint2((uint32_t)v[0] | (uint32_t)v[1] << 16, (uint32_t)v[2] | (uint32_t)v[3] << 16);
    else
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = (T)v[k];
}

// samples x - 1 .. x + 4 of a row, the outer two clamped into [0, pw)
template <typename T>
__device__ __forceinline__ void load6(const T *row, int x, int pw, bool vec, int v[6])
{
    v[0] = row[max(x - 1, 0)];
    load4(row + x, vec, v + 1);
    v[5] = row[min(x + 4, pw - 1)];
}

template <int S>
__global__ __launch_bounds__(256) void k_sao_apply(const SaoApplyArgs a)
{
    typedef typename Sample<S>::T T;
    __shared__ int16_t table[2][32];
    const int tid = threadIdx.x, ctu = xcd_block(blockIdx.x, gridDim.x);
    const int rx = ctu % a.ctus_x, ry = ctu / a.ctus_x, ctb = 1 << a.log2;
    const havoc_mi355x_sao_decision &dec = a.decisions[ctu];
    sao_offset_table(table, dec.comp, tid, a.bd);
    // LoopFilter::Ctu of one slice and one tile when no bounds are given: only the picture's edges are unavailable
    havoc_mi355x_sao_bounds b;
    if (a.bounds)
        b = a.bounds[ctu];
    else
    {
        const int last_x = rx == a.ctus_x - 1, last_y = ry == a.nctus / a.ctus_x - 1;
        b.left = 0, b.top = 0, b.right = a.width, b.bottom = a.height;
        b.corners = (rx > 0 && ry > 0) | (!last_x && ry > 0) << 1 | (rx > 0 && !last_y) << 2 | (!last_x && !last_y) << 3;
    }
    __syncthreads();
    const int mx = (1 << a.bd) - 1;
    for (int plane = 0; plane < 3; ++plane)
    {
        const int sub = plane ? 1 : 0, ci = sub;
        const int n = ctb >> sub, pw = a.width >> sub, ph = a.height >> sub;
        const int x0 = rx * n, y0 = ry * n, bw = min(n, pw - x0), bh = min(n, ph - y0), groups = (bw >> 2) * bh;
        const long rs = a.rs[sub], ds = a.ds[sub];
        const T *rec = reinterpret_cast<const T *>(a.rec[plane]);
        T *dst = reinterpret_cast<T *>(a.dst[plane]);
        const bool vec = ((reinterpret_cast<uintptr_t>(rec) | reinterpret_cast<uintptr_t>(dst)) & (4 * S - 1)) == 0 && ((rs | ds) & 3) == 0;
        // Ctu::set: SaoTypeIdx 0 where the slice flag is off; a record that is not a decision is all off
        const int type = ((a.flags >> ci) & 1) && dec.decided == 1 ? dec.comp[ci].type : 0;
        const int e = dec.comp[ci].eo_class & 3;
        const int16_t *tb = table[ci];

        // filterBlockSao's undo counters (LoopFilter.h:913-975), for the edge type only
        int undoT = 0, undoL = 0, undoR = 0, undoB = 0, right = 0, bottom = 0;
        if (type == 2)
        {
            const int top = b.top >> sub, left = b.left >> sub;
            right = b.right >> sub, bottom = b.bottom >> sub;
            const bool availableL = left < x0, availableR = right > x0 + n, availableT = top < y0, availableB = bottom > y0 + n;
            const bool availableTL = b.corners & 1, availableTR = b.corners & 2, availableBL = b.corners & 4, availableBR = b.corners & 8;
            if (e == 2)
            {
                if (!availableTL) ++undoT, ++undoL;
                if (!availableBR) ++undoR, ++undoB;
            }
            if (e != 1)
            {
                if (!availableL) undoL = n;
                if (!availableR) undoR = n;
            }
            if (e != 0)
            {
                if (!availableT) undoT = n;
                if (!availableB) undoB = n;
            }
            if (e == 3)
            {
                if (availableTR) --undoT, --undoR;
                if (availableBL) --undoL, --undoB;
            }
            right = min(right, x0 + n);
            bottom = min(bottom, y0 + n);
        }
        // neighbours of the edge class (sao.cpp:63-73): horizontal, vertical, 135 degrees, 45 degrees
        const int dxa = e == 1 ? 0 : (e == 3 ? 1 : -1), dya = e == 0 ? 0 : -1;

        for (int g = tid; g < groups; g += 256)
        {
            const int j = g / (bw >> 2), i = (g - j * (bw >> 2)) << 2, x = x0 + i, y = y0 + j;
            const T *r = rec + y * rs + x;
            int c[4], o[4];
            load4(r, vec, c);
            if (type == 1)
            {
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = min(max(c[k] + tb[c[k] >> (a.bd - 5)], 0), mx);
            }
            else if (type == 2)
            {
                int na[6], nb[6];
                load6(rec + clip3(0, ph - 1, y + dya) * rs, x, pw, vec, na);
                load6(rec + clip3(0, ph - 1, y - dya) * rs, x, pw, vec, nb);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                {
                    int idx = 2 + sign3(c[k] - na[1 + k + dxa]) + sign3(c[k] - nb[1 + k - dxa]);
                    idx = idx > 2 ? idx : (idx == 2 ? 0 : idx + 1);
                    o[k] = min(max(c[k] + tb[idx], 0), mx);
                    // the undo copies (LoopFilter.h:982-985) at positions right - 1 and bottom - 1 after clamping
                    const int ii = i + k, xx = x + k;
                    if ((j == 0 && ii < undoT) || (ii == 0 && j < undoL) || (xx == right - 1 && j >= n - undoR) || (y == bottom - 1 && ii >= n - undoB))
                        o[k] = c[k];
                }
            }
            else
            {
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = c[k];
            }
            // restoreUnfilteredRegions (LoopFilter.h:850-877): the lane's 4 samples lie in one 8x8 luma region
            if (type && a.block_data && (a.block_data[(long)((y << sub) >> 3) * a.block_stride + ((x << sub) >> 3)] & 1))
            {
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = c[k];
            }
            store4(dst + y * ds + x, vec, o);
        }
    }
}

} // namespace

hipError_t launch_sao_apply(hipStream_t st, int S, int bitDepth, int flags, int width, int height, int log2, const void *rec_y, const void *rec_cb,
                            const void *rec_cr, long rsy, long rsc, void *dst_y, void *dst_cb, void *dst_cr, long dsy, long dsc, const havoc_mi355x_sao_decision *decisions,
                            const havoc_mi355x_sao_bounds *bounds, const int8_t *block_data, long block_stride)
{
    SaoApplyArgs a;
    a.rec[0] = static_cast<const char *>(rec_y), a.rec[1] = static_cast<const char *>(rec_cb), a.rec[2] = static_cast<const char *>(rec_cr);
    a.dst[0] = static_cast<char *>(dst_y), a.dst[1] = static_cast<char *>(dst_cb), a.dst[2] = static_cast<char *>(dst_cr);
    a.rs[0] = rsy, a.rs[1] = rsc, a.ds[0] = dsy, a.ds[1] = dsc;
    a.decisions = decisions;
    a.bounds = bounds;
    a.block_data = block_data;
    a.block_stride = block_stride;
    a.width = width, a.height = height, a.log2 = log2, a.bd = bitDepth, a.flags = flags;
    a.ctus_x = (width + (1 << log2) - 1) >> log2;
    a.nctus = a.ctus_x * ((height + (1 << log2) - 1) >> log2);
    if (S == 1) hipLaunchKernelGGL(k_sao_apply<1>, dim3(a.nctus), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_sao_apply<2>, dim3(a.nctus), dim3(256), 0, st, a);
    return hipGetLastError();
}

} // namespace havoc_gpu
