// k_cqt_decide: the coding quadtree of every CTU of a picture -- Search<coding_quadtree>::go (turing/Search.hpp:709-887, the decision :808-886) over
// Syntax<coding_quadtree>::go (turing/SyntaxCtu.hpp:95-139) and the writer of split_cu_flag (turing/Binarization.h:102-122) -- over the closed coding units
// havoc_mi355x_cu_close left on the device.  DESIGN 7, row f2^6; the decision itself is restated in search/cqt_decision.hpp (decideCqt), which this file follows
// line by line.
//
// The walk of a CTU is a dependent chain: at most 85 nodes (CTB 64, MinCb 8), each visited at most once -- a node belongs to exactly one parent's split candidate --
// with two context-coded bins.  CTUs chain too: split_cu_flag's ctxInc reads the decided depth of the left and upper neighbours across CTU borders, and its three
// contexts flow from CTU to CTU under the WPP rule.  So the form is k_sao_merge_rows': one workgroup per CTU row, rows taken by ticket in the order workgroups start
// (a row only ever waits for a running workgroup); without WPP one workgroup walks the whole picture.  A workgroup is two wavefronts:
//   wave 0  lane 0 walks CTU x: the (state, bin) -> (state, rate) table of cabac_tables.h in LDS, the three contexts in one register, the CTU's CtDepth cells (eight
//           64-bit rows of a byte per MinCb cell), its node inputs and its node records in LDS.  The recursion has the depth as a template parameter (four levels);
//           nothing is indexed dynamically in private memory.  Then all 64 lanes mark the decided tree, and write the node records, the CtDepth cells (plain vector
//           stores), the CTU record and the snapshot; lane 0 publishes ONE 64-bit word (done, the three context states) with an agent-scope release store.
//   wave 1  meanwhile stages CTU x + 1: follows every node's index to its havoc_mi355x_cu_choice record (outcome, rate, lambda_distortion), marks the nodes that
//           have a candidate somewhere below them, waits -- bounded -- for
//           the word of CTU max(x + 1, min(1, cx - 1)) of the row above (the upper depths come from CTU x + 1, the row's start contexts from CTU 1), and reads the
//           upper neighbours' CtDepth from the picture's map behind an acquire fence.  This keeps every global load off the chain.
// A wait that gives up raises the give-up word; the rows below are let through and k_cqt_finish clears `decided` in every record of the call.
// k_cqt_commit (below, with its own comment) acts on the decision: the final units of every decided CTU into one picture and a per-cell field.  DESIGN 7, row f2^8.
// k_cqt_block_cells (below) turns that field into the 4x4 cells the loop filter's boundary strengths are derived from.  DESIGN 7, row f2^9.
// k_cqt_motion_store (below) turns it into the collocated motion store the next picture's temporal candidate is derived from.  DESIGN 7, row f2^10.
#include "cabac_tables.h"
#include "common.h"
#include "launch.h"

namespace havoc_gpu {

namespace {

using CqtCtu = havoc_mi355x_cqt_ctu;
using CqtNode = havoc_mi355x_cqt_node;

constexpr int kMaxNodes = 85;
constexpr int kSpinLimit = 1 << 22;     // polls of a hand-off word before a wait gives up
constexpr unsigned long long kDone = 1ull << 63;

// the workspace: per CTU the published word, then the row ticket and the give-up word
struct CqtWork
{
    unsigned long long *pub;
    int32_t *ticket, *gaveUp;
};
__host__ __device__ inline CqtWork cqt_work_of(void *base, int n)
{
    CqtWork w;
    w.pub = static_cast<unsigned long long *>(base);
    w.ticket = reinterpret_cast<int32_t *>(w.pub + n);
    w.gaveUp = w.ticket + 1;
    return w;
}

struct CqtLds
{
    int bins[256];                          // 2 state + bin -> new state | Q16 rate << 8
    long long rate[2][kMaxNodes];           // the staged node inputs, double-buffered
    long long dist[2][kMaxNodes];
    int outcome[2][kMaxNodes];              // HAVOC_CU_OUTCOME_*; REFUSED: no candidate
    unsigned char below[2][kMaxNodes + 3];  // some node below this one has a candidate
    unsigned long long up[2];               // CtDepth above the CTU, a byte per cell (-1 outside the picture)
    unsigned int startCtx[2];               // the contexts a WPP row starts from (read at x == 0, r > 0)
    unsigned long long rows[8];             // the CTU's CtDepth cells
    unsigned long long left;                // CtDepth left of the CTU
    unsigned long long node[3 * kMaxNodes]; // the CTU's havoc_mi355x_cqt_node records
    int ticket;
    int gaveUp[2];                          // a wait of the staging of buffer b gave up (read an iteration after it is written)
};

struct Sum { long long rate, flagRate, dist; };

struct Walk
{
    CqtLds &S;
    int buf, levels, cells, cellsX, cellsY, ecu;
    unsigned int ctx;       // the three ContextModel::state of split_cu_flag, a byte each
    bool refused;
};

__device__ __forceinline__ int first_node(int d) { return d == 0 ? 0 : d == 1 ? 1 : d == 2 ? 5 : 21; }

__device__ __forceinline__ long long price(Walk &w, int inc, int bin)
{
    const int sh = 8 * inc, e = w.S.bins[2 * (int)(w.ctx >> sh & 255) + bin];
    w.ctx = (w.ctx & ~(255u << sh)) | (unsigned)(e & 255) << sh;
    return e >> 8;
}

__device__ __forceinline__ void fill(Walk &w, int x, int y, int s, int d)
{
    const unsigned long long mask = (s == 8 ? ~0ull : (1ull << 8 * s) - 1) << 8 * x, v = 0x0101010101010101ull * (unsigned)d & mask;
    for (int j = 0; j < s; ++j) w.S.rows[y + j] = (w.S.rows[y + j] & ~mask) | v;
}

__device__ __forceinline__ void put_node(Walk &w, int k, int choice, int flags, int inc, long long costFull, long long costSplit)
{
    w.S.node[3 * k] = (unsigned)(choice | flags << 8 | inc << 16);
    w.S.node[3 * k + 1] = (unsigned long long)costFull;
    w.S.node[3 * k + 2] = (unsigned long long)costSplit;
}

template <int D> __device__ Sum walk(Walk &w, int z, int x, int y);

// Syntax<coding_quadtree>::go's four children (SyntaxCtu.hpp:117-135): z-order, one after the other; a child whose origin lies outside the picture is deleted
template <int D>
__device__ __forceinline__ Sum children(Walk &w, int z, int x, int y)
{
    Sum r = {0, 0, 0};
    if constexpr (D < 3)
    {
        const int h = w.cells >> (D + 1);
#pragma unroll 1
        for (int k = 0; k < 4; ++k)
        {
            if (w.refused) break;
            const int cx = x + (k & 1) * h, cy = y + (k >> 1) * h;
            if (cx >= w.cellsX || cy >= w.cellsY)
            {
                w.S.node[3 * (first_node(D + 1) + 4 * z + k)] = HAVOC_CQT_DELETED;
                continue;
            }
            const Sum c = walk<D + 1>(w, 4 * z + k, cx, cy);
            r.rate += c.rate;
            r.flagRate += c.flagRate;
            r.dist += c.dist;
        }
    }
    return r;
}

// Search<coding_quadtree>::go (Search.hpp:808-886) of node (D, z) at cell (x, y) of the CTU -> the winner's rate, coded flags and lambdaDistortion
template <int D>
__device__ Sum walk(Walk &w, int z, int x, int y)
{
    CqtLds &S = w.S;
    const int s = w.cells >> D, k = first_node(D) + z;
    const bool mustSplit = x + s > w.cellsX || y + s > w.cellsY, minCb = D == w.levels - 1, coded = !mustSplit && !minCb;
    int flags = 0, inc = 0;
    if (coded)
    {   // Binarization.h:114-116
        const int l = x > 0 ? (int8_t)(S.rows[y] >> 8 * (x - 1)) : (int8_t)(S.left >> 8 * y);
        const int u = y > 0 ? (int8_t)(S.rows[y - 1] >> 8 * x) : (int8_t)(S.up[w.buf] >> 8 * x);
        inc = (l > D) + (u > D);
        flags = HAVOC_CQT_NODE_FLAG_CODED;
    }
    if (mustSplit)
    {   // :819-823
        const Sum r = children<D>(w, z, x, y);
        put_node(w, k, HAVOC_CQT_SPLIT, flags | HAVOC_CQT_NODE_MUST_SPLIT, inc, -1, r.rate + r.dist);
        return r;
    }
    const int outcome = S.outcome[w.buf][k];
    const bool present = outcome != HAVOC_CU_OUTCOME_REFUSED;
    const unsigned int before = w.ctx;
    Sum full = {0, 0, 0};
    long long costFull = -1;
    if (present)
    {   // :839-851: split_cu_flag(0), then the coding unit
        if (coded) full.flagRate = price(w, inc, 0);
        full.rate = full.flagRate + S.rate[w.buf][k];
        full.dist = S.dist[w.buf][k];
        fill(w, x, y, s, D);
        costFull = full.rate + full.dist;
    }
    else
        flags |= HAVOC_CQT_NODE_NO_CANDIDATE;
    const bool ecuStop = present && !minCb && w.ecu && outcome == HAVOC_CU_OUTCOME_SKIPPED;     // :854
    if (ecuStop) flags |= HAVOC_CQT_NODE_ECU_STOP;
    const bool bare = present && !minCb && !S.below[w.buf][k];         // nothing to compare the unit with: testSplit == false
    if (bare) flags |= HAVOC_CQT_NODE_NO_SPLIT_CANDIDATE;
    if (present && (minCb || ecuStop || bare))
    {
        put_node(w, k, HAVOC_CQT_CU, flags, inc, costFull, -1);
        return full;
    }
    if (minCb)
    {   // a node at MinCb without a candidate: the CTU is refused
        w.refused = true;
        return full;
    }
    // :857-871: from the state before the node, split_cu_flag(1), then the children
    const unsigned int after = w.ctx;
    w.ctx = before;
    const long long flag = coded ? price(w, inc, 1) : 0;
    Sum split = children<D>(w, z, x, y);
    if (w.refused) return split;
    split.rate += flag;
    split.flagRate += flag;
    const long long costSplit = split.rate + split.dist;
    if (!present || costSplit < costFull)
    {   // :875: strict
        put_node(w, k, HAVOC_CQT_SPLIT, flags, inc, costFull, costSplit);
        return split;
    }
    w.ctx = after;
    fill(w, x, y, s, D);
    put_node(w, k, HAVOC_CQT_CU, flags, inc, costFull, costSplit);
    return full;
}

struct CqtArgs
{
    int wc, hc;             // the picture in MinCb cells
    int cx, cy;             // ... in CTUs
    int levels, flags, nChoice;
    const int32_t *nodeCu;
    const havoc_mi355x_cu_choice *choice;
    CqtCtu *ctu;
    CqtNode *node;
    int8_t *depth;
    uint8_t *syntaxOut;
};

__global__ __launch_bounds__(256) void k_cqt_reset(CqtWork wk, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) wk.pub[i] = 0;
    if (i == 0) *wk.ticket = *wk.gaveUp = 0;
}

__global__ __launch_bounds__(256) void k_cqt_finish(CqtWork wk, int n, CqtCtu *__restrict__ ctu)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && *wk.gaveUp) ctu[i].decided = 0;        // a wait gave up: no record of the call is a decision
}

// wave 1: CTU (t, r)'s node inputs, the word of the row above it depends on, and the CtDepth above it, into buffer b
__device__ void stage(CqtLds &S, const CqtArgs &A, const CqtWork &wk, unsigned int initial, int r, int t, int b, int lane)
{
    const int nodes = first_node(A.levels - 1) + (1 << 2 * (A.levels - 1)), cells = 1 << (A.levels - 1), wpp = A.flags & HAVOC_CQT_WPP;
    const long i = (long)r * A.cx + t;
    for (int k = lane; k < nodes; k += 64)
    {
        const int idx = A.nodeCu[i * nodes + k];
        int outcome = HAVOC_CU_OUTCOME_REFUSED;
        long long rate = 0, dist = 0;
        if (idx >= 0 && idx < A.nChoice)
        {
            const havoc_mi355x_cu_choice *c = A.choice + idx;
            outcome = c->outcome;
            rate = c->rate;
            dist = c->lambda_distortion;
        }
        S.outcome[b][k] = outcome;
        S.rate[b][k] = rate;
        S.dist[b][k] = dist;
    }
    for (int d = A.levels - 1; d >= 0; --d)
    {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        for (int z = lane; z < 1 << 2 * d; z += 64)
        {
            bool any = false;
            if (d + 1 < A.levels)
                for (int k = first_node(d + 1) + 4 * z; k < first_node(d + 1) + 4 * z + 4; ++k) any = any || S.outcome[b][k] != HAVOC_CU_OUTCOME_REFUSED || S.below[b][k];
            S.below[b][first_node(d) + z] = any;
        }
    }
    unsigned long long word = kDone | initial;
    if (r > 0)
    {
        const int need = wpp ? max(t, min(1, A.cx - 1)) : t;
        const unsigned long long *p = wk.pub + (long)(r - 1) * A.cx + need;
        int spins = 0;
        for (;;)
        {
            word = __shfl(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), 0);      // one answer for the wavefront
            if (word & kDone) break;
            __builtin_amdgcn_s_sleep(8);
            if (++spins > kSpinLimit || __hip_atomic_load(wk.gaveUp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            {
                if (lane == 0) S.gaveUp[b] = 1;
                return;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");      // the CtDepth cells of the row above were written before its words
    }
    if (lane < 8)
    {
        int8_t d = -1;      // outside the picture, and the cells of `up` no node reads
        if (r > 0 && lane < cells) d = A.depth[((long)r * cells - 1) * ((long)A.cx * cells) + (long)t * cells + lane];
        reinterpret_cast<int8_t *>(&S.up[b])[lane] = d;
    }
    // with WPP a row starts from the contexts after CTU (1, r - 1) -- the word just read -- or the slice's when that CTU does not exist
    if (lane == 0 && t == 0) S.startCtx[b] = r > 0 && A.cx >= 2 ? (unsigned int)word & 0xffffffu : initial;
}

__global__ __launch_bounds__(128) void k_cqt_decide(CqtArgs A, CqtWork wk, const uint8_t *__restrict__ syntax)
{
    __shared__ CqtLds S;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int k = tid; k < 256; k += 128) S.bins[k] = bin_entry(k >> 1, k & 1);
    const unsigned long long lo0 = reinterpret_cast<const unsigned long long *>(syntax)[0], hi0 = reinterpret_cast<const unsigned long long *>(syntax)[1];
    static_assert(HAVOC_CU_SYNTAX_CTX_SPLIT_CU_FLAG == 0, "split_cu_flag's contexts are the snapshot's first three bytes");
    const unsigned int initial = (unsigned int)lo0 & 0xffffffu;
    const int levels = A.levels, cells = 1 << (levels - 1), nodes = first_node(levels - 1) + (1 << 2 * (levels - 1)), wpp = A.flags & HAVOC_CQT_WPP;
    unsigned int ctx = initial;     // lane 0 of wave 0: the contexts as the last CTU left them
    for (;;)
    {
        __syncthreads();
        if (tid == 0)
        {
            S.ticket = atomicAdd(wk.ticket, 1);
            S.gaveUp[0] = S.gaveUp[1] = 0;
        }
        __syncthreads();
        const int r = S.ticket;
        if (r >= A.cy) return;
        if (wave == 1) stage(S, A, wk, initial, r, 0, 0, lane);
        __syncthreads();
        for (int x = 0; x < A.cx; ++x)
        {
            const long i = (long)r * A.cx + x;
            if (S.gaveUp[x & 1])
            {   // the row gives up: the rows below are let through (they see the word too); k_cqt_finish clears every decision
                if (tid == 0) atomicOr(wk.gaveUp, 1);
                for (int k = x + tid; k < A.cx; k += 128) __hip_atomic_store(wk.pub + (long)r * A.cx + k, kDone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
            const int b = x & 1;
            if (wave == 1)
            {
                if (x + 1 < A.cx) stage(S, A, wk, initial, r, x + 1, b ^ 1, lane);
            }
            else
            {
                // the cells left of the CTU are the last CTU's rightmost; then a clean CTU
                int8_t l = -1;
                if (lane < 8 && x > 0) l = (int8_t)(S.rows[lane] >> 8 * (cells - 1));
                for (int k = lane; k < 3 * nodes; k += 64) S.node[k] = 0;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                if (lane < 8)
                {
                    reinterpret_cast<int8_t *>(&S.left)[lane] = l;
                    S.rows[lane] = 0;
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                Sum sum = {0, 0, 0};
                int refused = 0;
                if (lane == 0)
                {
                    if (x == 0 && r > 0 && wpp) ctx = S.startCtx[b];
                    else if (x == 0 && r == 0) ctx = initial;
                    Walk w = {S, b, levels, cells, min(cells, A.wc - x * cells), min(cells, A.hc - r * cells), (A.flags & HAVOC_CQT_ECU) != 0, ctx, false};
                    sum = walk<0>(w, 0, 0, 0);
                    refused = w.refused;
                    if (!refused) ctx = w.ctx;
                }
                refused = __shfl(refused, 0);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                int ncus = 0;
                if (refused)
                {   // no trace: node records and cells 0, the contexts as they came
                    for (int k = lane; k < 3 * nodes; k += 64) S.node[k] = 0;
                    if (lane < 8) S.rows[lane] = 0;
                }
                else
                {
                    // the decided tree: a node whose every ancestor chose the split
                    if (lane == 0) S.node[0] |= HAVOC_CQT_NODE_FINAL << 8;
                    for (int d = 1; d < levels; ++d)
                    {
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                        for (int z = lane; z < 1 << 2 * d; z += 64)
                        {
                            const unsigned int p = (unsigned int)S.node[3 * (first_node(d - 1) + (z >> 2))], n = (unsigned int)S.node[3 * (first_node(d) + z)];
                            if ((p >> 8 & HAVOC_CQT_NODE_FINAL) && (p & 255) == HAVOC_CQT_SPLIT && (n & 255) != HAVOC_CQT_NOT_VISITED)
                                S.node[3 * (first_node(d) + z)] = n | HAVOC_CQT_NODE_FINAL << 8;
                        }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    for (int k = lane; k < 128; k += 64)
                    {
                        const unsigned int n = k < nodes ? (unsigned int)S.node[3 * k] : 0;
                        ncus += __popcll(__ballot((n >> 8 & HAVOC_CQT_NODE_FINAL) && (n & 255) == HAVOC_CQT_CU));
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                unsigned long long *nodeOut = reinterpret_cast<unsigned long long *>(A.node + i * nodes);
                for (int k = lane; k < 3 * nodes; k += 64) nodeOut[k] = S.node[k];
                if (lane < cells * cells)
                {
                    const int row = lane / cells, col = lane % cells;
                    A.depth[((long)r * cells + row) * ((long)A.cx * cells) + (long)x * cells + col] = (int8_t)(S.rows[row] >> 8 * col);
                }
                if (lane == 0)
                {
                    CqtCtu c = {1, ncus, sum.rate, sum.flagRate, sum.dist, sum.rate + sum.dist};
                    if (refused) c = CqtCtu{0, 0, 0, 0, 0, 0};
                    A.ctu[i] = c;
                    unsigned long long *so = reinterpret_cast<unsigned long long *>(A.syntaxOut) + 2 * i;
                    so[0] = (lo0 & ~0xffffffull) | ctx;
                    so[1] = hi0;
                }
                // every lane's stores, then the word
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                __builtin_amdgcn_wave_barrier();
                if (lane == 0) __hip_atomic_store(wk.pub + i, kDone | ctx, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();
        }
    }
}

// k_cqt_commit: acting on the decision -- the final coding units of every decided CTU into one picture of three planes and one record per MinCb cell (DESIGN 7, row
// f2^8; the rule is restated in search/cqt_decision.hpp: commitCqt).  Nothing is computed: the samples were made by unit_pred_select and the tu_reconstruct launches of
// the unit plan, this kernel selects.  k_unit_pred_select's form: a wavefront per SEARCHED unit, four per workgroup, no LDS; every decision is wave-uniform, and the
// wavefront of a unit that is not committed -- most of them: the searched units overlap, the final ones tile the picture once -- returns after reading its unit, CTU,
// node-table and node records.  Rows go round the lanes in 8-byte pieces (4-byte pieces for an 8-bit 4x4 block), plain vector loads and stores.
// The final units of a CTU PARTITION it (test_cqt: the decided tree is a partition), and a unit is committed only as the node its own geometry names, so no two
// wavefronts write the same sample or cell: no atomics, no order between wavefronts.
using CommitArgs = havoc_mi355x_cqt_commit_args;

// a (1 << log2)^2 block of S-byte samples; strides in bytes
template <int S>
__device__ __forceinline__ void copy_block(char *d, long sd, const char *a, long sa, int log2, int lane)
{
    const int rowBytes = S << log2;
    if (rowBytes >= 8)
    {
        const int lp = __builtin_ctz(rowBytes) - 3, items = (1 << log2) << lp;     // pieces per row (a power of two), pieces of the block
        for (int t = lane; t < items; t += 64)
        {
            const int y = t >> lp, x = (t & ((1 << lp) - 1)) * 8;
            st8(d + y * sd + x, ld8(a + y * sa + x));
        }
    }
    else if (lane < 4)      // 4 rows of 4 bytes
        st4(d + lane * sd, ld4(a + lane * sa));
}

// a block of a plane from candidate pieces: one piece of size log2 (quads == false), or four of size log2 - 1 in z-order; `at` the (first) candidate's index
template <int S>
__device__ __forceinline__ void copy_pieces(char *d, long sd, const void *const *pieces, int log2, bool quads, int at, int lane)
{
    if (!quads)
    {
        copy_block<S>(d, sd, static_cast<const char *>(pieces[log2 - 2]) + ((long)at << 2 * log2) * S, S << log2, log2, lane);
        return;
    }
    const int l = log2 - 1;
    const char *a = static_cast<const char *>(pieces[l - 2]);
#pragma unroll 1
    for (int q = 0; q < 4; ++q)
        copy_block<S>(d + ((long)(q >> 1) << l) * sd + ((long)(q & 1) << l) * S, sd, a + ((long)(at + q) << 2 * l) * S, S << l, l, lane);
}

template <int S>
__global__ __launch_bounds__(256) void k_cqt_commit(CommitArgs A, int cx, int nodes)
{
    const int lane = threadIdx.x & 63, p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= A.n) return;       // wave-uniform, as every branch below
    const havoc_mi355x_rqt_unit u = A.d_units[p];
    const int L = u.log2_size, size = 1 << L, d = A.ctb_log2 - L;
    if (L < A.min_cb_log2 || d < 0) return;
    if (u.x0 < 0 || u.y0 < 0 || ((u.x0 | u.y0) & (size - 1)) || u.x0 + size > A.width || u.y0 + size > A.height) return;     // no such node: skipped, not followed
    const int c = (u.y0 >> A.ctb_log2) * cx + (u.x0 >> A.ctb_log2);
    if (A.d_ctu[c].decided != 1) return;
    const int px = (u.x0 & ((1 << A.ctb_log2) - 1)) >> L, py = (u.y0 & ((1 << A.ctb_log2) - 1)) >> L;
    int z = 0;
#pragma unroll
    for (int b = 0; b < 3; ++b) z |= (px >> b & 1) << 2 * b | (py >> b & 1) << (2 * b + 1);
    const long at = (long)c * nodes + first_node(d) + z;
    if (A.d_node_cu[at] != p) return;
    const unsigned int node = (unsigned int)*reinterpret_cast<const unsigned long long *>(A.d_node + at);        // choice, flags, ctx_inc
    if ((node & 255) != HAVOC_CQT_CU || !(node >> 8 & HAVOC_CQT_NODE_FINAL)) return;
    const int outcome = A.d_cu[p].outcome;
    if (outcome != HAVOC_CU_OUTCOME_CODED && outcome != HAVOC_CU_OUTCOME_NO_RESIDUAL && outcome != HAVOC_CU_OUTCOME_SKIPPED) return;

    char *recY = static_cast<char *>(A.d_rec_y) + (A.rec_origin + (long)u.y0 * A.rec_stride + u.x0) * S;
    const long cAt = (long)(u.y0 >> 1) * A.c_stride + (u.x0 >> 1), sdY = A.rec_stride * S, sdC = A.c_stride * S;
    char *recCb = static_cast<char *>(A.d_rec_c) + (A.cb_origin + cAt) * S, *recCr = static_cast<char *>(A.d_rec_c) + (A.cr_origin + cAt) * S;
    int trDepth = 0;
    unsigned int cbf = 0;
    if (outcome == HAVOC_CU_OUTCOME_CODED)
    {   // the pieces of the depth that stands: cu_close's own rule; a 64x64 unit has its depth-1 pieces only
        const havoc_mi355x_rqt_choice *ch = A.d_choice + p;
        trDepth = (L < 6 && ch->depth == 0 && ch->tried_zero) ? 0 : 1;
        const havoc_mi355x_rqt_tree_choice tc = A.d_tree_choice[p];
        const havoc_mi355x_rqt_chroma_at ca = A.d_chroma_at[p];
        cbf = trDepth ? tc.mask_one : tc.mask_zero;
        copy_pieces<S>(recY, sdY, A.luma_pieces, L, trDepth != 0, trDepth ? A.d_one_at[p] : A.d_zero_at[p], lane);
        const bool quads = trDepth != 0 && L > 3;       // an 8x8 unit's one 4x4 block per component serves both depths
        copy_pieces<S>(recCb, sdC, A.chroma_pieces, L - 1, quads, quads ? ca.cb_one : ca.cb_zero, lane);
        copy_pieces<S>(recCr, sdC, A.chroma_pieces, L - 1, quads, quads ? ca.cr_one : ca.cr_zero, lane);
    }
    else
    {   // left at its prediction
        const int32_t *off = A.d_pred_off + 3 * (long)p;
        const char *predY = static_cast<const char *>(A.d_pred_y), *predC = static_cast<const char *>(A.d_pred_c);
        copy_block<S>(recY, sdY, predY + (long)off[0] * S, A.pred_stride * S, L, lane);
        copy_block<S>(recCb, sdC, predC + (long)off[1] * S, A.pred_stride_c * S, L - 1, lane);
        copy_block<S>(recCr, sdC, predC + (long)off[2] * S, A.pred_stride_c * S, L - 1, lane);
    }
    // the unit's cells: at most 8 x 8, a lane each, three 8-byte stores
    const int cl = L - A.min_cb_log2;
    if (lane < 1 << 2 * cl)
    {
        const int pred = A.d_best[p] & 255, cand = A.d_unit_cand[p];
        unsigned long long mv = 0;
        if (A.d_cand_mv != nullptr && cand >= 0) mv = *reinterpret_cast<const unsigned long long *>(A.d_cand_mv + 4 * (long)cand);
        if (pred != 0 && pred != 2) mv &= ~0xffffffffull;       // a list the mode does not use: 0, 0
        if (pred != 1 && pred != 2) mv &= 0xffffffffull;
        const long cell = (long)((u.y0 >> A.min_cb_log2) + (lane >> cl)) * (A.width >> A.min_cb_log2) + (u.x0 >> A.min_cb_log2) + (lane & ((1 << cl) - 1));
        unsigned long long *o = reinterpret_cast<unsigned long long *>(A.d_cells + cell);
        o[0] = (unsigned int)p | (unsigned long long)(unsigned int)cand << 32;
        o[1] = mv;
        o[2] = (unsigned long long)(L | outcome << 8 | pred << 16 | trDepth << 24) | (unsigned long long)cbf << 32;
    }
}

// k_cqt_block_cells: the 4x4 cells havoc_mi355x_derive_bs reads, made from the committed 8x8 (MinCb) cells (DESIGN 7, row f2^9; the rule is stated in
// include/havoc_mi355x.h and restated in search/cqt_decision.hpp: cqtBlockCells).  A lane per OUTPUT cell in raster order: three aligned 8-byte loads of the record
// that covers it (the lanes of one MinCb cell read the same lines), every branch a select, one aligned 16-byte store -- a wavefront writes 1 KB contiguous when the
// rows are dense.  A coding unit is aligned to its size, so the cell's own position names the unit's origin: no unit table, no second pass, every cell written once.
__global__ __launch_bounds__(256) void k_cqt_block_cells(const havoc_mi355x_cqt_cell *__restrict__ q, int cw, int count, int minCbLog2, int qcw, int qp, int dpb0, int dpb1,
                                                         havoc_mi355x_cell *__restrict__ cells, long stride)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int cy = i / cw, cx = i - cy * cw, x = cx << 2, y = cy << 2;
    const unsigned long long *r = reinterpret_cast<const unsigned long long *>(q + (long)(y >> minCbLog2) * qcw + (x >> minCbLog2));
    const unsigned long long head = r[0], mv = r[1], tail = r[2];
    const bool decided = (int)(unsigned int)head >= 0;          // unit -1: the commit left all-ones bytes, nothing else of the record means anything
    const unsigned int info = (unsigned int)tail, cbf = (unsigned int)(tail >> 32);
    const int L = decided ? (int)(info & 255) : 3, outcome = info >> 8 & 255, pred = info >> 16 & 255, depth = info >> 24 & 255;
    const int size = 1 << L, ox = x & (size - 1), oy = y & (size - 1), half = size >> 1;
    const int k = depth ? (oy >= half) * 2 + (ox >= half) : 0;
    const bool coded = outcome == HAVOC_CU_OUTCOME_CODED && (cbf >> k & 1);
    const unsigned int flags = decided ? (coded ? HAVOC_CELL_CODED : 0) | (ox == 0 ? HAVOC_CELL_PU_LEFT : 0) | (oy == 0 ? HAVOC_CELL_PU_TOP : 0) : HAVOC_CELL_NO_FILTER;
    const unsigned int d0 = decided && pred != 1 ? (unsigned int)dpb0 : 255u, d1 = decided && pred != 0 ? (unsigned int)dpb1 : 255u;
    const unsigned int tu = decided ? (unsigned int)min(L - depth, 5) : 2u;
    const unsigned long long v = decided ? mv : 0ull;
    *reinterpret_cast<u32x4 *>(cells + (long)cy * stride + cx) = u32x4{(unsigned int)v, (unsigned int)(v >> 32), d0 | d1 << 8 | flags << 16 | (unsigned int)qp << 24, tu};
}

// k_cqt_motion_store: the collocated motion store of the committed picture, one 24-byte record per 16x16 luma samples (DESIGN 7, row f2^10; the rule is stated in
// include/havoc_mi355x.h and restated in search/cqt_decision.hpp: cqtMotionStore).  A lane per ENTRY in raster order: three aligned 8-byte loads of the committed cell
// that covers luma sample (16 X, 16 Y) -- the one unit whose fillRectangle writes the entry --, every branch a select, three aligned 8-byte stores.  8 160 entries at
// 1080p: the launch is bound by its latency, nothing cleverer is wanted.
__global__ __launch_bounds__(256) void k_cqt_motion_store(const havoc_mi355x_cqt_cell *__restrict__ q, int sw, int count, int minCbLog2, int qcw, int refPoc0, int refPoc1,
                                                          havoc_mi355x_col_cell *__restrict__ store)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int Y = i / sw, X = i - Y * sw;
    const unsigned long long *r = reinterpret_cast<const unsigned long long *>(q + (long)((Y << 4) >> minCbLog2) * qcw + ((X << 4) >> minCbLog2));
    const unsigned long long head = r[0], mv = r[1], tail = r[2];
    const bool decided = (int)(unsigned int)head >= 0;          // unit -1: the commit left all-ones bytes, nothing else of the record means anything
    const int pred = (unsigned int)tail >> 16 & 255;
    const bool p0 = decided && pred != 1, p1 = decided && pred != 0;
    const unsigned long long use = (p0 ? 0xffffffffull : 0ull) | (p1 ? 0xffffffff00000000ull : 0ull);
    unsigned long long *o = reinterpret_cast<unsigned long long *>(store + i);
    o[0] = mv & use;
    o[1] = ((unsigned long long)(unsigned int)refPoc0 | (unsigned long long)(unsigned int)refPoc1 << 32) & use;
    o[2] = (p0 ? 1ull : 0ull) | (p1 ? 256ull : 0ull);          // pred_flag[0], pred_flag[1]; long_term 0, 0; reserved 0
}

} // namespace

hipError_t launch_cqt_commit(hipStream_t st, const havoc_mi355x_cqt_commit_args &A)
{
    const int wc = A.width >> A.min_cb_log2, hc = A.height >> A.min_cb_log2;
    const int cx = (A.width + (1 << A.ctb_log2) - 1) >> A.ctb_log2, levels = A.ctb_log2 - A.min_cb_log2 + 1;
    // every cell "no unit" first: the cells of an undecided CTU stay so
    hipError_t e = hipMemsetAsync(A.d_cells, 0xff, (size_t)wc * hc * sizeof(havoc_mi355x_cqt_cell), st);
    if (e != hipSuccess || A.n <= 0) return e;
    const dim3 grid((unsigned)((A.n + 3) / 4)), block(256);
    if (A.bit_depth == 8)
        hipLaunchKernelGGL(k_cqt_commit<1>, grid, block, 0, st, A, cx, ((1 << 2 * levels) - 1) / 3);
    else
        hipLaunchKernelGGL(k_cqt_commit<2>, grid, block, 0, st, A, cx, ((1 << 2 * levels) - 1) / 3);
    return hipGetLastError();
}

hipError_t launch_cqt_block_cells(hipStream_t st, int width, int height, int minCbLog2, int qp, int dpb0, int dpb1, const havoc_mi355x_cqt_cell *cqtCells,
                                  havoc_mi355x_cell *cells, long stride)
{
    const int cw = width >> 2, count = cw * (height >> 2);
    hipLaunchKernelGGL(k_cqt_block_cells, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, cqtCells, cw, count, minCbLog2, width >> minCbLog2, qp, dpb0, dpb1, cells,
                       stride);
    return hipGetLastError();
}

hipError_t launch_cqt_motion_store(hipStream_t st, int width, int height, int minCbLog2, int refPoc0, int refPoc1, const havoc_mi355x_cqt_cell *cqtCells,
                                   havoc_mi355x_col_cell *store)
{
    const int sw = (width + 15) >> 4, count = sw * ((height + 15) >> 4);
    hipLaunchKernelGGL(k_cqt_motion_store, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, cqtCells, sw, count, minCbLog2, width >> minCbLog2, refPoc0, refPoc1, store);
    return hipGetLastError();
}

size_t cqt_decide_workspace_bytes(int nctus) { return nctus <= 0 ? 0 : (size_t)nctus * 8 + 16; }

hipError_t launch_cqt_decide(hipStream_t st, int width, int height, int ctbLog2, int minCbLog2, int flags, const uint8_t *syntax, const int32_t *nodeCu,
                             const havoc_mi355x_cu_choice *choice, int nChoice, void *work, havoc_mi355x_cqt_ctu *ctu, havoc_mi355x_cqt_node *node, int8_t *depth,
                             uint8_t *syntaxOut)
{
    const int cx = (width + (1 << ctbLog2) - 1) >> ctbLog2, cy = (height + (1 << ctbLog2) - 1) >> ctbLog2, n = cx * cy;
    const CqtWork wk = cqt_work_of(work, n);
    const CqtArgs A = {width >> minCbLog2, height >> minCbLog2, cx, cy, ctbLog2 - minCbLog2 + 1, flags, nChoice, nodeCu, choice, ctu, node, depth, syntaxOut};
    // rows by ticket: at most one workgroup per CU (cdna_hip_programming 1: the grid stays resident); without WPP the rows are a chain
    const int grid = (flags & HAVOC_CQT_WPP) ? (cy < 256 ? cy : 256) : 1;
    hipLaunchKernelGGL(k_cqt_reset, dim3((n + 255) / 256), dim3(256), 0, st, wk, n);
    hipLaunchKernelGGL(k_cqt_decide, dim3(grid), dim3(128), 0, st, A, wk, syntax);
    hipLaunchKernelGGL(k_cqt_finish, dim3((n + 255) / 256), dim3(256), 0, st, wk, n, ctu);
    return hipGetLastError();
}

} // namespace havoc_gpu
