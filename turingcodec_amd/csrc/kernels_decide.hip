// Decisions that are data-parallel -- one lane per partition, no chain between partitions -- taken ON THE DEVICE between the launches they
// separate, so that neither the costs they read nor the job tables they produce cross the link (round 3):
//
//   k_intra_order   the 35 costs of a partition -> the order its modes are RD-refined in.  Restates intraModeOrder of
//                   turingcodec_amd/search/decision.hpp, i.e. turing/Search.hpp:55-98 (rate offsets of the most probable modes + lambda * SATD)
//                   and :143-190 (repeated selection of the cheapest mode, first index on ties; after `maxRefine` selections the most probable
//                   modes not yet taken are forced in).  Q16 costs in 64-bit integers, the host's arithmetic bit for bit.
//   k_intra_expand  every candidate (partition, mode of its order) -> the four job records of the chain that reconstructs it: intra prediction
//                   into a piece, residual + forward transform, Rdoq::runQuantisation (intra, scan by mode: turing/Global.h:1212-1227),
//                   reconstruction + SSD, level statistics.  Slots are handed out with an atomic counter (which slot a candidate gets does not
//                   matter to anything but addresses).
//   k_intra_decide  a partition's candidates' outcomes -> the champion (decideIntraRd of search/tu_decision.hpp; Search.hpp:143-255: the first
//                   candidate with the smallest mode rate + residual rate + ssd * reciprocal lambda) and the job that reconstructs it into the
//                   caller's buffer.  RATED: the rate is the caller's per candidate (havoc_mi355x_intra_rate: the reference's CABAC bits; k_intra_rate_jobs
//                   makes that kernel's records from the tables here).
// The host forms of the same rules stay: they are what the per-call arms of the tests run over the reference's tables.
#include "common.h"
#include "launch.h"
#include "../search/cand_mode_list.hpp"

namespace havoc_gpu {

namespace {

using IntraCtx = havoc_mi355x_intra_mpm;
using SearchJob = havoc_mi355x_intra_search_job;
using IntraJob = havoc_mi355x_intra_job;
using TuJob = havoc_mi355x_tu_fused_job;
using RdoqJob = havoc_mi355x_rdoq_job;

constexpr int kMaxOrder = HAVOC_MI355X_INTRA_MAX_ORDER;      // maxRefine (<= 8) + 3 most probable modes, + 1 spare
constexpr int64_t kCostMax = 0x7fffffffffffffffll;

} // namespace (the aliases name public types, so the kernels taking them have external linkage like the library's others; the mirrors made them internal)

// order[i][0 .. count[i]) ; slot[i] = first candidate slot of partition i; total[0] = slots handed out, total[1] != 0: a partition wanted more
// than kMaxOrder candidates
__global__ __launch_bounds__(64) void k_intra_order(const int32_t *__restrict__ satd35, const IntraCtx *__restrict__ ictx, int n, int32_t lambdaQ16,
                                                    int32_t *__restrict__ order, int32_t *__restrict__ count, int32_t *__restrict__ slot, int32_t *__restrict__ total)
{
    __shared__ int64_t costs[35][64];      // [mode][lane]
    const int lane = threadIdx.x, i = blockIdx.x * 64 + lane;
    if (i >= n) return;
    IntraCtx c = ictx[i];
    // the records come from device memory: a mode outside 0..34 or more than three neighbour modes would index past costs[] / cand[] -- flagged
    // (total[1] bit 1) and brought into range, so nothing is written outside the partition's own slots
    const bool bad = (unsigned)c.cand_mode_list[0] > 34u || (unsigned)c.cand_mode_list[1] > 34u || (unsigned)c.cand_mode_list[2] > 34u || (unsigned)c.neighbour_modes > 3u || c.max_refine < 1;
    if (bad)
    {
        atomicOr(total + 1, 2);
        for (int k = 0; k < 3; ++k) c.cand_mode_list[k] = min(max(c.cand_mode_list[k], 0), 34);
        c.neighbour_modes = min(max(c.neighbour_modes, 0), 3);
        c.max_refine = max(c.max_refine, 1);
    }
    for (int m = 0; m < 35; ++m) costs[m][lane] = 0;
    costs[c.cand_mode_list[0]][lane] = c.rate_a_minus_c;
    costs[c.cand_mode_list[1]][lane] = c.rate_b_minus_c;
    costs[c.cand_mode_list[2]][lane] = c.rate_b_minus_c;
    for (int m = 0; m < 35; ++m) costs[m][lane] += (int64_t)lambdaQ16 * (int64_t)satd35[35 * (long)i + m];
    int cnt = 0, nMpm = 0;
    for (int j = 0; j < c.max_refine + nMpm; ++j)
    {
        if (cnt == kMaxOrder)      // more candidates than a partition has slots: reported, nothing written past them
        {
            atomicOr(total + 1, 1);
            break;
        }
        int mode = 0;
        int64_t best = costs[0][lane];
        for (int m = 1; m < 35; ++m)
        {
            const int64_t v = costs[m][lane];
            if (v < best)
            {
                best = v;
                mode = m;
            }
        }
        costs[mode][lane] = kCostMax;
        if (j == c.max_refine - 1)
            for (int k = 0; k < c.neighbour_modes; ++k)
                if (costs[c.cand_mode_list[k]][lane] != kCostMax)
                {
                    costs[c.cand_mode_list[k]][lane] = 0;
                    ++nMpm;
                }
        order[kMaxOrder * (long)i + cnt++] = mode;
    }
    count[i] = cnt;
    slot[i] = atomicAdd(total, cnt);
}

__global__ __launch_bounds__(256) void k_intra_expand(const SearchJob *__restrict__ parts, const int32_t *__restrict__ order, const int32_t *__restrict__ count,
                                                      const int32_t *__restrict__ slot, const int32_t *__restrict__ ctxIndex, int n, int log2, int quantScale,
                                                      int quantShift, int invScale, int lambdaQ16, int sdhFactor, int sdh, IntraJob *__restrict__ ij,
                                                      TuJob *__restrict__ tj, RdoqJob *__restrict__ rj, int32_t *__restrict__ sj, int32_t *__restrict__ owner)
{
    const long t = blockIdx.x * 256L + threadIdx.x;
    const int i = (int)(t / kMaxOrder), k = (int)(t - (long)i * kMaxOrder);
    if (i >= n || k >= count[i]) return;
    const SearchJob p = parts[i];
    const int mode = order[kMaxOrder * (long)i + k], c = slot[i] + k, area = 1 << (2 * log2);
    const uint64_t mask = (uint64_t)p.filt_lo | ((uint64_t)p.filt_hi << 32);
    IntraJob a = {c * area, ((mask >> mode) & 1) ? p.nbf_off : p.nb_off, log2, mode, p.edge, {0, 0, 0}};
    ij[c] = a;
    TuJob b = {c * area, p.src_off, c * area, c * area};
    tj[c] = b;
    RdoqJob r = {c * area, c * area, quantScale, quantShift, invScale, lambdaQ16, sdhFactor, ctxIndex[i], 0,
                    (uint8_t)((log2 == 2 || log2 == 3) ? ((mode >= 6 && mode <= 14) ? 2 : ((mode >= 22 && mode <= 30) ? 1 : 0)) : 0), 1, (uint8_t)(sdh != 0), {0, 0, 0}};
    rj[c] = r;
    sj[2 * c] = c * area;
    sj[2 * c + 1] = area;
    owner[c] = i;
}

// every candidate slot -> its havoc_mi355x_intra_rate record: where k_intra_expand put its levels, which snapshot and scan its Rdoq job names, and where its mode
// stands in candModeList (Binarization.h:432-447: the FIRST x with mode == candModeList[x]; none: rem_intra_luma_pred_mode)
__global__ __launch_bounds__(256) void k_intra_rate_jobs(const IntraCtx *__restrict__ ictx, const int32_t *__restrict__ order, const int32_t *__restrict__ count,
                                                         const int32_t *__restrict__ slot, const RdoqJob *__restrict__ rj, int n, int flags,
                                                         havoc_mi355x_intra_rate_job *__restrict__ out)
{
    const long t = blockIdx.x * 256L + threadIdx.x;
    const int i = (int)(t / kMaxOrder), k = (int)(t - (long)i * kMaxOrder);
    if (i >= n || k >= count[i]) return;
    const int mode = order[kMaxOrder * (long)i + k], c = slot[i] + k;
    const IntraCtx m = ictx[i];
    const RdoqJob r = rj[c];
    const int mpm = mode == m.cand_mode_list[0] ? 0 : (mode == m.cand_mode_list[1] ? 1 : (mode == m.cand_mode_list[2] ? 2 : 3));
    havoc_mi355x_intra_rate_job j = {r.dst_off, r.ctx_index, c, r.scan_idx, r.sdh, (uint8_t)mpm, (uint8_t)flags, {0, 0, 0, 0}};
    out[c] = j;
}

// RATED: the whole rate of a candidate is the caller's (havoc_mi355x_intra_rate: the reference's bits) in place of the first stage's mode offsets and the stand-in;
// nothing else differs.  The reference measures a challenger's rate only when its distortion alone is below the champion's cost (Search.hpp:242-246); rates are
// never negative, so pricing every candidate and comparing whole costs with the strict `<` in refinement order picks the same champion at the same cost.
template <bool RATED>
__global__ __launch_bounds__(256) void k_intra_decide(const IntraCtx *__restrict__ ictx, const int32_t *__restrict__ order, const int32_t *__restrict__ count,
                                                      const int32_t *__restrict__ slot, const int32_t *__restrict__ cbf, const uint32_t *__restrict__ ssd,
                                                      const int32_t *__restrict__ stats, const int64_t *__restrict__ rates, const TuJob *__restrict__ tj, int n, int log2,
                                                      int32_t reciprocalLambdaQ16, havoc_mi355x_intra_choice *__restrict__ out, TuJob *__restrict__ fin)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const IntraCtx c = ictx[i];
    havoc_mi355x_intra_choice r = {-1, 0, 0, 0, kCostMax, 0, 0, 0, 0};
    const int base = slot[i];
    for (int j = 0; j < count[i]; ++j)
    {
        const int mode = order[kMaxOrder * (long)i + j], s = base + j;
        const bool haveStats = !RATED || stats != nullptr;      // (no level statistics: the rated form)
        const int nonzero = haveStats ? stats[2 * s] : 0, sumAbs = haveStats ? stats[2 * s + 1] : 0;
        int64_t rate;
        if (RATED)
            rate = rates[s];
        else
        {
            const int64_t modeRate = mode == c.cand_mode_list[0] ? c.rate_a_minus_c : ((mode == c.cand_mode_list[1] || mode == c.cand_mode_list[2]) ? c.rate_b_minus_c : 0);
            rate = modeRate + ((int64_t)(1 + (cbf[s] ? 2 * nonzero + sumAbs : 0)) << 16);      // search/tu_decision.hpp: tuRate (stand-in; the RATED form has the reference's bits)
        }
        const int64_t cost = rate + (int64_t)reciprocalLambdaQ16 * (int64_t)(int32_t)ssd[s];
        ++r.evaluated;
        if (cost < r.cost)
        {
            r.mode = mode;
            r.index = j;
            r.cost = cost;
            r.cbf = cbf[s];
            r.ssd = ssd[s];
            r.nonzero = nonzero;
            r.sum_abs = sumAbs;
        }
    }
    out[i] = r;
    // a partition without candidates (count 0: max_refine < 1, which the host wrapper refuses) has no champion: out[i].mode stays -1 and its final job reads the
    // first slots of the buffers instead of a slot that belongs to another partition or lies past the allocation
    TuJob f = count[i] > 0 ? tj[base + max(0, r.index)] : TuJob{0, 0, 0, 0};
    f.rec_off = i << (2 * log2);
    fin[i] = f;
}

// ---- the transform-tree decision of inter units and the picture's block structure, ON THE DEVICE (round 4) -----------------------------------------------
// search/tu_decision.hpp's decideRqt (turing/Reconstruct.cpp:1296-1428) restated lane per unit over the outcomes of its five candidate blocks (depth 0: one block,
// depth 1: four, evaluated by the chain tu_forward -> rdoq -> tu_reconstruct -> level_stats), so that a picture's launches after its searches need no host in
// between (the residual term is the stand-in of tu_decision.hpp, or -- RATED -- the reference's bits of each candidate's residual_coding from
// kernels_residual_rate.hip; cbf_luma, split_transform_flag and the chroma residuals are priced by neither -- or, kRqtTree, the reference's whole comparison over three
// planes from havoc_mi355x_tree_rate): the decision, the job records that reconstruct EVERY candidate -- the chosen ones into the picture, the others into a dump area (a fixed number of jobs per
// size: the sequence can be recorded into a HIP graph) -- and the 4x4 cells havoc_mi355x_derive_bs reads.  The host forms stay: tests hold these against them.
using RqtUnit = havoc_mi355x_rqt_unit;
using TuOutcome = havoc_mi355x_tu_outcome;
using RqtResult = havoc_mi355x_rqt_choice;
using RqtSize = havoc_mi355x_rqt_size;      // one transform size
using Cell = havoc_mi355x_cell;
struct RqtSizes { RqtSize s[4]; };

struct RqtRates { const int64_t *r[4]; };      // havoc_mi355x_rqt_decide_rated: the Q16 rate of candidate j of each transform size

// havoc_mi355x_rqt_decide_tree: the chroma candidates per chroma transform size, where each unit finds its own, the whole-tree rate and cbf mask per unit and depth
// (havoc_mi355x_tree_rate), the chroma reconstruction planes and the 16-byte records
struct RqtTree
{
    RqtSizes c;
    const havoc_mi355x_rqt_chroma_at *at;
    const int64_t *rate;
    const uint32_t *cbf;
    long cbOrigin, crOrigin;
    int cStride, cDump;
    havoc_mi355x_rqt_tree_choice *out;
};

enum RqtMode { kRqtStandIn, kRqtRated, kRqtTree, kRqtUnits };

__device__ __forceinline__ TuOutcome outcomeOf(const RqtSize &z, int j)
{
    return z.d_stats ? TuOutcome{z.d_cbf[j], z.d_ssd[j], z.d_stats[2 * j], z.d_stats[2 * j + 1]} : TuOutcome{z.d_cbf[j], z.d_ssd[j], 0, 0};      // (no level statistics: the rated form)
}
__device__ __forceinline__ int64_t tuRateOf(const TuOutcome &t) { return (int64_t)(1 + (t.cbf ? 2 * t.nonzero + t.sum_abs : 0)) << 16; }      // tu_decision.hpp: tuRate (stand-in)

// kRqtRated: the residual term is the caller's rate of each candidate (havoc_mi355x_residual_rate: the reference's bits) in place of the stand-in; nothing else differs.
// kRqtTree: the reference's own comparison -- the rate is the whole transform_tree's of the depth (havoc_mi355x_tree_rate), the distortion ssdY + 4 ssdCb + 4 ssdCr in
// int32, "coded" means a level in any of the three planes -- and the chroma candidates get their final job records beside the luma ones.
// kRqtUnits (havoc_mi355x_rqt_decide_units): kRqtTree's decision for units that overlap one another -- the searched units of every size, 64x64 included -- which cannot
// all be reconstructed into one picture: NO final job record is written (d_final is never touched; recOrigin, recStride, dumpOff and the tree's chroma planes are not
// read).  A 64x64 unit has depth 1 only (its split is inferred above MaxTbLog2SizeY, Reconstruct.cpp:1300-1310): four 32x32 luma candidates in z.s[3], four Cb and Cr
// 16x16 candidates in tree.c.s[2]; zeroAt, cb_zero and cr_zero are not read, depth 0 stays untried and depth = 1 exactly when the tree has a level.
template <int MODE>
__global__ __launch_bounds__(256) void k_rqt_decide(const RqtUnit *__restrict__ units, int n, const int32_t *__restrict__ zeroAt, const int32_t *__restrict__ oneAt,
                                                    const RqtSizes z, const RqtRates rates, const RqtTree tree, long recOrigin, int recStride, int dumpOff,
                                                    int32_t reciprocalLambdaQ16, RqtResult *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const RqtUnit u = units[i];
    constexpr bool TREE = MODE == kRqtTree || MODE == kRqtUnits;
    if (u.log2_size < 3 || u.log2_size > (MODE == kRqtUnits ? 6 : 5))      // a unit has a depth-0 block of 8 .. 32 and four depth-1 blocks of half that: anything else has no size table
    {
        RqtResult bad = RqtResult();
        bad.depth = -1;
        out[i] = bad;
        if (TREE) tree.out[i] = havoc_mi355x_rqt_tree_choice();
        return;
    }
    const bool inferred = MODE == kRqtUnits && u.log2_size == 6;      // the split is inferred: the unit has no depth-0 candidate in any plane
    const RqtSize &s0 = z.s[inferred ? 3 : u.log2_size - 2], &s1 = z.s[u.log2_size - 3];
    const int j0 = inferred ? 0 : zeroAt[i], j1 = oneAt[i], half = 1 << (u.log2_size - 1);
    // the unit's chroma candidates (kRqtTree): depth 0 one Cb and one Cr block of log2 max(L - 1, 2); depth 1 four of each of log2 L - 2 -- an 8x8 unit's one 4x4
    // block per component is the same candidate at both depths
    const int chromaOne = u.log2_size > 3 ? 4 : 0;
    const RqtSize &c0 = tree.c.s[u.log2_size > 3 ? u.log2_size - 3 : 0], &c1 = tree.c.s[u.log2_size > 3 ? u.log2_size - 4 : 0];
    havoc_mi355x_rqt_chroma_at ca = havoc_mi355x_rqt_chroma_at();
    havoc_mi355x_rqt_tree_choice tc = havoc_mi355x_rqt_tree_choice();
    RqtResult r = RqtResult();
    int32_t ssdOne = 0;      // (int32 as the reference's StateEncodeSubstream::ssd: four 16x16 blocks of <= 255^2 * 256 each, or 10-bit SSDs >> 4, stay far below 2^31)
    bool coded = false;
    int64_t rateOne = 0;
    for (int k = 0; k < 4; ++k)      // rqtdepth = 1 first (Reconstruct.cpp:1325-1326), blocks in z-order
    {
        r.one[k] = outcomeOf(s1, j1 + k);
        ssdOne += (int32_t)r.one[k].ssd;
        coded |= r.one[k].cbf != 0;
        if (!TREE) rateOne += MODE == kRqtRated ? rates.r[u.log2_size - 3][j1 + k] : tuRateOf(r.one[k]);
    }
    if (TREE)
    {
        ca = tree.at[i];
        uint32_t chroma = 0;
        if (chromaOne)
            for (int k = 0; k < 4; ++k) chroma += c1.d_ssd[ca.cb_one + k] + c1.d_ssd[ca.cr_one + k];
        else
            chroma = c0.d_ssd[ca.cb_zero] + c0.d_ssd[ca.cr_zero];
        tc.chroma_ssd_one = (int32_t)chroma;
        tc.mask_one = tree.cbf[2 * i + 1];
        ssdOne = (int32_t)((uint32_t)ssdOne + 4u * chroma);      // ssd[0] + 4 ssd[1] + 4 ssd[2], int32
        coded = tc.mask_one != 0;                                 // rqt_root_cbf of the split tree: a level in ANY plane
        rateOne = tree.rate[2 * i + 1];
    }
    r.cost_one = rateOne + (int64_t)reciprocalLambdaQ16 * (int64_t)ssdOne;
    if (coded && inferred)
        r.depth = 1;      // the one tree there is (the reference's rqtdepth 0 of a 64x64 unit IS this tree: recorded as what is coded, which is what cu_close reads)
    else if (coded)
    {
        r.tried_zero = 1;
        r.zero = outcomeOf(s0, j0);
        int32_t ssdZero = (int32_t)r.zero.ssd;
        int64_t rateZero = 0;
        if (TREE)
        {
            const uint32_t chroma = c0.d_ssd[ca.cb_zero] + c0.d_ssd[ca.cr_zero];
            tc.chroma_ssd_zero = (int32_t)chroma;
            tc.mask_zero = tree.cbf[2 * i];
            ssdZero = (int32_t)((uint32_t)ssdZero + 4u * chroma);
            rateZero = tree.rate[2 * i];
        }
        else
            rateZero = MODE == kRqtRated ? rates.r[u.log2_size - 2][j0] : tuRateOf(r.zero);
        r.cost_zero = rateZero + (int64_t)reciprocalLambdaQ16 * (int64_t)ssdZero;
        r.depth = r.cost_zero < r.cost_one ? 0 : 1;      // Reconstruct.cpp:1389
    }
    out[i] = r;
    if (TREE) tree.out[i] = tc;
    if (MODE == kRqtUnits) return;
    // every candidate is reconstructed once more: the chosen tree into the picture -- a unit left without residual through its four depth-1 blocks, whose levels are
    // all zero (= the prediction) -- the rest into the dump area
    const bool zeroWins = r.depth == 0 && r.tried_zero;
    TuJob f = s0.d_jobs[j0];
    f.rec_off = zeroWins ? (int32_t)(recOrigin + (long)u.y0 * recStride + u.x0) : dumpOff;
    s0.d_final[j0] = f;
    for (int k = 0; k < 4; ++k)
    {
        TuJob g = s1.d_jobs[j1 + k];
        g.rec_off = zeroWins ? dumpOff : (int32_t)(recOrigin + (long)(u.y0 + (k >> 1) * half) * recStride + u.x0 + (k & 1) * half);
        s1.d_final[j1 + k] = g;
    }
    if (MODE == kRqtTree)
    {   // ... and the chroma candidates into the chroma reconstruction planes the same way (an 8x8 unit's only chroma candidate belongs to both trees)
        const long at = (long)(u.y0 >> 1) * tree.cStride + (u.x0 >> 1);
        const bool zeroChroma = zeroWins || !chromaOne;
        TuJob cb = c0.d_jobs[ca.cb_zero], cr = c0.d_jobs[ca.cr_zero];
        cb.rec_off = zeroChroma ? (int32_t)(tree.cbOrigin + at) : tree.cDump;
        cr.rec_off = zeroChroma ? (int32_t)(tree.crOrigin + at) : tree.cDump;
        c0.d_final[ca.cb_zero] = cb;
        c0.d_final[ca.cr_zero] = cr;
        const int quarter = half >> 1;
        for (int k = 0; k < chromaOne; ++k)
        {
            const long sub = at + (long)((k >> 1) * quarter) * tree.cStride + (k & 1) * quarter;
            cb = c1.d_jobs[ca.cb_one + k];
            cr = c1.d_jobs[ca.cr_one + k];
            cb.rec_off = zeroWins ? tree.cDump : (int32_t)(tree.cbOrigin + sub);
            cr.rec_off = zeroWins ? tree.cDump : (int32_t)(tree.crOrigin + sub);
            c1.d_final[ca.cb_one + k] = cb;
            c1.d_final[ca.cr_one + k] = cr;
        }
    }
}

// havoc_search_block_cells on the device: every unit one inter 2Nx2N prediction unit from list 0 at the vector the field holds at its origin, its transform tree as decided
__global__ __launch_bounds__(256) void k_block_cells_blank(Cell *__restrict__ cells, int count, int qp, int dpb0)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    Cell c = Cell();
    c.dpb_index[0] = (int8_t)dpb0;
    c.dpb_index[1] = -1;
    c.qp_y = (int8_t)qp;
    c.tu_log2 = 2;
    cells[i] = c;
}

__global__ __launch_bounds__(64) void k_block_cells(const RqtUnit *__restrict__ units, const RqtResult *__restrict__ dec, int n, const int32_t *__restrict__ field, int cw,
                                                    int qp, int dpb0, Cell *__restrict__ cells)
{
    const int i = blockIdx.x;
    if (i >= n) return;
    const RqtUnit u = units[i];
    const int x4 = u.x0 >> 2, y4 = u.y0 >> 2, n4 = (1 << u.log2_size) >> 2, half = n4 >> 1;
    const int32_t packed = field[(long)y4 * cw + x4];
    const RqtResult &d = dec[i];
    const bool split = d.depth == 1, coded0 = d.tried_zero == 1 && d.zero.cbf != 0;
    for (int t = threadIdx.x; t < n4 * n4; t += 64)
    {
        const int y = t / n4, x = t - y * n4;
        Cell c = Cell();
        c.mv[0][0] = (int16_t)(packed & 0xffff);
        c.mv[0][1] = (int16_t)(packed >> 16);
        c.dpb_index[0] = (int8_t)dpb0;
        c.dpb_index[1] = -1;
        c.qp_y = (int8_t)qp;
        const bool coded = split ? d.one[(y >= half) * 2 + (x >= half)].cbf != 0 : coded0;
        c.flags = (uint8_t)((coded ? 2 : 0) | (x == 0 ? 8 : 0) | (y == 0 ? 16 : 0));      // HAVOC_CELL_CODED, _PU_LEFT, _PU_TOP
        c.tu_log2 = (uint8_t)(u.log2_size - (split ? 1 : 0));
        cells[(long)(y4 + y) * cw + x4 + x] = c;
    }
}

hipError_t launch_rqt_decide(hipStream_t st, const RqtUnit *units, int n, const int32_t *zeroAt, const int32_t *oneAt, const RqtSize sizes[4], long recOrigin, int recStride, int dumpOff,
                             int32_t rlQ16, RqtResult *out, const int64_t *const *rates)
{
    if (n <= 0) return hipSuccess;
    const RqtSizes z{{sizes[0], sizes[1], sizes[2], sizes[3]}};
    if (rates)
        hipLaunchKernelGGL(k_rqt_decide<kRqtRated>, dim3((n + 255) / 256), dim3(256), 0, st, units, n, zeroAt, oneAt, z,
                           RqtRates{{rates[0], rates[1], rates[2], rates[3]}}, RqtTree(), recOrigin, recStride, dumpOff, rlQ16, out);
    else
        hipLaunchKernelGGL(k_rqt_decide<kRqtStandIn>, dim3((n + 255) / 256), dim3(256), 0, st, units, n, zeroAt, oneAt, z, RqtRates(), RqtTree(), recOrigin, recStride, dumpOff,
                           rlQ16, out);
    return hipGetLastError();
}

hipError_t launch_rqt_decide_tree(hipStream_t st, const RqtUnit *units, int n, const int32_t *zeroAt, const int32_t *oneAt, const RqtSize sizes[4], const RqtSize csizes[4],
                                  const havoc_mi355x_rqt_chroma_at *chromaAt, const int64_t *treeRate, const uint32_t *treeCbf, long recOrigin, int recStride, int dumpOff,
                                  long cbOrigin, long crOrigin, int cStride, int cDump, int32_t rlQ16, RqtResult *out, havoc_mi355x_rqt_tree_choice *treeOut)
{
    if (n <= 0) return hipSuccess;
    const RqtSizes z{{sizes[0], sizes[1], sizes[2], sizes[3]}};
    const RqtTree tree{{{csizes[0], csizes[1], csizes[2], csizes[3]}}, chromaAt, treeRate, treeCbf, cbOrigin, crOrigin, cStride, cDump, treeOut};
    hipLaunchKernelGGL(k_rqt_decide<kRqtTree>, dim3((n + 255) / 256), dim3(256), 0, st, units, n, zeroAt, oneAt, z, RqtRates(), tree, recOrigin, recStride, dumpOff, rlQ16, out);
    return hipGetLastError();
}

hipError_t launch_rqt_decide_units(hipStream_t st, const RqtUnit *units, int n, const int32_t *zeroAt, const int32_t *oneAt, const RqtSize sizes[4], const RqtSize csizes[4],
                                   const havoc_mi355x_rqt_chroma_at *chromaAt, const int64_t *treeRate, const uint32_t *treeCbf, int32_t rlQ16, RqtResult *out,
                                   havoc_mi355x_rqt_tree_choice *treeOut)
{
    if (n <= 0) return hipSuccess;
    const RqtSizes z{{sizes[0], sizes[1], sizes[2], sizes[3]}};
    const RqtTree tree{{{csizes[0], csizes[1], csizes[2], csizes[3]}}, chromaAt, treeRate, treeCbf, 0, 0, 0, 0, treeOut};
    hipLaunchKernelGGL(k_rqt_decide<kRqtUnits>, dim3((n + 255) / 256), dim3(256), 0, st, units, n, zeroAt, oneAt, z, RqtRates(), tree, 0L, 0, 0, rlQ16, out);
    return hipGetLastError();
}

hipError_t launch_block_cells(hipStream_t st, int width, int height, int qp, int dpb0, const int16_t *field, const RqtUnit *units, const RqtResult *dec, int n, Cell *cells, bool blank)
{
    const int cw = width >> 2, ch = height >> 2;
    if (blank)
        hipLaunchKernelGGL(k_block_cells_blank, dim3((cw * ch + 255) / 256), dim3(256), 0, st, cells, cw * ch, qp, dpb0);
    if (n > 0)
        hipLaunchKernelGGL(k_block_cells, dim3(n), dim3(64), 0, st, units, dec, n, reinterpret_cast<const int32_t *>(field), cw, qp, dpb0, cells);
    return hipGetLastError();
}

// ---- an intra picture's partitions with their REAL dependencies (round 4; turing/Reconstruct.cpp:609-615, CandModeList.h:33-95) ----------------------------
// A partition predicts from the RECONSTRUCTION of what precedes it and takes its most probable modes from its neighbours' champions, so the partitions of
// a picture form a dependency graph; the host cuts it into levels (partitions whose neighbours are all final) and runs the batch chain level by level.
// What a level needs from the picture's running state is made here, on the device:
//   k_intra_gather   per partition: the 4n + 1 reference samples from the reconstruction picture with the substitution process of HEVC 8.4.4.2.2 for the
//                    ones not yet coded / outside the picture (availability = "the 4x4 cell's owner precedes me in coding order"), their filtered copy ([1 2 1], or the bi-linear
//                    strong smoothing of a flat 32x32 block's edges: IntraReferenceSamples.h:373-421), and candModeList from the modes decided left of and above it (CandModeList.h)
//   k_intra_commit   per partition: the champion's reconstruction into the picture, its mode into the mode map
using ChainPart = havoc_mi355x_intra_chain_part;
using ChainLayout = havoc_mi355x_intra_chain_layout;

template <int S>
__global__ __launch_bounds__(64) void k_intra_gather(const ChainLayout L, const char *__restrict__ recv, const int32_t *__restrict__ owner, const uint8_t *__restrict__ modes,
                                                     const ChainPart *__restrict__ parts, int n, const SearchJob *__restrict__ jobs, char *__restrict__ nbv,
                                                     IntraCtx *__restrict__ ictx)
{
    typedef typename Sample<S>::T T;
    __shared__ int32_t val[132];
    __shared__ uint8_t have[132];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const ChainPart p = parts[i];
    const SearchJob job = jobs[i];
    const T *rec = reinterpret_cast<const T *>(recv);
    T *nb = reinterpret_cast<T *>(nbv);
    const int nn = 1 << p.log2, len = 4 * nn + 1;
    auto available = [&](int x, int y) {
        return x >= 0 && y >= 0 && x < L.pic_width && y < L.pic_height && owner[(y >> 2) * L.cells_per_row + (x >> 2)] < p.index;
    };
    for (int k = lane; k < len; k += 64)
    {   // k < 2n: the left column from the bottom; 2n: the corner; beyond: the row above
        const int x = k <= 2 * nn ? p.x0 - 1 : p.x0 + k - 2 * nn - 1;
        const int y = k < 2 * nn ? p.y0 + 2 * nn - 1 - k : p.y0 - 1;
        const bool a = available(x, y);
        have[k] = a;
        val[k] = a ? (int)rec[(long)(y + L.pad) * L.stride + x + L.pad] : 0;
    }
    __syncthreads();
    if (lane == 0)
    {   // 8.4.4.2.2: nothing there -> mid grey; else the first sample takes the first one there is, every other missing one its predecessor
        int first = 0;
        while (first < len && !have[first]) ++first;
        if (first == len)
            for (int k = 0; k < len; ++k) val[k] = 1 << (L.bit_depth - 1);
        else
        {
            if (first) val[0] = val[first];
            for (int k = 1; k < len; ++k)
                if (!have[k]) val[k] = val[k - 1];
        }
    }
    __syncthreads();
    const long base = job.nb_off - (2 * nn + 1), basef = job.nbf_off - (2 * nn + 1);
    // IntraReferenceSamples.h:382-402 (HEVC 8.4.4.2.3): a 32x32 block whose two edges are nearly linear takes the bi-linear interpolation between the corner
    // and the ends instead of the [1 2 1] filter (strong_intra_smoothing_enabled_flag, on by default: Encoder.cpp:688)
    const int corner = val[2 * nn], thr = 1 << (L.bit_depth - 5);
    const bool strong = L.strong_intra_smoothing == 1 && nn == 32 && abs(corner + val[4 * nn] - 2 * val[3 * nn]) < thr && abs(corner + val[0] - 2 * val[nn]) < thr;
    for (int k = lane; k < len; k += 64)
    {
        nb[base + k] = (T)val[k];
        int f;
        if (strong)      // k <= 64: the left column from the bottom (k = 63 - y), corner at 64; beyond: the row above (x = k - 65)
            f = k < 64 ? (k * corner + (64 - k) * val[0] + 32) >> 6 : k == 64 ? corner : ((128 - k) * corner + (k - 64) * val[128] + 32) >> 6;
        else
            f = (k == 0 || k == len - 1) ? val[k] : (val[k - 1] + 2 * val[k] + val[k + 1] + 2) >> 2;
        nb[basef + k] = (T)f;
    }
    if (lane == 0)
    {   // CandModeList.h:33-95: A = left, B = above (DC when not there, or above in another CTU row)
        const int a = available(p.x0 - 1, p.y0) ? modes[(p.y0 >> 2) * L.cells_per_row + ((p.x0 - 1) >> 2)] : 1;
        const int b = available(p.x0, p.y0 - 1) && (p.y0 - 1) >= ((p.y0 >> L.ctb_log2) << L.ctb_log2) ? modes[((p.y0 - 1) >> 2) * L.cells_per_row + (p.x0 >> 2)] : 1;
        IntraCtx c = ictx[i];
        int cand[3];
        c.neighbour_modes = havoc_search::candModeListOf(a, b, cand);      // (search/cand_mode_list.hpp: pinned against the encoder's own lists)
        c.cand_mode_list[0] = cand[0]; c.cand_mode_list[1] = cand[1]; c.cand_mode_list[2] = cand[2];
        ictx[i] = c;
    }
}

template <int S>
__global__ __launch_bounds__(256) void k_intra_commit(const ChainLayout L, char *__restrict__ recv, uint8_t *__restrict__ modes, const ChainPart *__restrict__ parts, int n,
                                                      const char *__restrict__ blocksv, const int32_t *__restrict__ choice, int choiceStride)
{
    typedef typename Sample<S>::T T;
    const int i = blockIdx.x;
    if (i >= n) return;
    const ChainPart p = parts[i];
    const int nn = 1 << p.log2, area = nn * nn;
    const T *blk = reinterpret_cast<const T *>(blocksv) + (long)i * area;
    T *rec = reinterpret_cast<T *>(recv);
    for (int t = threadIdx.x; t < area; t += 256)
    {
        const int y = t >> p.log2, x = t & (nn - 1);
        rec[(long)(p.y0 + y + L.pad) * L.stride + p.x0 + x + L.pad] = blk[t];
    }
    const int cw = nn >> 2, mode = choice[(long)i * choiceStride];      // a plain array of modes (stride 1) or the choice records (stride 10: `mode` leads)
    for (int t = threadIdx.x; t < cw * cw; t += 256)
        modes[((p.y0 >> 2) + t / cw) * L.cells_per_row + (p.x0 >> 2) + t % cw] = (uint8_t)mode;
}

// the candidate slots [total[0], capacity) nobody was given: copies of slot 0's records that write into their OWN slots, so that the chain can be launched over
// `capacity` jobs without the host first learning how many candidates there are (an intra picture's levels: thousands of small batches, no wait between them)
__global__ __launch_bounds__(256) void k_intra_fill_spare(const int32_t *__restrict__ total, int capacity, int log2, IntraJob *__restrict__ ij, TuJob *__restrict__ tj,
                                                          RdoqJob *__restrict__ rj, int32_t *__restrict__ sj, int32_t *__restrict__ owner)
{
    const int c = total[0] + blockIdx.x * 256 + threadIdx.x;
    if (c >= capacity || total[0] <= 0) return;
    const int area = 1 << (2 * log2);
    IntraJob a = ij[0];
    a.dst_off = c * area;
    ij[c] = a;
    const TuJob b = {c * area, tj[0].src_off, c * area, c * area};
    tj[c] = b;
    RdoqJob r = rj[0];
    r.dst_off = r.src_off = c * area;
    rj[c] = r;
    sj[2 * c] = c * area;
    sj[2 * c + 1] = area;
    owner[c] = owner[0];
}

hipError_t launch_intra_fill_spare(hipStream_t st, const int32_t *total, int capacity, int log2, IntraJob *ij, TuJob *tj, RdoqJob *rj, int32_t *sj, int32_t *owner)
{
    if (capacity <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_intra_fill_spare, dim3((capacity + 255) / 256), dim3(256), 0, st, total, capacity, log2, ij, tj, rj, sj, owner);
    return hipGetLastError();
}

hipError_t launch_intra_gather(hipStream_t st, int S, const ChainLayout *layout, const void *rec, const int32_t *owner, const uint8_t *modes, const ChainPart *parts, int n,
                               const SearchJob *jobs, void *nb, IntraCtx *ictx)
{
    if (n <= 0) return hipSuccess;
    if (S == 1) hipLaunchKernelGGL((k_intra_gather<1>), dim3(n), dim3(64), 0, st, *layout, (const char *)rec, owner, modes, parts, n, jobs, (char *)nb, ictx);
    else hipLaunchKernelGGL((k_intra_gather<2>), dim3(n), dim3(64), 0, st, *layout, (const char *)rec, owner, modes, parts, n, jobs, (char *)nb, ictx);
    return hipGetLastError();
}

hipError_t launch_intra_commit(hipStream_t st, int S, const ChainLayout *layout, void *rec, uint8_t *modes, const ChainPart *parts, int n, const void *blocks, const int32_t *choice,
                               int choiceStride)
{
    if (n <= 0) return hipSuccess;
    if (S == 1) hipLaunchKernelGGL((k_intra_commit<1>), dim3(n), dim3(256), 0, st, *layout, (char *)rec, modes, parts, n, (const char *)blocks, choice, choiceStride);
    else hipLaunchKernelGGL((k_intra_commit<2>), dim3(n), dim3(256), 0, st, *layout, (char *)rec, modes, parts, n, (const char *)blocks, choice, choiceStride);
    return hipGetLastError();
}

// ---- job tables made ON THE DEVICE from the decided motion field (round 4): what a host would otherwise build per picture and upload -----------------
// The prediction jobs of the steps that follow the searches -- every unit at its decided vector (luma 8-tap, chroma 4-tap), every unit's spatial merge
// candidates bi-directionally in three planes -- depend on the field the search kernel has just left in device memory; building them there keeps the
// picture's step free of host work between its launches.  Layout of the pictures: planes of one component at multiples of `planeElems` (luma: source, list 0,
// list 1; chroma: Cb source, list 0, list 1, then Cr source, list 0, list 1), `pad` samples of border, `stride` samples per row.
using MergeLayout = havoc_mi355x_field_layout;
using PredBiJob = havoc_mi355x_pred_bi_job;

__device__ __forceinline__ void clampVector(const MergeLayout &L, int x0, int y0, int n, int &mx, int &my)
{   // as LimitFullPelMv (Search.hpp:1366-1407) keeps the searches: the block stays within `range` samples of the picture (quarter-sample units)
    mx = min(max(mx, (-L.range - x0) * 4), (L.pic_width + L.range - x0 - n) * 4);
    my = min(max(my, (-L.range - y0) * 4), (L.pic_height + L.range - y0 - n) * 4);
}

// thread = (unit, candidate k of 5): the vectors of both lists at spatial merge position k (HEVC 8.5.3.2.3: A1, B1, B0, A0, B2; outside the picture: zero)
__global__ __launch_bounds__(256) void k_merge_jobs(const MergeLayout L, const int32_t *__restrict__ field, const int32_t *__restrict__ ux, const int32_t *__restrict__ uy, int n,
                                                    int log2, PredBiJob *__restrict__ jl, PredBiJob *__restrict__ jcb, PredBiJob *__restrict__ jcr, int32_t *__restrict__ vectors)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 5 * n) return;
    const int i = t / 5, k = t - 5 * i, nn = 1 << log2, x0 = ux[i], y0 = uy[i];
    const int px = k == 0 || k >= 3 ? x0 - 1 : (k == 1 ? x0 + nn - 1 : x0 + nn);
    const int py = k == 0 ? y0 + nn - 1 : (k == 3 ? y0 + nn : y0 - 1);
    const bool inside = px >= 0 && py >= 0 && px < L.pic_width && py < L.pic_height;
    const int ch = (L.pic_height + 3) >> 2;
    int mv[2][2];
    for (int lst = 0; lst < 2; ++lst)
    {
        const int32_t packed = inside ? field[((long)lst * ch + (py >> 2)) * L.field_cw + (px >> 2)] : 0;
        mv[lst][0] = (int16_t)(packed & 0xffff);
        mv[lst][1] = (int16_t)(packed >> 16);
        clampVector(L, x0, y0, nn, mv[lst][0], mv[lst][1]);
        vectors[2 * t + lst] = (mv[lst][0] & 0xffff) | (mv[lst][1] << 16);
    }
    {
        PredBiJob j = PredBiJob();
        j.dst_off = t * nn * nn;
        j.w = j.h = nn;
        const int here = (y0 + L.luma_pad) * L.luma_stride + x0 + L.luma_pad;
        j.ref0_off = 1 * L.luma_plane_elems + here + (mv[0][1] >> 2) * L.luma_stride + (mv[0][0] >> 2);
        j.ref1_off = 2 * L.luma_plane_elems + here + (mv[1][1] >> 2) * L.luma_stride + (mv[1][0] >> 2);
        j.xFrac0 = mv[0][0] & 3; j.yFrac0 = mv[0][1] & 3; j.xFrac1 = mv[1][0] & 3; j.yFrac1 = mv[1][1] & 3;
        jl[t] = j;
    }
    for (int comp = 0; comp < 2; ++comp)
    {
        PredBiJob j = PredBiJob();
        const int cn = nn >> 1;
        j.dst_off = t * cn * cn;
        j.w = j.h = cn;
        const int here = ((y0 >> 1) + L.chroma_pad) * L.chroma_stride + (x0 >> 1) + L.chroma_pad;
        j.ref0_off = (3 * comp + 1) * L.chroma_plane_elems + here + (mv[0][1] >> 3) * L.chroma_stride + (mv[0][0] >> 3);
        j.ref1_off = (3 * comp + 2) * L.chroma_plane_elems + here + (mv[1][1] >> 3) * L.chroma_stride + (mv[1][0] >> 3);
        j.xFrac0 = mv[0][0] & 7; j.yFrac0 = mv[0][1] & 7; j.xFrac1 = mv[1][0] & 7; j.yFrac1 = mv[1][1] & 7;
        (comp ? jcr : jcb)[t] = j;
    }
}

// thread = unit: its HavocPredUni job at the vector decided for list `list` at its origin; plane 0 = luma (8-tap phases), 1 / 2 = Cb / Cr (eighth-sample phases)
__global__ __launch_bounds__(256) void k_pred_jobs(const MergeLayout L, const int32_t *__restrict__ field, int list, const int32_t *__restrict__ ux, const int32_t *__restrict__ uy,
                                                   int n, int log2, int plane, const int32_t *__restrict__ dstOff, havoc_mi355x_pred_uni_job *__restrict__ jobs)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x0 = ux[i], y0 = uy[i], ch = (L.pic_height + 3) >> 2;
    const int32_t packed = field[((long)list * ch + (y0 >> 2)) * L.field_cw + (x0 >> 2)];
    const int mx = (int16_t)(packed & 0xffff), my = (int16_t)(packed >> 16);
    havoc_mi355x_pred_uni_job j = havoc_mi355x_pred_uni_job();
    j.dst_off = dstOff[i];
    if (plane == 0)
    {
        j.w = j.h = 1 << log2;
        j.ref_off = (1 + list) * L.luma_plane_elems + (y0 + (my >> 2) + L.luma_pad) * L.luma_stride + x0 + (mx >> 2) + L.luma_pad;
        j.xFrac = mx & 3; j.yFrac = my & 3;
    }
    else
    {
        j.w = j.h = 1 << (log2 - 1);
        j.ref_off = (3 * (plane - 1) + 1 + list) * L.chroma_plane_elems + ((y0 >> 1) + (my >> 3) + L.chroma_pad) * L.chroma_stride + (x0 >> 1) + (mx >> 3) + L.chroma_pad;
        j.xFrac = mx & 7; j.yFrac = my & 7;
    }
    jobs[i] = j;
}

// thread = unit: cost of its five candidates = stand-in rate of the merge index (k + 1 bits, 4 at most) + (satdY + satdCb + satdCr) * reciprocalSqrtLambda (Q16: measurePuCost,
// Search.hpp:1659-1706), best = the first of the cheapest (`cost < bestCost`, searchMergeModes :1754-1768)
__global__ __launch_bounds__(256) void k_merge_decide(const int32_t *__restrict__ sy, const int32_t *__restrict__ scb, const int32_t *__restrict__ scr, int n, int64_t lamQ16,
                                                      int64_t *__restrict__ cost, int32_t *__restrict__ best)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int64_t bestCost = 0;
    int b = 0;
    for (int k = 0; k < 5; ++k)
    {
        const int t = 5 * i + k;
        const int64_t c = ((int64_t)min(k + 1, 4) << 16) + ((int64_t)sy[t] + scb[t] + scr[t]) * lamQ16;
        cost[t] = c;
        if (k == 0 || c < bestCost) { bestCost = c; b = k; }
    }
    best[i] = b;
}

hipError_t launch_merge_decide(hipStream_t st, const int32_t *sy, const int32_t *scb, const int32_t *scr, int n, int64_t lamQ16, int64_t *cost, int32_t *best)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_merge_decide, dim3((n + 255) / 256), dim3(256), 0, st, sy, scb, scr, n, lamQ16, cost, best);
    return hipGetLastError();
}

hipError_t launch_merge_jobs(hipStream_t st, const MergeLayout *layout, const int16_t *field, const int32_t *ux, const int32_t *uy, int n, int log2, PredBiJob *jl, PredBiJob *jcb, PredBiJob *jcr,
                             int16_t *vectors)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_merge_jobs, dim3((5 * n + 255) / 256), dim3(256), 0, st, *layout, reinterpret_cast<const int32_t *>(field), ux, uy, n, log2, jl, jcb, jcr,
                       reinterpret_cast<int32_t *>(vectors));
    return hipGetLastError();
}

hipError_t launch_pred_jobs(hipStream_t st, const MergeLayout *layout, const int16_t *field, int list, const int32_t *ux, const int32_t *uy, int n, int log2, int plane,
                            const int32_t *dstOff, havoc_mi355x_pred_uni_job *jobs)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pred_jobs, dim3((n + 255) / 256), dim3(256), 0, st, *layout, reinterpret_cast<const int32_t *>(field), list, ux, uy, n, log2, plane, dstOff, jobs);
    return hipGetLastError();
}

hipError_t launch_intra_order(hipStream_t st, const int32_t *satd35, const IntraCtx *ictx, int n, int32_t lambdaQ16, int32_t *order, int32_t *count, int32_t *slot,
                              int32_t *total)
{
    if (n <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(total, 0, 8, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_intra_order, dim3((n + 63) / 64), dim3(64), 0, st, satd35, ictx, n, lambdaQ16, order, count, slot, total);
    return hipGetLastError();
}

hipError_t launch_intra_expand(hipStream_t st, const SearchJob *parts, const int32_t *order, const int32_t *count, const int32_t *slot, const int32_t *ctxIndex, int n, int log2,
                               int quantScale, int quantShift, int invScale, int lambdaQ16, int sdhFactor, int sdh, IntraJob *ij, TuJob *tj, RdoqJob *rj, int32_t *sj,
                               int32_t *owner)
{
    if (n <= 0) return hipSuccess;
    const long threads = (long)n * kMaxOrder;
    hipLaunchKernelGGL(k_intra_expand, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, parts, order, count, slot, ctxIndex, n, log2, quantScale,
                       quantShift, invScale, lambdaQ16, sdhFactor, sdh, ij, tj, rj, sj, owner);
    return hipGetLastError();
}

hipError_t launch_intra_decide(hipStream_t st, const IntraCtx *ictx, const int32_t *order, const int32_t *count, const int32_t *slot, const int32_t *cbf, const uint32_t *ssd,
                               const int32_t *stats, const TuJob *tj, int n, int log2, int32_t reciprocalLambdaQ16, havoc_mi355x_intra_choice *out, TuJob *fin,
                               const int64_t *rates)
{
    if (n <= 0) return hipSuccess;
    if (rates)
        hipLaunchKernelGGL(k_intra_decide<true>, dim3((n + 255) / 256), dim3(256), 0, st, ictx, order, count, slot, cbf, ssd, stats, rates, tj, n, log2,
                           reciprocalLambdaQ16, out, fin);
    else
        hipLaunchKernelGGL(k_intra_decide<false>, dim3((n + 255) / 256), dim3(256), 0, st, ictx, order, count, slot, cbf, ssd, stats, rates, tj, n, log2,
                           reciprocalLambdaQ16, out, fin);
    return hipGetLastError();
}

hipError_t launch_intra_rate_jobs(hipStream_t st, const IntraCtx *ictx, const int32_t *order, const int32_t *count, const int32_t *slot, const RdoqJob *rj, int n, int flags,
                                  havoc_mi355x_intra_rate_job *out)
{
    if (n <= 0) return hipSuccess;
    const long threads = (long)n * kMaxOrder;
    hipLaunchKernelGGL(k_intra_rate_jobs, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, ictx, order, count, slot, rj, n, flags, out);
    return hipGetLastError();
}

} // namespace havoc_gpu
