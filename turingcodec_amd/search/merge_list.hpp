// merge_list.hpp -- a prediction unit's merge candidate list (HEVC 8.5.3.2.2 - 8.5.3.2.5 as turing/Mvp.h:486-716 applies it) as PRODUCT text: compiled into
// k_cqt_merge_lists (csrc/kernels_merge.hip) and into the host clients, one function for both (cqtMergeList), as amvp.hpp's temporalCandidateOf is for
// k_temporal_candidates.  DESIGN 7, row f2^12.
//
// The rule itself (deriveMergeCandidateList) is this project's second statement of it: the first, tests/merge.hpp, is pinned against 41 880 lists of six traced
// encodes and stays test infrastructure; the product includes nothing from tests/, so the text stands here again under names of its own (namespace
// havoc_search::merge_list, MergeCand) -- both headers fit into one translation unit, and tests/test_merge_list.py holds them against each other on 400 000 random
// rows and against the encoder's own recorded lists.
//
// THE FORM.  A lane of the kernel keeps the five neighbours and the list in registers, so NOTHING here is indexed by a run-time value: every loop has a constant
// trip count and is unrolled, `out[n++] = m` is putCand (a select per place), the combined candidates' `out[l0Idx[c]]` has c unrolled into constants, and the picture
// order counts behind a reference index come through a functor (the committed picture has one reference per list: its functor ignores the index).  Indexed by a
// run-time value such records go to scratch memory or into LDS (row f2^10 records 12 KB of LDS for colocatedVector's cells before it was rewritten with selects).
#pragma once

#include "picture_order.hpp"

namespace havoc_search {
namespace merge_list {

struct MergeCand
{
    bool predFlag[2] = {false, false};
    int refIdx[2] = {0, 0};
    Mv mv[2];
    HAVOC_HD bool available() const { return predFlag[0] || predFlag[1]; }      // PuData::isAvailable: coded and not intra
    // PuData::operator== (turing/BlockData.h:82-95): per list the same reference index (or both unused) and, where used, the same vector
    HAVOC_HD bool same(const MergeCand &o) const
    {
        bool eq = true;
        HAVOC_UNROLL
        for (int l = 0; l < 2; ++l)
        {
            if (predFlag[l] != o.predFlag[l]) eq = false;
            if (predFlag[l] && (refIdx[l] != o.refIdx[l] || mv[l] != o.mv[l])) eq = false;
        }
        return eq;
    }
};

// out[n] = m without an index: n is a run-time value, the places are not.  Every place is STORED, unconditionally, with a value chosen per field: five conditional
// stores of one record the compiler merges into one store through a chosen ADDRESS, and the list is back in memory (112 bytes of scratch per lane, measured)
HAVOC_HD inline void putCand(MergeCand out[5], int n, const MergeCand &m)
{
    HAVOC_UNROLL
    for (int k = 0; k < 5; ++k)
    {
        const bool hit = k == n;
        HAVOC_UNROLL
        for (int l = 0; l < 2; ++l)
        {
            out[k].predFlag[l] = hit ? m.predFlag[l] : out[k].predFlag[l];
            out[k].refIdx[l] = hit ? m.refIdx[l] : out[k].refIdx[l];
            out[k].mv[l].x = hit ? m.mv[l].x : out[k].mv[l].x;
            out[k].mv[l].y = hit ? m.mv[l].y : out[k].mv[l].y;
        }
    }
}

// picture order counts of the lists' entries, looked up in two tables (the general caller) ...
struct PocTables
{
    const int *poc0, *poc1;
    HAVOC_HD int operator()(int list, int refIdx) const { return list ? poc1[refIdx] : poc0[refIdx]; }
};
// ... or one picture per list (reference index 0 is the only one)
struct PocPair
{
    int poc0, poc1;
    HAVOC_HD int operator()(int list, int) const { return list ? poc1 : poc0; }
};

// one combined bi-predictive candidate, combIdx C: list 0 of out[I0] with list 1 of out[I1], unless both name the same picture with the same vector
template <int C, int I0, int I1, class Poc>
HAVOC_HD inline void combineCands(MergeCand out[5], int &n, int combMax, int maxCand, Poc poc)
{
    if (C < combMax && n < maxCand)
    {
        const MergeCand p = out[I0], q = out[I1];
        if (p.predFlag[0] && q.predFlag[1] && (poc(0, p.refIdx[0]) != poc(1, q.refIdx[1]) || p.mv[0] != q.mv[1]))
        {
            MergeCand m = p;
            m.predFlag[1] = true;
            m.refIdx[1] = q.refIdx[1];
            m.mv[1] = q.mv[1];
            putCand(out, n++, m);
        }
    }
}

// nb[0..4] = A1 (left), B1 (above), B0 (above-right), A0 (below-left), B2 (above-left) as the neighbour fetch returned them (not available = no prediction flags);
// partIdx / nPbW / nPbH = the prediction unit after the parallel-merge-level adjustment (the second unit of an Nx2N-like split may not take A1, of a 2NxN-like split
// B1: they would rebuild the 2Nx2N unit), nOrigPbW / nOrigPbH = the unit's own size (step 10, Mvp.h:709-716: an 8x4 / 4x8 unit is never bi-predicted -- its candidates
// keep list 0 only); col = the temporal candidate (reference index 0 in every list it has); poc(list, refIdx) = the picture order count of a list's entry, compared for
// equality only; maxCand 1..5; out[0 .. maxCand - 1] are written, every other place is left as it was.  Returns the number of candidates that came from neighbours,
// the temporal candidate and their combinations (the rest are zero vectors).
template <class Poc>
HAVOC_HD inline int deriveMergeCandidateList(const MergeCand nb[5], int partIdx, int nPbW, int nPbH, int nOrigPbW, int nOrigPbH, bool colAvailable, const MergeCand &col,
                                             bool sliceB, int numRef0, int numRef1, Poc poc, int maxCand, MergeCand out[5])
{
    int n = 0, real = -1;
    const MergeCand none;
    // spatial candidates, each compared with the neighbours the standard names -- with what was FETCHED there, taken into the list or not
    const bool takeA1 = !(partIdx && nPbW < nPbH), takeB1 = !(partIdx && nPbH < nPbW);
    MergeCand a1 = nb[0], b1 = nb[1];           // (copies, then overwritten: a choice between two OBJECTS is a pointer the compiler must keep in memory)
    if (!takeA1) a1 = none;
    if (!takeB1) b1 = none;
    if (a1.available()) putCand(out, n++, a1);
    if (n < maxCand && b1.available() && !a1.same(b1)) putCand(out, n++, b1);
    if (n < maxCand && nb[2].available() && !nb[2].same(b1)) putCand(out, n++, nb[2]);
    if (n < maxCand && nb[3].available() && !nb[3].same(a1)) putCand(out, n++, nb[3]);
    if (n < maxCand && n != 4 && nb[4].available() && !nb[4].same(a1) && !nb[4].same(b1)) putCand(out, n++, nb[4]);
    if (n < maxCand && colAvailable) putCand(out, n++, col);
    // combined bi-predictive candidates (B slices): list 0 of one candidate with list 1 of another, unless both name the same picture with the same vector
    if (n < maxCand && sliceB)
    {
        // combIdx 0..11 in the standard's order (l0CandIdx, l1CandIdx); every one reads places below the number of candidates the step started with
        const int combMax = n * (n - 1);
        combineCands<0, 0, 1>(out, n, combMax, maxCand, poc);
        combineCands<1, 1, 0>(out, n, combMax, maxCand, poc);
        combineCands<2, 0, 2>(out, n, combMax, maxCand, poc);
        combineCands<3, 2, 0>(out, n, combMax, maxCand, poc);
        combineCands<4, 1, 2>(out, n, combMax, maxCand, poc);
        combineCands<5, 2, 1>(out, n, combMax, maxCand, poc);
        combineCands<6, 0, 3>(out, n, combMax, maxCand, poc);
        combineCands<7, 3, 0>(out, n, combMax, maxCand, poc);
        combineCands<8, 1, 3>(out, n, combMax, maxCand, poc);
        combineCands<9, 3, 1>(out, n, combMax, maxCand, poc);
        combineCands<10, 2, 3>(out, n, combMax, maxCand, poc);
        combineCands<11, 3, 2>(out, n, combMax, maxCand, poc);
    }
    real = n;
    // zero vectors: one per reference index the lists share, then index 0 (at most five places are left: five rounds cover both loops of the rule)
    const int numRef = sliceB && numRef1 < numRef0 ? numRef1 : numRef0;
    HAVOC_UNROLL
    for (int z = 0; z < 5; ++z)
        if (n < maxCand)
        {
            MergeCand m;
            m.predFlag[0] = true;
            m.refIdx[0] = z < numRef ? z : 0;
            if (sliceB) { m.predFlag[1] = true; m.refIdx[1] = m.refIdx[0]; }
            putCand(out, n++, m);
        }
    if (nOrigPbW + nOrigPbH == 12)
    {
        HAVOC_UNROLL
        for (int k = 0; k < 5; ++k)
            if (k < maxCand && out[k].predFlag[0] && out[k].predFlag[1])
            {
                out[k].predFlag[1] = false;
                out[k].refIdx[1] = 0;
                out[k].mv[1] = Mv(0, 0);
            }
    }
    return real;
}

// ---- the list of a committed picture's final coding unit (havoc_mi355x_cqt_merge_lists; the rule of the fetch is stated in include/havoc_mi355x.h) ----
struct CqtMergeParams           // = havoc_mi355x_merge_params, 48 bytes
{
    int32_t picWidth, picHeight, ctbLog2, minCbLog2, maxCand, refPoc[2], reserved[5];
};
struct CqtMergeRecord           // = havoc_mi355x_merge_list, 64 bytes, as the eight aligned 8-byte words both forms store
{
    unsigned long long w[8];
};

// a committed cell (havoc_mi355x_cqt_cell: its second and third 8-byte words) as a neighbour: one inter 2Nx2N unit with reference index 0 in the lists it uses
HAVOC_HD inline MergeCand cqtCellMotion(unsigned long long mv, unsigned long long tail)
{
    const int pred = int(tail >> 16) & 255;
    MergeCand c;
    c.predFlag[0] = pred != 1;
    c.predFlag[1] = pred != 0;
    c.mv[0] = c.predFlag[0] ? Mv(int16_t(mv), int16_t(mv >> 16)) : Mv(0, 0);
    c.mv[1] = c.predFlag[1] ? Mv(int16_t(mv >> 32), int16_t(mv >> 48)) : Mv(0, 0);
    return c;
}

HAVOC_HD inline uint32_t packMv(Mv v) { return uint32_t(uint16_t(v.x)) | uint32_t(uint16_t(v.y)) << 16; }
// the j-th 4-byte word (0 list 0's vector, 1 list 1's vector, 2 pred_flag and ref_idx) of a havoc_mi355x_merge_cand; a place beyond the list is zero bytes
HAVOC_HD inline uint64_t candWord(const MergeCand &c, bool inList, int j)
{
    const uint32_t v = j == 0 ? packMv(c.mv[0])
                     : j == 1 ? packMv(c.mv[1])
                              : uint32_t(c.predFlag[0]) | uint32_t(c.predFlag[1]) << 8 | uint32_t(uint8_t(c.refIdx[0])) << 16 | uint32_t(uint8_t(c.refIdx[1])) << 24;
    return inList ? v : 0u;
}

// cells: the committed map as 8-byte words, three per cell, (picHeight >> minCbLog2) rows of (picWidth >> minCbLog2); temporal: the records of
// havoc_mi355x_temporal_candidates as 8-byte words, index 2 * unit + list, or nullptr (no temporal candidate); p, (x0, y0, w, h): the searched unit.
// Reads the unit's origin cell only when the unit's geometry can be a final unit's, a neighbour's cell only when neighbourPositionAvailable allows the position
// (which is then inside the picture), the temporal records only for a final unit: never anything outside the tables.
HAVOC_HD inline CqtMergeRecord cqtMergeList(const CqtMergeParams &P, const unsigned long long *cells, const unsigned long long *temporal, int p, int x0, int y0, int w,
                                            int h)
{
    CqtMergeRecord r;
    HAVOC_UNROLL
    for (int j = 0; j < 7; ++j) r.w[j] = 0;
    r.w[7] = 0x00ff0000ull << 32;                // n_cand 0, n_real 0, match -1, reserved 0: a unit that is not final
    int L = -1;
    HAVOC_UNROLL
    for (int l = 3; l <= 6; ++l)
        if (w == (1 << l)) L = l;
    const bool shaped = w == h && L >= P.minCbLog2 && L <= P.ctbLog2 && x0 >= 0 && y0 >= 0 && x0 <= P.picWidth - w && y0 <= P.picHeight - h && !((x0 | y0) & (w - 1));
    if (!shaped) return r;
    const long cw = P.picWidth >> P.minCbLog2;
    const unsigned long long *own = cells + 3 * (long(y0 >> P.minCbLog2) * cw + (x0 >> P.minCbLog2));
    const unsigned long long head = own[0], ownMv = own[1], ownTail = own[2];
    if (int(uint32_t(head)) != p || int(ownTail & 255) != L) return r;
    const MergeCand self = cqtCellMotion(ownMv, ownTail);

    havoc_picture_pu q = {x0, y0, w, h, 0, 0, 0, 0};
    const int xN[5] = {x0 - 1, x0 + w - 1, x0 + w, x0 - 1, x0 - 1};                  // A1, B1, B0, A0, B2 (Mvp.h:540-640)
    const int yN[5] = {y0 + h - 1, y0 - 1, y0 - 1, y0 + h, y0 - 1};
    MergeCand nb[5];
    HAVOC_UNROLL
    for (int k = 0; k < 5; ++k)
        if (neighbourPositionAvailable(q, 1 << P.ctbLog2, P.picWidth, P.picHeight, xN[k], yN[k]))
        {
            const unsigned long long *c = cells + 3 * (long(yN[k] >> P.minCbLog2) * cw + (xN[k] >> P.minCbLog2));
            const unsigned long long cHead = c[0], cMv = c[1], cTail = c[2];
            if (int(uint32_t(cHead)) >= 0) nb[k] = cqtCellMotion(cMv, cTail);       // unit -1: the CTU there is undecided -- all-ones bytes, nothing else means anything
        }
    MergeCand col;
    if (temporal)
    {
        const unsigned long long t0 = temporal[2 * long(p)], t1 = temporal[2 * long(p) + 1];
        col.predFlag[0] = int16_t(t0 >> 32) != 0;
        col.predFlag[1] = int16_t(t1 >> 32) != 0;
        col.mv[0] = col.predFlag[0] ? Mv(int16_t(t0), int16_t(t0 >> 16)) : Mv(0, 0);
        col.mv[1] = col.predFlag[1] ? Mv(int16_t(t1), int16_t(t1 >> 16)) : Mv(0, 0);
    }
    MergeCand out[5];
    const PocPair poc = {P.refPoc[0], P.refPoc[1]};
    const int real = deriveMergeCandidateList(nb, 0, w, h, w, h, col.available(), col, true, 1, 1, poc, P.maxCand, out);
    int match = -1;
    HAVOC_UNROLL
    for (int k = 4; k >= 0; --k)
        if (k < P.maxCand && out[k].same(self)) match = k;
    // five 12-byte candidates and the four count bytes as eight 8-byte words: candidate k is the 4-byte words 3 k .. 3 k + 2 (list 0's vector, list 1's, flags)
    const uint64_t tail = uint32_t(uint8_t(P.maxCand)) | uint32_t(uint8_t(real)) << 8 | uint32_t(uint8_t(match)) << 16;
    const int mc = P.maxCand;
    r.w[0] = candWord(out[0], 0 < mc, 0) | candWord(out[0], 0 < mc, 1) << 32;
    r.w[1] = candWord(out[0], 0 < mc, 2) | candWord(out[1], 1 < mc, 0) << 32;
    r.w[2] = candWord(out[1], 1 < mc, 1) | candWord(out[1], 1 < mc, 2) << 32;
    r.w[3] = candWord(out[2], 2 < mc, 0) | candWord(out[2], 2 < mc, 1) << 32;
    r.w[4] = candWord(out[2], 2 < mc, 2) | candWord(out[3], 3 < mc, 0) << 32;
    r.w[5] = candWord(out[3], 3 < mc, 1) | candWord(out[3], 3 < mc, 2) << 32;
    r.w[6] = candWord(out[4], 4 < mc, 0) | candWord(out[4], 4 < mc, 1) << 32;
    r.w[7] = candWord(out[4], 4 < mc, 2) | tail << 32;
    return r;
}

} // namespace merge_list
} // namespace havoc_search
