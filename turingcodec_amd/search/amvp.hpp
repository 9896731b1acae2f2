// amvp.hpp -- the reference's derivation of a prediction unit's two motion vector predictors (HEVC 8.5.3.2.6 / 8.5.3.2.7 as turing/Mvp.h:195-436 applies it),
// restated as DATA-ONLY code: what it reads of the encoder's state is handed in as five neighbour records and the temporal candidate.
//
// Why it is here: until round 5 picture_order.hpp's derivePredictors was a two-candidate stand-in (the cell left of the bottom-left sample, the cell
// above the top-right sample; it gives the encoder's predictors for 75 % of the recorded derivations) and every decision-path number depends on it.  This file is the real
// rule, PINNED: the traced reference encoder records, for every searchUni call, the five neighbours as its neighbourPuData() returned them, the temporal candidate and the
// two predictors it derived (the HAVOC_TRACE_AMVP trace point, inserted after Search.hpp:1779); tests/test_trace_pin.py requires deriveAmvp() to give the same two
// predictors for every record of six encodes (0 differ); the temporal candidate is derived below from the collocated picture's cells and pinned likewise.  picture_order.hpp's walk -- on the host and inside k_search_rows -- derives its predictors with it, from the five
// positions under the encoder's availability rules; the walk's neighbours are vectors of the same list into the same reference picture (no scaling); the temporal candidate is the walk's optional input (TemporalCand
// below, one record per (unit, list) as havoc_mi355x_temporal_candidates wrote it), absent unless the caller hands a table in.
#pragma once

#include "decision.hpp"

namespace havoc_search {

struct AmvpNeighbour
{
    bool available = false;      // neighbourPuData(...).isAvailable(): inside the picture / slice, already coded, not intra (turing/StateSpatial.h:208-260)
    bool predFlag[2] = {false, false};
    int refPoc[2] = {0, 0};      // picture order count of the reference picture the neighbour's list-l vector points into
    Mv mv[2];
};

// 8.5.3.2.7 (turing/Mvp.h: distScale): the vector of a candidate that points into another reference picture, scaled by the ratio of the picture distances
HAVOC_HD inline int amvpClip3(int lo, int hi, int v) { return v < lo ? lo : (v > hi ? hi : v); }
HAVOC_HD inline Mv amvpDistScale(Mv mv, int tD, int tB)
{
    const int td = amvpClip3(-128, 127, tD), tb = amvpClip3(-128, 127, tB);
    const int tx = (16384 + (td < 0 ? -td : td) / 2) / td;
    const int f = amvpClip3(-4096, 4095, (tb * tx + 32) >> 6);
    auto one = [f](int c) {
        const int p = f * c;
        const int a = ((p < 0 ? -p : p) + 127) >> 8;
        return amvpClip3(-32768, 32767, p < 0 ? -a : a);
    };
    return Mv(int16_t(one(mv.x)), int16_t(one(mv.y)));
}

// ---- the temporal candidate (8.5.3.2.8 / 8.5.3.2.9 as turing/Mvp.h:44-181 applies it), data-only: what it reads of the collocated picture is handed in as two of that
// picture's 16x16 motion cells.  PINNED with the rest: the traced encoder records the two cells with every predictMvp and every populateMergeCandidates, and
// tests/test_trace_pin.py requires the candidate (available or not, vector) the encoder derived -- per list, reference index 0 for merge -- from them.
struct ColocatedCell
{
    bool predFlag[2] = {false, false};      // neither: intra, or not coded
    Mv mv[2];
    int refPoc[2] = {0, 0};                 // picture order count of the picture its list-l vector points into
    bool longTerm[2] = {false, false};
};

// one cell's contribution for list X towards the picture `targetPoc` (short-term): Mvp.h:44-121
HAVOC_HD inline bool colocatedVector(const ColocatedCell &c, int X, int colPoc, int curPoc, int targetPoc, bool allBackwards, bool collocatedFromL0, Mv *out)
{
    *out = Mv(0, 0);
    if (!c.predFlag[0] && !c.predFlag[1]) return false;
    // which of the cell's vectors: its only one; with two, the current list's when every reference picture lies in the past, else the list the collocated picture is NOT taken from
    const int listCol = !c.predFlag[0] ? 1 : (!c.predFlag[1] ? 0 : (allBackwards ? X : (collocatedFromL0 ? 1 : 0)));
    // (selects, not c.x[listCol]: on the device a record indexed by a run-time value leaves the registers -- the compiler moved both cells into LDS)
    const bool colLongTerm = listCol ? c.longTerm[1] : c.longTerm[0];
    const int colRefPoc = listCol ? c.refPoc[1] : c.refPoc[0];
    const Mv colMv = listCol ? c.mv[1] : c.mv[0];
    if (colLongTerm) return false;      // (the target is a short-term picture: the reference encoder has no others)
    const int colPocDiff = colPoc - colRefPoc, currPocDiff = curPoc - targetPoc;
    // THIS PROJECT'S OWN RULE: a vector that points into the collocated picture itself (distance 0) counts as no motion.  The reference would divide by zero in
    // distScale; no conforming stream has the case (a picture does not predict from itself), so no trace can show it.
    if (colPocDiff == 0) return false;
    *out = colPocDiff == currPocDiff ? colMv : amvpDistScale(colMv, colPocDiff, currPocDiff);
    return true;
}

// the prediction unit's temporal candidate for list X: the cell at its bottom-right corner if that lies in the same CTU row and inside the picture and has motion, else the
// cell at its centre (Mvp.h:141-181)
HAVOC_HD inline bool deriveTemporalCandidate(int xPb, int yPb, int nPbW, int nPbH, int picW, int picH, int ctbLog2, const ColocatedCell &bottomRight, const ColocatedCell &centre,
                                             int X, int colPoc, int curPoc, int targetPoc, bool allBackwards, bool collocatedFromL0, Mv *out)
{
    const int xBr = xPb + nPbW, yBr = yPb + nPbH;
    bool available = false;
    if ((yPb >> ctbLog2) == (yBr >> ctbLog2) && yBr < picH && xBr < picW)
        available = colocatedVector(bottomRight, X, colPoc, curPoc, targetPoc, allBackwards, collocatedFromL0, out);
    if (!available) available = colocatedVector(centre, X, colPoc, curPoc, targetPoc, allBackwards, collocatedFromL0, out);
    return available;
}

// ---- the collocated motion store as plain data (turing/StateCollocatedMotion.h:51-122): one record per 16x16 luma samples, the motion of the unit that contains the
// area's top-left sample.  = havoc_mi355x_col_cell, 24 bytes; havoc_mi355x_cqt_motion_store writes it (host form: cqt_decision.hpp's cqtMotionStore),
// havoc_mi355x_temporal_candidates reads it through the two functions below -- the same text on the host and inside k_temporal_candidates.
struct ColStoreCell
{
    int16_t mv[2][2];
    int32_t refPoc[2];
    uint8_t predFlag[2], longTerm[2];
    uint32_t reserved;
};

HAVOC_HD inline ColocatedCell colocatedCellOf(const ColStoreCell &s)
{
    ColocatedCell c;
    HAVOC_UNROLL
    for (int l = 0; l < 2; ++l)
    {
        c.predFlag[l] = s.predFlag[l] != 0;
        c.mv[l] = Mv(s.mv[l][0], s.mv[l][1]);
        c.refPoc[l] = s.refPoc[l];
        c.longTerm[l] = s.longTerm[l] != 0;
    }
    return c;
}

struct TemporalParams           // = havoc_mi355x_temporal_params, 48 bytes
{
    int32_t picWidth, picHeight, ctbLog2, colPoc, curPoc, targetPoc[2], allBackwards, collocatedFromL0, reserved[3];
};
struct TemporalCand             // = havoc_mi355x_temporal_cand, 8 bytes
{
    int16_t mv[2], available, source;       // source: 0 none, 1 the bottom-right cell, 2 the centre cell
};

// where the two cells of a prediction unit lie in the store (in cells), and whether the rule consults the bottom-right one at all (Mvp.h:141-181): never a cell
// outside the store for a unit inside the picture -- the bottom-right cell is consulted only inside the picture, the centre sample is the unit's own
HAVOC_HD inline bool temporalBottomRightConsulted(int x0, int y0, int w, int h, const TemporalParams &P)
{
    return (y0 >> P.ctbLog2) == ((y0 + h) >> P.ctbLog2) && y0 + h < P.picHeight && x0 + w < P.picWidth;
}
HAVOC_HD inline bool temporalPuInside(int x0, int y0, int w, int h, const TemporalParams &P)
{
    return x0 >= 0 && y0 >= 0 && w > 0 && h > 0 && w <= P.picWidth - x0 && h <= P.picHeight - y0;
}

// one record of havoc_mi355x_temporal_candidates: deriveTemporalCandidate over the two cells as stored, and which of them gave the vector.  bottomRight is read only
// when consulted (hand in any cell otherwise).  A unit that is not inside the picture has no candidate
HAVOC_HD inline TemporalCand temporalCandidateOf(int x0, int y0, int w, int h, const TemporalParams &P, const ColStoreCell &bottomRight, const ColStoreCell &centre, int X)
{
    TemporalCand r = {{0, 0}, 0, 0};
    if (!temporalPuInside(x0, y0, w, h, P)) return r;
    const ColocatedCell br = colocatedCellOf(bottomRight), ce = colocatedCellOf(centre);
    const bool back = P.allBackwards != 0, fromL0 = P.collocatedFromL0 != 0;
    const int target = X ? P.targetPoc[1] : P.targetPoc[0];
    Mv v, unused;
    const bool available = deriveTemporalCandidate(x0, y0, w, h, P.picWidth, P.picHeight, P.ctbLog2, br, ce, X, P.colPoc, P.curPoc, target, back, fromL0, &v);
    const bool fromBr = temporalBottomRightConsulted(x0, y0, w, h, P) && colocatedVector(br, X, P.colPoc, P.curPoc, target, back, fromL0, &unused);
    r.mv[0] = available ? v.x : int16_t(0);
    r.mv[1] = available ? v.y : int16_t(0);
    r.available = available ? 1 : 0;
    r.source = int16_t(available ? (fromBr ? 1 : 2) : 0);
    return r;
}

// nb[0..4] = A0 (below-left), A1 (left), B0 (above-right), B1 (above), B2 (above-left); X = the list being predicted, curPoc / targetPoc = the picture order counts of
// the current picture and of RefPicList(X)[refIdxLX]; every reference picture is a short-term one (the reference encoder uses no long-term pictures);
// colAvailable / col = the temporal candidate (Mvp.h:141-181), consulted only where the rule consults it.  out[0..1] = mvpListLX[0..1].
HAVOC_HD inline void deriveAmvp(int X, int curPoc, int targetPoc, const AmvpNeighbour nb[5], bool colAvailable, Mv col, Mv out[2])
{
    const int Y = 1 - X;
    bool availableA = false, availableB = false;
    Mv mvA, mvB;
    const bool isScaled = nb[0].available || nb[1].available;
    // (every loop has a constant trip count and is unrolled on the device: the five records then live in registers -- indexed, they went to scratch memory and cost the
    // walk 2.6 ms per 1080p picture)
    // A: the first of A0, A1 with a vector into the target picture (own list first) ...
    HAVOC_UNROLL
    for (int k = 0; k < 2; ++k)
        if (!availableA && nb[k].available)
        {
            if (nb[k].predFlag[X] && nb[k].refPoc[X] == targetPoc) { availableA = true; mvA = nb[k].mv[X]; }
            else if (nb[k].predFlag[Y] && nb[k].refPoc[Y] == targetPoc) { availableA = true; mvA = nb[k].mv[Y]; }
        }
    // ... else the first with any vector, scaled to the target picture's distance (step 7)
    HAVOC_UNROLL
    for (int k = 0; k < 2; ++k)
        if (!availableA && nb[k].available)
        {
            int poc = 0;
            if (nb[k].predFlag[X]) { availableA = true; mvA = nb[k].mv[X]; poc = nb[k].refPoc[X]; }
            else if (nb[k].predFlag[Y]) { availableA = true; mvA = nb[k].mv[Y]; poc = nb[k].refPoc[Y]; }
            if (availableA && poc != targetPoc) mvA = amvpDistScale(mvA, curPoc - poc, curPoc - targetPoc);
        }
    // B: the first of B0, B1, B2 with a vector into the target picture
    HAVOC_UNROLL
    for (int k = 2; k < 5; ++k)
        if (!availableB && nb[k].available)
        {
            if (nb[k].predFlag[X] && nb[k].refPoc[X] == targetPoc) { availableB = true; mvB = nb[k].mv[X]; }
            else if (nb[k].predFlag[Y] && nb[k].refPoc[Y] == targetPoc) { availableB = true; mvB = nb[k].mv[Y]; }
        }
    // steps 4 / 5: with neither A0 nor A1 there, B's unscaled candidate becomes A and B is looked for again, this time allowing a scaled one
    if (!isScaled && availableB)
    {
        availableA = true;
        mvA = mvB;
    }
    if (!isScaled)
    {
        availableB = false;
        HAVOC_UNROLL
        for (int k = 2; k < 5; ++k)
            if (!availableB && nb[k].available)
            {
                int poc = 0;
                if (nb[k].predFlag[X]) { availableB = true; mvB = nb[k].mv[X]; poc = nb[k].refPoc[X]; }
                else if (nb[k].predFlag[Y]) { availableB = true; mvB = nb[k].mv[Y]; poc = nb[k].refPoc[Y]; }
                if (availableB && poc != targetPoc) mvB = amvpDistScale(mvB, curPoc - poc, curPoc - targetPoc);
            }
    }
    // the temporal candidate only when A and B do not already give two different predictors
    const bool useCol = !(availableA && availableB && mvA != mvB) && colAvailable;
    // mvpListLX: A, then B unless it repeats A, then the temporal candidate, zero-filled to two (the list's third entry is never used)
    Mv first(0, 0), second(0, 0);
    int n = 0;
    if (availableA) { first = mvA; n = 1; }
    if (availableB && !(n == 1 && mvB == first))
    {
        if (n == 0) first = mvB; else second = mvB;
        ++n;
    }
    if (useCol && n < 2)
    {
        if (n == 0) first = col; else second = col;
        ++n;
    }
    out[0] = first;
    out[1] = second;
}

} // namespace havoc_search
