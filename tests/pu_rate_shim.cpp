// TEST INFRASTRUCTURE ONLY.  The reference's own rate of one candidate of a prediction unit as measurePuCost measures it (turing/Search.hpp:1656-1706):
// Syntax<prediction_unit>::go (turing/SyntaxCtu.hpp:267-314) driven over a small stand-in handle whose tag is Measure<void>, so that every element goes to the
// reference's own writer -- Write<Element<merge_flag, ae>>, <merge_idx>, <inter_pred_idc> (turing/Binarization.h:538-612), Write<mvd_coding> (turing/Write.h:1505-1527)
// -> Syntax<mvd_coding>::go (SyntaxCtu.hpp:382-405) -> <abs_mvd_greater0_flag>, <abs_mvd_greater1_flag>, <abs_mvd_minus2>, <mvd_sign_flag>, <mvp_l0_flag>, <mvp_l1_flag>
// (Binarization.h:745-831) -- and every bin to Measure<EncodeDecision> / Measure<EncodeBypass> (Write.h:494-567).  Compiled with oracle/Makefile's TURFLAGS into a
// temporary directory by tests/pu_rate_tools.py; nothing of the reference is stored.
//
// The stand-in holds a real ContextsAndCost, prediction_unit, coding_quadtree and a real StateCodedData over a scratch buffer whose codedCu / codedPu words are filled
// the way Search<prediction_unit>::State fills them: searchMergeMode (Search.hpp:1754-1759: word1().merge[partIdx] = i + 1), searchUni (:1770-1794: init, mvp_lX_flag,
// ref_idx_lX, predFlag, mvd; searchMotionUni's result :1651-1652) and searchBi (:1796-1827: word 0 the OR of the two uni words, the L0 vector words, the L1 vector
// words; searchMotionBi's results through mvd(refList) and the metadata).  merge_flag, merge_idx, inter_pred_idc, ref_idx_lX, mvp_lX_flag and Mvd are answered by the
// reference's own Access<> over that data (turing/CodedData.h:732-764, turing/StateEncode.h:1019-1093).  cu_skip_flag (the encoder reads it from the neighbourhood
// snake) and the slice values are the handle's own.
//
// Restated here: ref_idx_l0 / ref_idx_l1.  The reference has NO writer for them: the generic Write<Element<V, ae>> (Binarization.h:52-59) asserts "not yet
// implemented" and, in a release build, writes nothing.  The handle routes the two elements to the inverse of the reference's reader ReadRefIdx (turing/Read.h:1864-1888):
// truncated Rice with cMax = num_ref_idx_lX_active_minus1, bins 0 and 1 EncodeDecision<ref_idx_lX> with ctxInc = binIdx, the rest EncodeBypass.  The syntax reaches them
// only when num_ref_idx_lX_active_minus1 > 0.
//
// pu_rate_cost is measurePuCost's last line with the reference's Cost and Lambda types.
#include "turing/StateEncode.h"
#include "turing/EstimateRate.h"
#include "turing/Measure.h"
#include "turing/CodedData.h"
#include "turing/SyntaxCtu.hpp"
#include <cstdint>
#include <cstring>

namespace {

template <class Tag, class F> struct Rebind;
template <template <class> class Verb, class F> struct Rebind<Verb<void>, F> { typedef Verb<F> type; };

struct State
{
    ContextsAndCost cc;
    coding_quadtree cqt;
    prediction_unit pu;
    StateCodedData coded;
    CodedData::Type words[32];
    int skip, sliceType, maxNumMergeCand, mvdL1Zero, numRefIdx[2];
    int greater0[2], greater1[2], minus2[2], sign[2];
    State() : cqt(0, 0, 3, 0), pu(0, 0, 8, 8) {}
};

// never read: the places the reference's writers take a pointer to state they use only under other tags
alignas(64) char nobody[1 << 16];

struct Handle
{
    typedef Measure<void> Tag;
    State *st;

    // ---- ref_idx_lX: the inverse of ReadRefIdx (see the header)
    template <class V> void refIdx(int cMax, int synVal)
    {
        for (int binIdx = 0; binIdx < synVal + (synVal < cMax ? 1 : 0); ++binIdx)
        {
            const int binVal = binIdx < synVal ? 1 : 0;
            if (binIdx < 2) (*this)(EncodeDecision<V>(binVal, binIdx));
            else (*this)(EncodeBypass<V>(binVal));
        }
    }
    void operator()(ref_idx_l0 v, ae) { refIdx<ref_idx_l0>(st->numRefIdx[0], (*this)[v]); }
    void operator()(ref_idx_l1 v, ae) { refIdx<ref_idx_l1>(st->numRefIdx[1], (*this)[v]); }
    // ---- everything else by the tag
    template <class V, class M> void operator()(V v, M m) { Rebind<Tag, Element<V, M>>::type::go(Element<V, M>{ v, m }, *this); }
    template <class F> void operator()(F f) { Rebind<Tag, F>::type::go(f, *this); }

    // ---- values
    int operator[](cu_skip_flag) const { return st->skip; }
    int operator[](MaxNumMergeCand) const { return st->maxNumMergeCand; }
    int operator[](slice_type) const { return st->sliceType; }
    int operator[](mvd_l1_zero_flag) const { return st->mvdL1Zero; }
    int operator[](num_ref_idx_l0_active_minus1) const { return st->numRefIdx[0]; }
    int operator[](num_ref_idx_l1_active_minus1) const { return st->numRefIdx[1]; }
    int operator[](merge_flag v) { return Access<merge_flag, StateCodedData>::get(v, st->coded); }
    int operator[](merge_idx v) { return Access<merge_idx, StateCodedData>::get(v, st->coded); }
    int operator[](inter_pred_idc v) { return Access<inter_pred_idc, StateCodedData>::get(v, st->coded); }
    int operator[](ref_idx_l0 v) { return Access<ref_idx_l0, StateCodedData>::get(v, st->coded); }
    int operator[](ref_idx_l1 v) { return Access<ref_idx_l1, StateCodedData>::get(v, st->coded); }
    int operator[](mvp_l0_flag v) { return Access<mvp_l0_flag, StateCodedData>::get(v, st->coded); }
    int operator[](mvp_l1_flag v) { return Access<mvp_l1_flag, StateCodedData>::get(v, st->coded); }
    MotionVector &operator[](Mvd v) { return Access<Mvd, StateCodedData>::get(v, st->coded); }
    int &operator[](abs_mvd_greater0_flag v) { return st->greater0[v.compIdx]; }
    int &operator[](abs_mvd_greater1_flag v) { return st->greater1[v.compIdx]; }
    int &operator[](abs_mvd_minus2 v) { return st->minus2[v.compIdx]; }
    int &operator[](mvd_sign_flag v) { return st->sign[v.compIdx]; }

    // ---- state
    operator prediction_unit *() { return &st->pu; }
    operator coding_quadtree *() { return &st->cqt; }
    operator Contexts *() { return &st->cc; }
    operator StateEstimateRate *() { return &st->cc; }
    operator StateCodedData *() { return &st->coded; }
    template <class T> operator T *() { return reinterpret_cast<T *>(nobody); }
};

template <class Tag> void put(Contexts &c, const uint8_t *s, int n) { for (int i = 0; i < n; ++i) c.get<Tag>(i).state = s[i]; }
template <class Tag> void take(Contexts &c, uint8_t *s, int n) { for (int i = 0; i < n; ++i) s[i] = c.get<Tag>(i).state; }

// searchUni's words for one list: word 0 (the metadata), the vector difference
void uniWords(CodedData::Type *p, int refList, int refIdx, const int16_t *mvd, int mvpFlag)
{
    CodedData::PredictionUnit pu{ p };
    pu.init();
    pu.word0().metadata[refList].mvp_lX_flag = 0;
    pu.word0().metadata[refList].ref_idx_lX = refIdx;
    pu.word0().metadata[refList].predFlag = 1;
    pu.mvd(refList) = MotionVector{ 0, 0 };
    MotionVector best;
    best[0] = mvd[0];
    best[1] = mvd[1];
    pu.mvd(refList) = best;                                           // Search.hpp:1651
    pu.word0().metadata[refList].mvp_lX_flag = mvpFlag;               // :1652
}

} // namespace

template <> struct SampleType<Handle> { typedef uint8_t Type; };

// p: int32 [16] = skip, merge, merge_idx, pred (0 L0, 1 L1, 2 BI), mvd[2][2], mvp_flag[2], ref_idx[2], nPbW, nPbH, cqtDepth, unused; slice: int32 [5] = B slice,
// MaxNumMergeCand, mvd_l1_zero_flag, num_ref_idx_l0_active_minus1, num_ref_idx_l1_active_minus1; syntax: 16 bytes (HAVOC_PU_SYNTAX_CTX_*), updated in place -> the Q16 rate
extern "C" int64_t pu_rate_candidate(const int32_t *p, const int32_t *slice, uint8_t *syntax)
{
    State *st = new State();
    const int skip = p[0], merged = p[1] || skip, mergeIdx = p[2], pred = p[3];
    const int16_t mvd[2][2] = { { int16_t(p[4]), int16_t(p[5]) }, { int16_t(p[6]), int16_t(p[7]) } };
    st->skip = skip;
    st->sliceType = slice[0] ? B : P;
    st->maxNumMergeCand = slice[1];
    st->mvdL1Zero = slice[2];
    st->numRefIdx[0] = slice[3];
    st->numRefIdx[1] = slice[4];
    st->pu = prediction_unit(0, 0, p[12], p[13]);
    st->cqt = coding_quadtree(0, 0, 6 - p[14], p[14]);
    std::memset(st->words, 0, sizeof(st->words));
    StateCodedData &s = st->coded;
    s.reset(st->words);
    s.codedCu.init();
    s.codedCu.word0().CuPredMode = skip ? MODE_SKIP : MODE_INTER;
    s.partIdx = 0;
    s.codedPu = s.codedCu.firstPredictionUnit();
    if (merged)
        s.codedCu.word1().merge[s.partIdx] = mergeIdx + 1;            // searchMergeMode
    else
    {
        s.codedCu.word1().merge[s.partIdx] = 0;
        if (pred != 2)
            uniWords(s.codedPu.p, pred, p[10 + pred], mvd[pred], p[8 + pred]);      // searchUni
        else
        {   // searchBi over the two searchUni champions, then searchMotionBi's results
            CodedData::Type uni[2][3];
            for (int l = 0; l < 2; ++l) uniWords(uni[l], l, p[10 + l], mvd[l], p[8 + l]);
            s.codedPu.p[0] = uni[0][0] | uni[1][0];
            s.codedPu.p[1] = uni[0][1];
            s.codedPu.p[2] = uni[0][2];
            s.codedPu.p[3] = uni[1][1];
            s.codedPu.p[4] = uni[1][2];
            for (int l = 0; l < 2; ++l)
            {
                MotionVector best;
                best[0] = mvd[l][0];
                best[1] = mvd[l][1];
                s.codedPu.mvd(l) = best;
                s.codedPu.word0().metadata[l].mvp_lX_flag = p[8 + l];
            }
        }
    }
    Contexts &c = st->cc;
    put<merge_flag>(c, syntax + 0, 1);
    put<merge_idx>(c, syntax + 1, 1);
    put<inter_pred_idc>(c, syntax + 2, 5);
    put<ref_idx_lX>(c, syntax + 7, 2);
    put<abs_mvd_greater0_flag>(c, syntax + 9, 1);
    put<abs_mvd_greater1_flag>(c, syntax + 10, 1);
    put<mvp_lX_flag>(c, syntax + 11, 1);
    st->cc.rate = Cost();
    Handle h{ st };
    Syntax<prediction_unit>::go(st->pu, h);
    const int64_t rate = st->cc.rate.value;
    take<merge_flag>(c, syntax + 0, 1);
    take<merge_idx>(c, syntax + 1, 1);
    take<inter_pred_idc>(c, syntax + 2, 5);
    take<ref_idx_lX>(c, syntax + 7, 2);
    take<abs_mvd_greater0_flag>(c, syntax + 9, 1);
    take<abs_mvd_greater1_flag>(c, syntax + 10, 1);
    take<mvp_lX_flag>(c, syntax + 11, 1);
    delete st;
    return rate;
}

// measurePuCost's `rate + (satd[0] + satd[1] + satd[2]) * lambda` (Search.hpp:1691-1705) with lambda.set(reciprocalSqrtLambda); *lambdaQ16 = the Lambda's value
extern "C" int64_t pu_rate_cost(int64_t rate, int32_t satdY, int32_t satdCb, int32_t satdCr, double reciprocalSqrtLambda, int32_t *lambdaQ16)
{
    Cost r;
    r.value = rate;
    Lambda lambda;
    lambda.set(reciprocalSqrtLambda);
    *lambdaQ16 = lambda.value;
    int32_t satd[3] = { satdY, satdCb, satdCr };
    const Cost cost = r + (satd[0] + satd[1] + satd[2]) * lambda;
    return cost.value;
}
