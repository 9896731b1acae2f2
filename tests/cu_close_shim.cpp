// TEST INFRASTRUCTURE ONLY.  The reference's own bits of an inter coding unit as Search<IfCbf<rqt_root_cbf, transform_tree>>::go measures them
// (turing/Search.hpp:2362-2568): Syntax<coding_unit>::go (turing/SyntaxCtu.hpp:143-264) driven over a small stand-in handle whose tag is Measure<void>, so that
// every CU element goes to the reference's own writer -- Write<Element<cu_skip_flag, ae>>, <pred_mode_flag>, <part_mode> (turing/Binarization.h:283-375),
// <rqt_root_cbf> (:524-533), <merge_idx> (:549-582) -- and every bin to Measure<EncodeDecision> / Measure<EncodeBypass> (turing/Write.h:494-567), which is the
// measureEncodeDecision EstimateRate<void> uses too (turing/EstimateRate.h:78-90).  Compiled with oracle/Makefile's TURFLAGS into a temporary directory by
// tests/cu_close_tools.py; nothing of the reference is stored.
//
// The stand-in holds a real ContextsAndCost, coding_quadtree and a real StateCodedData over a scratch buffer: CuPredMode, the cbf word (rqt_root_cbf) and
// word1().merge[0] (merge_flag, merge_idx) are answered from it, rqt_root_cbf, merge_flag and merge_idx by the reference's own Access<> (turing/CodedData.h:722-740).
// The neighbours' cu_skip_flag (the encoder reads them from the snake), PartMode and the parameter-set values are the handle's own.
//
// Stubs: h(prediction_unit) adds the supplied rate of the CU's prediction units once (pinned by tests/pu_rate_shim.cpp) -- for a skipped CU it is the skip branch of
// Syntax<prediction_unit>::go (SyntaxCtu.hpp:270-274): merge_idx when MaxNumMergeCand > 1, through the reference's writer; h(IfCbf<rqt_root_cbf, transform_tree>) adds
// the supplied tree rate when rqt_root_cbf is set (pinned by the transform-tree shim).  The elements the preconditions exclude (cu_transquant_bypass_flag, PCM, the
// intra modes) abort.
//
// cu_close_costs is the close's two cost computations (Search.hpp:2397, 2512-2517) with the reference's Cost and Lambda types.
#include "turing/StateEncode.h"
#include "turing/EstimateRate.h"
#include "turing/Measure.h"
#include "turing/CodedData.h"
#include "turing/SyntaxCtu.hpp"
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace {

template <class Tag, class F> struct Rebind;
template <template <class> class Verb, class F> struct Rebind<Verb<void>, F> { typedef Verb<F> type; };

const int X0 = 64, Y0 = 64;

struct State
{
    ContextsAndCost cc;
    coding_quadtree cqt;
    StateCodedData coded;
    CodedData::Type words[32];
    int skip, left, up, sliceType, minCbLog2, amp, maxNumMergeCand, maxTrafoDepth, puCalls;
    PartModeType partMode;
    int64_t ratePu, rateTree;
    State() : cqt(X0, Y0, 3, 0) {}
};

alignas(64) char nobody[1 << 16];

struct Handle
{
    typedef Measure<void> Tag;
    State *st;

    // ---- the stubs
    void operator()(prediction_unit pu)
    {
        if (st->puCalls++) return;
        if ((*this)[cu_skip_flag(pu.x0, pu.y0)])
        {
            if ((*this)[MaxNumMergeCand()] > 1) (*this)(merge_idx(pu.x0, pu.y0), ae(v));
        }
        else
            st->cc.rate.value += st->ratePu;
    }
    void operator()(IfCbf<rqt_root_cbf, transform_tree> i)
    {
        if ((*this)[i.cbf]) st->cc.rate.value += st->rateTree;
    }
    // ---- excluded by the preconditions
    void operator()(cu_transquant_bypass_flag, ae) { abort(); }
    void operator()(pcm_flag, ae) { abort(); }
    void operator()(pcm_alignment_one_bit, f) { abort(); }
    void operator()(pcm_alignment_zero_bit, f) { abort(); }
    void operator()(pcm_sample) { abort(); }
    void operator()(prev_intra_luma_pred_flag, ae) { abort(); }
    void operator()(mpm_idx, ae) { abort(); }
    void operator()(rem_intra_luma_pred_mode, ae) { abort(); }
    void operator()(intra_chroma_pred_mode, ae) { abort(); }
    // ---- everything else by the tag
    template <class V, class M> void operator()(V v, M m) { Rebind<Tag, Element<V, M>>::type::go(Element<V, M>{ v, m }, *this); }
    template <class F> void operator()(F f) { Rebind<Tag, F>::type::go(f, *this); }

    // ---- values
    int operator[](transquant_bypass_enabled_flag) const { return 0; }
    int operator[](pcm_enabled_flag) const { return 0; }
    int operator[](Log2MinIpcmCbSizeY) const { return 0; }
    int operator[](Log2MaxIpcmCbSizeY) const { return 0; }
    int operator[](byte_aligned) const { return 1; }
    int operator[](ChromaArrayType) const { return 1; }
    int operator[](IntraSplitFlag) const { return 0; }
    int operator[](max_transform_hierarchy_depth_intra) const { return 1; }
    int operator[](max_transform_hierarchy_depth_inter) const { return 1; }
    int operator[](prev_intra_luma_pred_flag) const { return 0; }
    int operator[](Neighbouring<pcm_flag, Current>) const { return 0; }
    int &operator[](MaxTrafoDepth) { return st->maxTrafoDepth; }
    int operator[](slice_type) const { return st->sliceType; }
    int operator[](MinCbLog2SizeY) const { return st->minCbLog2; }
    int operator[](amp_enabled_flag) const { return st->amp; }
    int operator[](MaxNumMergeCand) const { return st->maxNumMergeCand; }
    PartModeType operator[](PartMode) const { return st->partMode; }
    int operator[](cu_skip_flag v) const { return v.x0 < X0 ? st->left : v.y0 < Y0 ? st->up : st->skip; }
    int operator[](Neighbouring<cu_skip_flag, Current>) const { return st->skip; }
    int operator[](Neighbouring<CuPredMode, Current>) { return st->coded.codedCu.word0().CuPredMode; }
    int operator[](rqt_root_cbf v) { return Access<rqt_root_cbf, StateCodedData>::get(v, st->coded); }
    int operator[](merge_flag v) { return Access<merge_flag, StateCodedData>::get(v, st->coded); }
    int operator[](merge_idx v) { return Access<merge_idx, StateCodedData>::get(v, st->coded); }

    // ---- state
    operator coding_quadtree *() { return &st->cqt; }
    operator const coding_quadtree *() { return &st->cqt; }
    operator Contexts *() { return &st->cc; }
    operator StateEstimateRate *() { return &st->cc; }
    operator StateCodedData *() { return &st->coded; }
    template <class T> operator T *() { return reinterpret_cast<T *>(nobody); }
};

template <class Tag> void put(Contexts &c, const uint8_t *s, int n) { for (int i = 0; i < n; ++i) c.get<Tag>(i).state = s[i]; }
template <class Tag> void take(Contexts &c, uint8_t *s, int n) { for (int i = 0; i < n; ++i) s[i] = c.get<Tag>(i).state; }

} // namespace

template <> struct SampleType<Handle> { typedef uint8_t Type; };

// p: int32 [12] = cu_skip_flag, PartMode, log2CbSize, MinCbLog2SizeY, amp_enabled_flag, the left neighbour's cu_skip_flag, the upper neighbour's, merge_flag of the
// first prediction unit, merge_idx, MaxNumMergeCand, rqt_root_cbf, B slice; cu: 16 bytes (HAVOC_CU_SYNTAX_CTX_*), pu: 16 bytes (HAVOC_PU_SYNTAX_CTX_*), both updated in
// place -> the Q16 rate of the coding unit
extern "C" int64_t cu_close_syntax(const int32_t *p, int64_t ratePu, int64_t rateTree, uint8_t *cu, uint8_t *pu)
{
    State *st = new State();
    st->skip = p[0];
    st->partMode = PartModeType(p[1]);
    st->cqt = coding_quadtree(X0, Y0, p[2], 6 - p[2]);
    st->minCbLog2 = p[3];
    st->amp = p[4];
    st->left = p[5];
    st->up = p[6];
    st->maxNumMergeCand = p[9];
    st->sliceType = p[11] ? B : P;
    st->maxTrafoDepth = -1;
    st->puCalls = 0;
    st->ratePu = ratePu;
    st->rateTree = rateTree;
    std::memset(st->words, 0, sizeof(st->words));
    StateCodedData &s = st->coded;
    s.reset(st->words);
    s.codedCu.init();
    s.codedCu.word0().CuPredMode = p[0] ? MODE_SKIP : MODE_INTER;
    s.codedCu.word0().cbfWord = p[10] ? 1 : 0;
    s.partIdx = 0;
    s.codedPu = s.codedCu.firstPredictionUnit();
    s.codedCu.word1().merge[0] = p[7] ? p[8] + 1 : 0;
    Contexts &c = st->cc;
    put<split_cu_flag>(c, cu + 0, 3);
    put<cu_skip_flag>(c, cu + 3, 3);
    put<pred_mode_flag>(c, cu + 6, 1);
    put<part_mode>(c, cu + 7, 4);
    put<rqt_root_cbf>(c, cu + 11, 1);
    put<merge_flag>(c, pu + 0, 1);
    put<merge_idx>(c, pu + 1, 1);
    put<inter_pred_idc>(c, pu + 2, 5);
    put<ref_idx_lX>(c, pu + 7, 2);
    put<abs_mvd_greater0_flag>(c, pu + 9, 1);
    put<abs_mvd_greater1_flag>(c, pu + 10, 1);
    put<mvp_lX_flag>(c, pu + 11, 1);
    st->cc.rate = Cost();
    Handle h{ st };
    Syntax<coding_unit>::go(coding_unit(X0, Y0, p[2]), h);
    const int64_t rate = st->cc.rate.value;
    take<split_cu_flag>(c, cu + 0, 3);
    take<cu_skip_flag>(c, cu + 3, 3);
    take<pred_mode_flag>(c, cu + 6, 1);
    take<part_mode>(c, cu + 7, 4);
    take<rqt_root_cbf>(c, cu + 11, 1);
    take<merge_flag>(c, pu + 0, 1);
    take<merge_idx>(c, pu + 1, 1);
    take<inter_pred_idc>(c, pu + 2, 5);
    take<ref_idx_lX>(c, pu + 7, 2);
    take<abs_mvd_greater0_flag>(c, pu + 9, 1);
    take<abs_mvd_greater1_flag>(c, pu + 10, 1);
    take<mvp_lX_flag>(c, pu + 11, 1);
    delete st;
    return rate;
}

// the two costs of the close: the coded candidate's lambdaDistortion += ssd * reciprocalLambda with ssd = ssd[0] + ssd[1] + ssd[2] (Search.hpp:2384-2397), the
// unit without residual's lambda * ssdPrediction[0..2] one after the other (:2512-2515), cost2() of both and cost2() < cost2() (:2517).
// out: int64 [6] = lambdaDistortion coded, cost coded, lambdaDistortion without, cost without, without < coded, Lambda::value
extern "C" void cu_close_costs(int64_t rateCoded, const int32_t *ssd, int64_t rateWithout, const int32_t *ssdPrediction, double reciprocalLambdaValue, int64_t *out)
{
    Lambda reciprocalLambda;
    reciprocalLambda.set(reciprocalLambdaValue);
    ContextsAndCost coded, without;
    coded.rate.value = rateCoded;
    coded.lambdaDistortion.value = 0;
    auto const sum = ssd[0] + ssd[1] + ssd[2];
    coded.lambdaDistortion += sum * reciprocalLambda;
    without.rate.value = rateWithout;
    without.lambdaDistortion.value = 0;
    Lambda lambda = reciprocalLambda;
    without.lambdaDistortion += lambda * ssdPrediction[0];
    without.lambdaDistortion += lambda * ssdPrediction[1];
    without.lambdaDistortion += lambda * ssdPrediction[2];
    out[0] = coded.lambdaDistortion.value;
    out[1] = coded.cost2().value;
    out[2] = without.lambdaDistortion.value;
    out[3] = without.cost2().value;
    out[4] = without.cost2() < coded.cost2();
    out[5] = reciprocalLambda.value;
}
