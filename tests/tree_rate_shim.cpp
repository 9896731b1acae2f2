// TEST INFRASTRUCTURE ONLY.  The reference's own rate of an inter coding unit's whole transform tree at one depth, as the inter transform-tree decision measures it
// (turing/Reconstruct.cpp:1296-1428: `if (m[rqt_root_cbf()]) m(tt)` under EstimateRate<void>): Syntax<transform_tree>::go (turing/SyntaxCtu.hpp:329-379) ->
// Syntax<transform_unit>::go (:411-502), driven over a small stand-in handle whose tag is EstimateRate<void>, so that every element goes to the reference's own
// writer -- Write<Element<split_transform_flag, ae>>, <cbf_cb>, <cbf_cr>, <cbf_luma> (turing/Binarization.h:617-666), bins to EstimateRate<EncodeDecision> /
// <EncodeBypass> -- and every residual_coding to EncodeResidual::inner.  Compiled with oracle/Makefile's TURFLAGS into a temporary directory by
// tests/tree_rate_tools.py; nothing of the reference is stored.
//
// The stand-in holds a real ContextsAndCost and a real StateCodedData over a scratch buffer that is FILLED by the reference's own CodedData functions in the order
// ReconstructInter<transform_tree> / <transform_unit> fill it (Reconstruct.cpp:57-116, 1040-1125): TransformTree::init, split_transform_flag, storeResidual per
// component (which sets the cbf bits of the transform tree's word and packs the levels), the children's cbfWord ORed into the parent's (:90-94); for an 8x8 unit at
// depth 1 the 4x4 chroma blocks are stored behind child 3's luma with child 3's word.  Every cbf the syntax asks about is answered by AccessCbf over that data
// (turing/CodedData.h:662-718), as the encoder's handle answers it.
//
// Restated here (the reference routes them through Write<F>, which wants the encoder's whole state -- the neighbourhood snake and its cursor, the loop filter):
//   Write<transform_tree>::go  (turing/Write.h:1167-1255), its MODE_INTER part: where stateCodedData->transformTree points at each depth and block, the ancestry,
//                              h[split_transform_flag()] from the word, the call of Syntax<transform_tree>::go; the handle keeps the current transform_tree;
//   Write<transform_unit>::go  (turing/Write.h:1258-1279): Syntax<transform_unit>::go, then the two pointers moved behind the unit's residuals;
//   Write<IfCbf<V, residual_coding>>::go (turing/Write.h:1405-1450): the residual pointer, `if (h[e.cbf]) EncodeResidual::encode(h)` as EncodeResidual::inner<false,
//                              is4x4> (encode() picks inner by the CPU's popcnt; the two agree), the pointers after Cr.  Every call is recorded: x0, y0, log2, cIdx, cbf.
#include "turing/StateEncode.h"
#include "turing/EstimateRate.h"
#include "turing/EncodeResidual.hpp"
#include "turing/CodedData.h"
#include "turing/SyntaxCtu.hpp"
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

template <class Tag, class F> struct Rebind;
template <template <class> class Verb, class F> struct Rebind<Verb<void>, F> { typedef Verb<F> type; };

struct State
{
    ContextsAndCost cc;
    coding_quadtree cqt;
    transform_tree tt;
    residual_coding rc;
    StateCodedData coded;
    std::vector<CodedData::Type> words;
    int sdh, minTb, maxTb, maxTrafoDepth, splitTransformFlag;
    int lastX[2], lastY[2];
    int32_t *calls;
    State() : cqt(0, 0, 3, 0), tt(0, 0, 0, 0, 3, 0, 0), rc(0, 0, 2, 0) {}
};

// never read: the places the reference's writers take a pointer to state they use only under other tags (StateEncode, StateEncodeSubstreamBase, ...)
alignas(64) char nobody[1 << 16];

struct Handle
{
    typedef EstimateRate<void> Tag;
    State *st;

    // ---- syntax functions: the three the handle routes itself, the rest by the tag
    void operator()(transform_tree f)
    {   // Write<transform_tree>::go, restated for MODE_INTER (see the header)
        StateCodedData &s = st->coded;
        st->tt = f;
        if (f.trafoDepth == 0)
            s.transformTree = { s.codedPu.p };
        else if (f.blkIdx == 0)
            ++s.transformTree.p;      // (have just split)
        s.transformTreeChroma = s.transformTree;
        s.transformTree.check(f.trafoDepth, f.blkIdx);
        s.transformTreeAncestry[f.trafoDepth] = s.transformTree;
        st->splitTransformFlag = s.transformTree.word0().split_transform_flag || s.transformTree.word0().trafoDepth > f.trafoDepth;
        Syntax<transform_tree>::go(f, *this);
    }
    void operator()(transform_unit f)
    {   // Write<transform_unit>::go, restated
        Syntax<transform_unit>::go(f, *this);
        st->coded.transformTree.p = st->coded.residual.p;
        st->coded.transformTreeChroma.p = st->coded.residual.p;
    }
    template <class V> void operator()(IfCbf<V, residual_coding> e)
    {   // Write<IfCbf<V, residual_coding>>::go, restated
        StateCodedData &s = st->coded;
        const residual_coding rc = e.f;
        if (rc.cIdx == 0) s.residual = s.transformTree.firstResidual();
        const int cbf = (*this)[e.cbf];
        int32_t *c = st->calls + 1 + 5 * st->calls[0]++;
        c[0] = rc.x0; c[1] = rc.y0; c[2] = rc.log2TrafoSize; c[3] = rc.cIdx; c[4] = cbf;
        if (cbf)
        {
            st->rc = rc;
            if (rc.log2TrafoSize == 2) EncodeResidual::inner<false, true>(*this);
            else EncodeResidual::inner<false, false>(*this);
        }
        if (rc.cIdx == 2)
        {
            s.transformTree.p = s.residual.p;
            s.transformTreeChroma.p = s.residual.p;
        }
        s.codedDataAfter = s.residual.p;
    }
    template <class V, class M> void operator()(V v, M m) { Rebind<Tag, Element<V, M>>::type::go(Element<V, M>{ v, m }, *this); }
    template <class F> void operator()(F f) { Rebind<Tag, F>::type::go(f, *this); }

    // ---- values
    int operator[](MaxTrafoDepth) const { return st->maxTrafoDepth; }
    int operator[](IntraSplitFlag) const { return 0; }
    int operator[](MinTbLog2SizeY) const { return st->minTb; }
    int operator[](MaxTbLog2SizeY) const { return st->maxTb; }
    int operator[](ChromaArrayType) const { return 1; }
    int &operator[](split_transform_flag) { return st->splitTransformFlag; }
    int operator[](cbf_luma v) const { return AccessCbf<cbf_luma, 0>::get(v, st->coded); }
    int operator[](cbf_cb v) const { return AccessCbf<cbf_cb, 1>::get(v, st->coded); }
    int operator[](cbf_cr v) const { return AccessCbf<cbf_cr, 2>::get(v, st->coded); }
    int operator[](Neighbouring<CuPredMode, Current>) const { return MODE_INTER; }
    int operator[](CuPredMode) const { return MODE_INTER; }
    int operator[](scanIdx) const { return 0; }
    int operator[](sign_data_hiding_enabled_flag) const { return st->sdh; }
    int operator[](Log2MaxTransformSkipSize) const { return 2; }
    int &operator[](last_sig_coeff_x_prefix) { return st->lastX[0]; }
    int &operator[](last_sig_coeff_x_suffix) { return st->lastX[1]; }
    int &operator[](last_sig_coeff_y_prefix) { return st->lastY[0]; }
    int &operator[](last_sig_coeff_y_suffix) { return st->lastY[1]; }
    // everything else the syntax asks about is off or absent: cu_qp_delta_enabled_flag, cu_chroma_qp_offset_enabled_flag, cross_component_prediction_enabled_flag,
    // transform_skip_enabled_flag, transform_skip_flag, cu_transquant_bypass_flag, ...
    template <class V> int operator[](V) const { return 0; }

    // ---- state
    operator residual_coding *() { return &st->rc; }
    operator transform_tree *() { return &st->tt; }
    operator transform_tree const *() { return &st->tt; }
    operator coding_quadtree *() { return &st->cqt; }
    operator coding_quadtree const *() { return &st->cqt; }
    operator Contexts *() { return &st->cc; }
    operator StateEstimateRate *() { return &st->cc; }
    operator StateCodedData *() { return &st->coded; }
    template <class T> operator T *() { return reinterpret_cast<T *>(nobody); }
};

template <class Tag> void put(Contexts &c, const uint8_t *s, int n) { for (int i = 0; i < n; ++i) c.get<Tag>(i).state = s[i]; }
template <class Tag> void take(Contexts &c, uint8_t *s, int n) { for (int i = 0; i < n; ++i) s[i] = c.get<Tag>(i).state; }

// CodedData::storeResidual of one block of levels with the transform tree's word `tt`: cbf = the block has a level
void store(CodedData::CodingUnit cu, CodedData::Residual &residual, const int16_t *levels, int log2, CodedData::TransformTree tt, int cIdx)
{
    std::vector<int16_t> block(levels, levels + (1 << 2 * log2));
    bool cbf = false;
    for (int16_t v : block) cbf |= v != 0;
    if (cbf) residual.transformSkipFlag() = 0;
    CodedData::storeResidual(cu, residual, block.data(), log2, 0, cbf, tt, cIdx);
}

} // namespace

template <> struct SampleType<Handle> { typedef uint8_t Type; };

// luma: depth 0 the unit's n x n levels (raster); depth 1 four (n/2)^2 blocks one after the other in z-order.  cb, cr: depth 0 or n == 8 one block of c x c, c = max(n/2, 4);
// depth 1 and n > 8 four (n/4)^2 blocks in z-order.  maxTrafoDepth, minTb, maxTb: MaxTrafoDepth, MinTbLog2SizeY, MaxTbLog2SizeY as the syntax sees them.  states: 128
// bytes (HAVOC_RDOQ_CTX_*), syntax: 4 bytes (HAVOC_INTRA_SYNTAX_CTX_*), both updated in place -> the Q16 rate.  mask: the cbf bits of the transform trees' words as
// storeResidual left them: bit k luma block k, bit 4 + k Cb, bit 8 + k Cr (an 8x8 unit's chroma at depth 1: k = 0).  calls[0]: how many IfCbf<., residual_coding> the syntax
// reached, then x0, y0, log2TrafoSize, cIdx, cbf of each in order (at most 12)
extern "C" int64_t tree_rate_tree(const int16_t *luma, const int16_t *cb, const int16_t *cr, int log2Cb, int depth, int maxTrafoDepth, int minTb, int maxTb, int sdh,
                                  uint8_t *states, uint8_t *syntax, uint32_t *mask, int32_t *calls)
{
    State *st = new State();
    st->sdh = sdh;
    st->minTb = minTb;
    st->maxTb = maxTb;
    st->maxTrafoDepth = maxTrafoDepth;
    st->splitTransformFlag = -1;
    st->calls = calls;
    calls[0] = 0;
    st->cqt = coding_quadtree(0, 0, log2Cb, 0);
    st->words.assign(8 * (1 << 2 * log2Cb) + 256, 0);
    StateCodedData &s = st->coded;
    s.reset(st->words.data());
    s.codedCu.init();
    s.codedCu.word0().CuPredMode = MODE_INTER;
    s.codedPu.p = st->words.data() + 8;
    *mask = 0;
    // ---- the coded data, in ReconstructInter's order
    if (depth == 0)
    {
        const int lc = log2Cb > 3 ? log2Cb - 1 : 2;
        CodedData::TransformTree tt{ s.codedPu.p };
        tt.init(0, 0);
        tt.word0().split_transform_flag = 0;
        CodedData::Residual residual = tt.firstResidual();
        store(s.codedCu, residual, luma, log2Cb, tt, 0);
        store(s.codedCu, residual, cb, lc, tt, 1);
        store(s.codedCu, residual, cr, lc, tt, 2);
        *mask = (uint32_t)tt.word0().cbf[0] | (uint32_t)tt.word0().cbf[1] << 4 | (uint32_t)tt.word0().cbf[2] << 8;
    }
    else
    {
        const int ly = log2Cb - 1, lc = log2Cb > 3 ? log2Cb - 2 : 2;
        CodedData::TransformTree parent{ s.codedPu.p };
        parent.init(0, 0);
        parent.word0().split_transform_flag = 1;
        CodedData::Type *q = parent.p + 1;
        for (int k = 0; k < 4; ++k)
        {
            CodedData::TransformTree tt{ q };
            tt.init(1, k);
            tt.word0().split_transform_flag = 0;
            CodedData::Residual residual = tt.firstResidual();
            store(s.codedCu, residual, luma + (k << 2 * ly), ly, tt, 0);
            if (log2Cb > 3)
            {
                store(s.codedCu, residual, cb + (k << 2 * lc), lc, tt, 1);
                store(s.codedCu, residual, cr + (k << 2 * lc), lc, tt, 2);
                *mask |= (uint32_t)tt.word0().cbf[1] << (4 + k) | (uint32_t)tt.word0().cbf[2] << (8 + k);
            }
            else if (k == 3)
            {
                store(s.codedCu, residual, cb, lc, tt, 1);
                store(s.codedCu, residual, cr, lc, tt, 2);
                *mask |= (uint32_t)tt.word0().cbf[1] << 4 | (uint32_t)tt.word0().cbf[2] << 8;
            }
            *mask |= (uint32_t)tt.word0().cbf[0] << k;
            parent.word0().cbfWord = parent.word0().cbfWord | tt.word0().cbfWord;      // Reconstruct.cpp:90-94
            q = residual.p;
        }
    }
    Contexts &c = st->cc;
    put<cbf_luma>(c, states + 1, 2);
    put<cbf_cX>(c, states + 3, 4);
    put<last_sig_coeff_x_prefix>(c, states + 8, 18);
    put<last_sig_coeff_y_prefix>(c, states + 26, 18);
    put<coded_sub_block_flag>(c, states + 44, 4);
    put<sig_coeff_flag>(c, states + 48, 44);
    put<coeff_abs_level_greater1_flag>(c, states + 92, 24);
    put<coeff_abs_level_greater2_flag>(c, states + 116, 6);
    put<split_transform_flag>(c, syntax + 1, 3);
    st->cc.rate = Cost();
    Handle h{ st };
    // Reconstruct.cpp:1346, 1391: `if (m[rqt_root_cbf()]) m(tt)`; Access<rqt_root_cbf> (CodedData.h:721-729) for an inter unit
    if (s.codedCu.word0().cbfWord) h(transform_tree(0, 0, 0, 0, log2Cb, 0, 0));
    const int64_t rate = st->cc.rate.value;
    take<cbf_luma>(c, states + 1, 2);
    take<cbf_cX>(c, states + 3, 4);
    take<last_sig_coeff_x_prefix>(c, states + 8, 18);
    take<last_sig_coeff_y_prefix>(c, states + 26, 18);
    take<coded_sub_block_flag>(c, states + 44, 4);
    take<sig_coeff_flag>(c, states + 48, 44);
    take<coeff_abs_level_greater1_flag>(c, states + 92, 24);
    take<coeff_abs_level_greater2_flag>(c, states + 116, 6);
    take<split_transform_flag>(c, syntax + 1, 3);
    delete st;
    return rate;
}
