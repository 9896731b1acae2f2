// TEST INFRASTRUCTURE ONLY.  The reference's own rate of one refined intra candidate "since the partition began": Syntax<IntraPartition>::go
// (turing/SyntaxCtu.hpp:704-722) -> Syntax<IntraPartitionPrediction>::go (:686-701) and Syntax<transform_tree>::go (:329-379) -> Syntax<transform_unit>::go (:411-502),
// driven over a small stand-in handle whose tag is EstimateRateLuma<void>, so that every element goes to the reference's own writer: Write<Element<
// prev_intra_luma_pred_flag, ae>>, <mpm_idx>, <rem_intra_luma_pred_mode>, <split_transform_flag>, <cbf_luma> (turing/Binarization.h:395-502, 617-651), cbf_cb / cbf_cr
// and the chroma residuals to Null (turing/EstimateRate.h:114-119), bins to EstimateRate<EncodeDecision> / <EncodeBypass>.  Compiled with oracle/Makefile's TURFLAGS into a
// temporary directory by tests/intra_rate_tools.py; nothing of the reference is stored.
//
// Restated here (the handle routes them itself; the reference routes them through Write<F>, which wants the encoder's whole state -- the neighbourhood snake and its
// cursor, the picture's loop filter):
//   Write<transform_tree>::go  (turing/Write.h:1167-1255): of it only `stateCodedData->transformTree = codedCu.firstTransformTree()`, `h[split_transform_flag()] = split`
//                              and the call of Syntax<transform_tree>::go; the handle also keeps the current transform_tree, as CopyValueToState does;
//   Write<transform_unit>::go  (turing/Write.h:1258-1279): the call of Syntax<transform_unit>::go;
//   Write<IfCbf<cbf_luma, residual_coding>>::go (turing/Write.h:1405-1450): `if (h[e.cbf]) EncodeResidual::encode(h)` as CodedData::storeResidual +
//                              EncodeResidual::inner<false, is4x4>, the way tests/residual_rate_shim.cpp does it (encode() picks inner by the CPU's popcnt; the two
//                              agree), over the same state with the tag changed to EstimateRate<void> as EncodeResidual::encode changes it (turing/EncodeResidual.h:39-45).
// The stand-in holds a real ContextsAndCost, CandModeList, coding_quadtree, transform_tree and StateCodedData over a scratch buffer whose coding-unit words carry
// CuPredMode = MODE_INTRA, part_mode and IntraPredModeY, and whose transform-tree word is zero (split_transform_flag = 0: a candidate is one transform block).
#include "turing/StateEncode.h"
#include "turing/EstimateRate.h"
#include "turing/EncodeResidual.hpp"
#include "turing/CodedData.h"
#include "turing/SyntaxCtu.hpp"
#include "turing/CandModeList.h"
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

template <class Tag, class F> struct Rebind;
template <template <class> class Verb, class F> struct Rebind<Verb<void>, F> { typedef Verb<F> type; };

struct State
{
    ContextsAndCost cc;
    CandModeList cand;
    coding_quadtree cqt;
    transform_tree tt;
    residual_coding rc;
    StateCodedData coded;
    std::vector<CodedData::Type> cuWords, residualWords;
    int16_t *levels;
    int scan, sdh, split, depthIntra, minTb, maxTb;
    int maxTrafoDepth, splitTransformFlag, prevFlag, mpmIdx, rem, cbf;
    int lastX[2], lastY[2];
    State() : cqt(0, 0, 3, 0), tt(0, 0, 0, 0, 3, 0, 0), rc(0, 0, 2, 0) {}
};

// never read: the places the reference's writers take a pointer to state they use only under other tags (Neighbourhood, StateEncode, QpState, ...)
alignas(64) char nobody[1 << 16];

template <class TagT>
struct HandleT
{
    typedef TagT Tag;
    State *st;

    // ---- syntax functions: the three the handle routes itself, the rest by the tag
    void operator()(IntraPartitionPrediction f) { Syntax<IntraPartitionPrediction>::go(f, *this); }
    void operator()(transform_tree f)
    {   // Write<transform_tree>::go, restated (see the header)
        st->tt = f;
        st->coded.transformTree = st->coded.codedCu.firstTransformTree();
        st->coded.transformTreeAncestry[f.trafoDepth] = st->coded.transformTree;
        st->splitTransformFlag = st->coded.transformTree.word0().split_transform_flag;
        Syntax<transform_tree>::go(f, *this);
    }
    void operator()(transform_unit f) { Syntax<transform_unit>::go(f, *this); }
    void operator()(IfCbf<cbf_luma, residual_coding> f)
    {   // Write<IfCbf<cbf_luma, residual_coding>>::go, restated
        if (!st->cbf) return;
        st->rc = f.f;
        const int log2 = f.f.log2TrafoSize;
        std::fill(st->residualWords.begin(), st->residualWords.end(), 0);
        CodedData::Type scratch[16] = {0};
        CodedData::Residual residual;
        residual.p = st->residualWords.data();
        CodedData::CodingUnit cu;
        cu.p = scratch;
        CodedData::TransformTree tt;
        tt.p = scratch + 8;
        CodedData::storeResidual(cu, residual, st->levels, log2, st->scan, true, tt, 0);
        st->coded.residual.p = st->residualWords.data();
        HandleT<EstimateRate<void>> hh{ st };      // EncodeResidual::encode: `auto hh = h.template change<EstimateRate<void>>()` for every tag but Write<void>
        if (log2 == 2) EncodeResidual::inner<false, true>(hh);
        else EncodeResidual::inner<false, false>(hh);
    }
    void operator()(IfCbf<cbf_cb, residual_coding> f) { Rebind<Tag, IfCbf<cbf_cb, residual_coding>>::type::go(f, *this); }      // Null
    void operator()(IfCbf<cbf_cr, residual_coding> f) { Rebind<Tag, IfCbf<cbf_cr, residual_coding>>::type::go(f, *this); }      // Null
    template <class V, class M> void operator()(V v, M m) { Rebind<Tag, Element<V, M>>::type::go(Element<V, M>{ v, m }, *this); }
    template <class F> void operator()(F f) { Rebind<Tag, F>::type::go(f, *this); }

    // ---- values
    int &operator[](MaxTrafoDepth) { return st->maxTrafoDepth; }
    int operator[](IntraSplitFlag) const { return st->split; }
    int operator[](max_transform_hierarchy_depth_intra) const { return st->depthIntra; }
    int operator[](MinTbLog2SizeY) const { return st->minTb; }
    int operator[](MaxTbLog2SizeY) const { return st->maxTb; }
    int operator[](ChromaArrayType) const { return 1; }
    int &operator[](split_transform_flag) { return st->splitTransformFlag; }
    int &operator[](prev_intra_luma_pred_flag) { return st->prevFlag; }
    int &operator[](mpm_idx) { return st->mpmIdx; }
    int &operator[](rem_intra_luma_pred_mode) { return st->rem; }
    int operator[](cbf_luma) const { return st->cbf; }
    int operator[](Neighbouring<CuPredMode, Current>) const { return MODE_INTRA; }
    int operator[](CuPredMode) const { return MODE_INTRA; }
    int operator[](scanIdx) const { return st->scan; }
    int operator[](sign_data_hiding_enabled_flag) const { return st->sdh; }
    int operator[](Log2MaxTransformSkipSize) const { return 2; }
    int &operator[](last_sig_coeff_x_prefix) { return st->lastX[0]; }
    int &operator[](last_sig_coeff_x_suffix) { return st->lastX[1]; }
    int &operator[](last_sig_coeff_y_prefix) { return st->lastY[0]; }
    int &operator[](last_sig_coeff_y_suffix) { return st->lastY[1]; }
    // everything else the syntax asks about is off or absent: cbf_cb, cbf_cr, cu_qp_delta_enabled_flag, cu_chroma_qp_offset_enabled_flag,
    // cross_component_prediction_enabled_flag, transform_skip_enabled_flag, cu_transquant_bypass_flag, ...
    template <class V> int operator[](V) const { return 0; }

    // ---- state
    operator residual_coding *() { return &st->rc; }
    operator transform_tree *() { return &st->tt; }
    operator transform_tree const *() { return &st->tt; }
    operator coding_quadtree *() { return &st->cqt; }
    operator coding_quadtree const *() { return &st->cqt; }
    operator CandModeList *() { return &st->cand; }
    operator Contexts *() { return &st->cc; }
    operator StateEstimateRate *() { return &st->cc; }
    operator StateCodedData *() { return &st->coded; }
    template <class T> operator T *() { return reinterpret_cast<T *>(nobody); }
};

template <class Tag> void put(Contexts &c, const uint8_t *s, int n) { for (int i = 0; i < n; ++i) c.get<Tag>(i).state = s[i]; }
template <class Tag> void take(Contexts &c, uint8_t *s, int n) { for (int i = 0; i < n; ++i) s[i] = c.get<Tag>(i).state; }

typedef HandleT<EstimateRateLuma<void>> Handle;

} // namespace

template <class TagT> struct SampleType<HandleT<TagT>> { typedef uint8_t Type; };

// levels: n x n int16 (raster); mode against cand[3] gives prev_intra_luma_pred_flag / mpm_idx / rem_intra_luma_pred_mode; split: IntraSplitFlag (the partition is one of
// the four of an NxN unit: blkIdx says which); depthIntra, minTb, maxTb: max_transform_hierarchy_depth_intra, MinTbLog2SizeY, MaxTbLog2SizeY; states: 128 bytes
// (HAVOC_RDOQ_CTX_*), syntax: 4 bytes (HAVOC_INTRA_SYNTAX_CTX_*), both updated in place -> the Q16 rate.  info[0] = mpm_idx (3: rem), info[1] = rem_intra_luma_pred_mode,
// info[2] = MaxTrafoDepth as the syntax set it
extern "C" int64_t intra_rate_candidate(const int16_t *levels, int log2, int mode, const int32_t *cand, int split, int blkIdx, int depthIntra, int minTb, int maxTb, int scan,
                                        int sdh, uint8_t *states, uint8_t *syntax, int32_t *info)
{
    State *st = new State();
    const int n2 = 1 << 2 * log2, log2Cb = log2 + split;
    std::vector<int16_t> block(levels, levels + n2);
    st->levels = block.data();
    st->scan = scan;
    st->sdh = sdh;
    st->split = split;
    st->depthIntra = depthIntra;
    st->minTb = minTb;
    st->maxTb = maxTb;
    st->maxTrafoDepth = -1;
    st->prevFlag = st->mpmIdx = st->rem = -1;
    st->cbf = 0;
    for (int i = 0; i < n2; ++i) st->cbf |= block[i] != 0;
    st->cand.candModeList = {{cand[0], cand[1], cand[2]}};
    st->cand.neighbourModes = 0;
    st->cqt = coding_quadtree(0, 0, log2Cb, 0);
    // the coding unit's words: CuPredMode, part_mode, IntraPredModeY of the partition; the transform tree behind them stays zero
    st->cuWords.assign(64, 0);
    st->residualWords.assign(4 * n2 + 64, 0);
    st->coded.reset(st->cuWords.data());
    st->coded.codedCu.word0().CuPredMode = MODE_INTRA;
    st->coded.codedCu.word0().part_mode = split;
    st->coded.codedCu.IntraPredModeY(split ? blkIdx : 0) = (int8_t)mode;
    Contexts &c = st->cc;
    put<cbf_luma>(c, states + 1, 2);
    put<last_sig_coeff_x_prefix>(c, states + 8, 18);
    put<last_sig_coeff_y_prefix>(c, states + 26, 18);
    put<coded_sub_block_flag>(c, states + 44, 4);
    put<sig_coeff_flag>(c, states + 48, 44);
    put<coeff_abs_level_greater1_flag>(c, states + 92, 24);
    put<coeff_abs_level_greater2_flag>(c, states + 116, 6);
    put<prev_intra_luma_pred_flag>(c, syntax + 0, 1);
    put<split_transform_flag>(c, syntax + 1, 3);
    st->cc.rate = Cost();
    Handle h{ st };
    Syntax<IntraPartition>::go(IntraPartition(0, 0, log2Cb, split, split ? blkIdx : 0), h);
    const int64_t rate = st->cc.rate.value;
    info[0] = st->prevFlag ? st->mpmIdx : 3;
    info[1] = st->rem;
    info[2] = st->maxTrafoDepth;
    take<cbf_luma>(c, states + 1, 2);
    take<last_sig_coeff_x_prefix>(c, states + 8, 18);
    take<last_sig_coeff_y_prefix>(c, states + 26, 18);
    take<coded_sub_block_flag>(c, states + 44, 4);
    take<sig_coeff_flag>(c, states + 48, 44);
    take<coeff_abs_level_greater1_flag>(c, states + 92, 24);
    take<coeff_abs_level_greater2_flag>(c, states + 116, 6);
    take<prev_intra_luma_pred_flag>(c, syntax + 0, 1);
    take<split_transform_flag>(c, syntax + 1, 3);
    delete st;
    return rate;
}
