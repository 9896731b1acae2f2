// TEST INFRASTRUCTURE ONLY.  The reference's own rate of one residual_coding: CodedData::storeResidual (turing/CodedData.h:457-517) over an n x n raster of
// levels, then EncodeResidual::inner<false, is4x4, Handle<EstimateRate<void>>> (turing/EncodeResidual.hpp:36-301) over a small stand-in handle.  Compiled with
// oracle/Makefile's TURFLAGS into a temporary directory by tests/residual_rate_tools.py; nothing of the reference is stored.
//
// The stand-in holds a real Contexts + StateEstimateRate (ContextsAndCost) filled from and read back to the flat 128-byte layout of include/havoc_mi355x.h
// (HAVOC_RDOQ_CTX_*, as oracle/ref_shim_rdoq.cpp fills it), a residual_coding and a StateCodedData over a scratch buffer.  It answers scanIdx,
// sign_data_hiding_enabled_flag, transform_skip_enabled_flag = 0 and cu_transquant_bypass_flag = 0, keeps the last-position prefixes and suffixes the walk sets, and
// dispatches elements and bins to EstimateRate<...> (Write's binarisation, measureEncodeDecision on the contexts, one whole bit per bypass bin).
#include "turing/StateEncode.h"
#include "turing/EstimateRate.h"
#include "turing/EncodeResidual.hpp"
#include "turing/CodedData.h"
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

template <class Tag, class F> struct Rebind;
template <template <class> class Verb, class F> struct Rebind<Verb<void>, F> { typedef Verb<F> type; };

struct State
{
    ContextsAndCost cc;
    residual_coding rc;
    StateCodedData coded;
    int scan, sdh;
    int lastX[2], lastY[2];      // prefix, suffix
    State() : rc(0, 0, 2, 0) {}
};

struct Handle
{
    typedef EstimateRate<void> Tag;
    State *st;

    template <class V, class M> void operator()(V v, M m) { Rebind<Tag, Element<V, M>>::type::go(Element<V, M>{ v, m }, *this); }
    template <class F> void operator()(F f) { Rebind<Tag, F>::type::go(f, *this); }

    int operator[](scanIdx) const { return st->scan; }
    int operator[](sign_data_hiding_enabled_flag) const { return st->sdh; }
    int operator[](transform_skip_enabled_flag) const { return 0; }
    int operator[](cu_transquant_bypass_flag) const { return 0; }
    int operator[](Log2MaxTransformSkipSize) const { return 2; }
    int &operator[](last_sig_coeff_x_prefix) { return st->lastX[0]; }
    int &operator[](last_sig_coeff_x_suffix) { return st->lastX[1]; }
    int &operator[](last_sig_coeff_y_prefix) { return st->lastY[0]; }
    int &operator[](last_sig_coeff_y_suffix) { return st->lastY[1]; }
    int operator[](transform_skip_flag) const { return 0; }

    operator residual_coding *() { return &st->rc; }
    operator Contexts *() { return &st->cc; }
    operator StateEstimateRate *() { return &st->cc; }
    operator StateCodedData *() { return &st->coded; }
    operator StateEncodeSubstreamBase *() { return nullptr; }          // (inner takes the pointers; it reads neither under the EstimateRate tag)
    template <class Sample> operator StateReconstructionCache<Sample> *() { return nullptr; }
};

template <class Tag> void put(Contexts &c, const uint8_t *s, int n) { for (int i = 0; i < n; ++i) c.get<Tag>(i).state = s[i]; }
template <class Tag> void take(Contexts &c, uint8_t *s, int n) { for (int i = 0; i < n; ++i) s[i] = c.get<Tag>(i).state; }

} // namespace

template <> struct SampleType<Handle> { typedef uint8_t Type; };

// levels: `count` blocks of n x n int16 (raster) one after the other; states: 128 bytes, updated in place; rates: count int64 (Q16 Cost, 0 for an all-zero block)
extern "C" void residual_rate_chain(const int16_t *levels, int count, int log2, int cIdx, int scan, int sdh, uint8_t *states, int64_t *rates)
{
    State *st = new State();
    st->scan = scan;
    st->sdh = sdh;
    st->rc = residual_coding(0, 0, log2, cIdx);
    Contexts &c = st->cc;
    put<last_sig_coeff_x_prefix>(c, states + 8, 18);
    put<last_sig_coeff_y_prefix>(c, states + 26, 18);
    put<coded_sub_block_flag>(c, states + 44, 4);
    put<sig_coeff_flag>(c, states + 48, 44);
    put<coeff_abs_level_greater1_flag>(c, states + 92, 24);
    put<coeff_abs_level_greater2_flag>(c, states + 116, 6);
    const int n2 = 1 << 2 * log2;
    std::vector<CodedData::Type> buffer(4 * n2 + 64), scratch(16);
    std::vector<int16_t> block(n2);
    Handle h{ st };
    for (int k = 0; k < count; ++k)
    {
        std::memcpy(block.data(), levels + (size_t)k * n2, n2 * sizeof(int16_t));
        bool cbf = false;
        for (int i = 0; i < n2; ++i) cbf |= block[i] != 0;
        st->cc.rate = Cost();
        if (cbf)      // IfCbf: a block without a coded level has no residual_coding
        {
            std::fill(buffer.begin(), buffer.end(), 0);
            std::fill(scratch.begin(), scratch.end(), 0);
            CodedData::Residual residual;
            residual.p = buffer.data();
            CodedData::CodingUnit cu;
            cu.p = scratch.data();
            CodedData::TransformTree tt;
            tt.p = scratch.data() + 8;
            CodedData::storeResidual(cu, residual, block.data(), log2, scan, true, tt, cIdx);
            st->coded.residual.p = buffer.data();
            if (log2 == 2) EncodeResidual::inner<false, true>(h);
            else EncodeResidual::inner<false, false>(h);
        }
        rates[k] = st->cc.rate.value;
    }
    take<last_sig_coeff_x_prefix>(c, states + 8, 18);
    take<last_sig_coeff_y_prefix>(c, states + 26, 18);
    take<coded_sub_block_flag>(c, states + 44, 4);
    take<sig_coeff_flag>(c, states + 48, 44);
    take<coeff_abs_level_greater1_flag>(c, states + 92, 24);
    take<coeff_abs_level_greater2_flag>(c, states + 116, 6);
    delete st;
}
