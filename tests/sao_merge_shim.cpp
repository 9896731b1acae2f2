// TEST INFRASTRUCTURE ONLY.  The reference's own SAO decision of a picture (turing/EncSao.h:949-1121, EncSao::rdSao, with the estimates
// it calls and Search<sao>::go, Search.hpp:641-705, pricing its candidates), instantiated over a small stand-in handle.  Compiled with
// oracle/Makefile's TURFLAGS into a temporary directory by tests/sao_merge_tools.py; nothing of the reference is stored.
//
// The stand-in is one State shared by handles of every verb: change<Verb>() gives a handle whose operator() dispatches a syntax element
// or a bin to Verb<...> (EstimateRate: Write's binarisation, measureEncodeDecision on the contexts, 1 << 16 per bypass bin).  It answers
// the syntax values the encoder reads and writes, with the SAO parameters of every CTU in a real StateSpatial::snakeSaoCtuData, and
// converts to:
//   StateEncode *            zeroed storage (only `saoslow` is read: false)
//   StateEncodePicture *     zeroed storage (only `reciprocalLambda` is read)
//   Candidate<Sample> *      zeroed storage with a real ContextsAndCost constructed where Candidate keeps it (only that base is used)
//   Contexts *, StateEstimateRate *   that ContextsAndCost
//   StateSpatial *, sao *    real objects
// The picture is walked in coding order like StatePictures.h:1030-1105: the CTU's SaoCtuData is reset, the contexts start from
// Contexts::initialize (slice start, or a WPP row whose CTU (1, r - 1) does not exist) or from the copy saved after CTU (1, r - 1); after
// rdSao (which restores the contexts it found) the chosen syntax is run once more through the context-updating EstimateRate -- the same
// context bins Write codes (SyntaxCtu.hpp:44-84; Cr's bins are bypass) -- and computeSaoDistortion gives the final distortion and,
// over the CTU copied from the reconstruction, leaves it filtered with the final parameters in saoPicture.
#include "turing/StateEncode.h"
#include "turing/Measure.h"
#include "turing/EncSao.h"
#include "turing/EstimateRate.h"
#include "turing/Search.hpp"
#include "turing/sao.h"
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

namespace {

template <class Tag, class F> struct Rebind;
template <template <class> class Verb, class F> struct Rebind<Verb<void>, F> { typedef Verb<F> type; };

struct State
{
    int addr, wctb, log2, W, H, bd, flags, mergeLeft, mergeUp;
    StateEncode *enc;
    StateEncodePicture *pic;
    void *candidate;
    ContextsAndCost *cc;
    StateSpatial spatial;
    sao s;
};

template <class Tag>
struct Handle
{
    State *st;

    template <class NewTag> Handle<NewTag> change() { return Handle<NewTag>{ st }; }
    template <class V, class M> void operator()(V v, M m) { Rebind<Tag, Element<V, M>>::type::go(Element<V, M>{ v, m }, *this); }
    template <class F> void operator()(F f) { Rebind<Tag, F>::type::go(f, *this); }

    SaoCtuData &ctu(int rx, int ry) { return const_cast<SaoCtuData &>(st->spatial.snakeSaoCtuData.at(rx, ry, 0)); }

    int operator[](CtbAddrInRs) const { return st->addr; }
    int operator[](CtbAddrInTs) const { return st->addr; }
    int operator[](CtbAddrRsToTs e) const { return e.ctbAddrRS; }
    int operator[](TileId) const { return 0; }
    int operator[](SliceAddrRs) const { return 0; }
    int operator[](PicWidthInCtbsY) const { return st->wctb; }
    int operator[](CtbLog2SizeY) const { return st->log2; }
    int operator[](pic_width_in_luma_samples) const { return st->W; }
    int operator[](pic_height_in_luma_samples) const { return st->H; }
    int operator[](BitDepthY) const { return st->bd; }
    int operator[](BitDepthC) const { return st->bd; }
    int operator[](xCtb) const { return (st->addr % st->wctb) << st->log2; }
    int operator[](yCtb) const { return (st->addr / st->wctb) << st->log2; }
    int operator[](slice_sao_luma_flag) const { return st->flags & 1; }
    int operator[](slice_sao_chroma_flag) const { return (st->flags >> 1) & 1; }
    int operator[](slice_tc_offset_div2) const { return 0; }
    int operator[](slice_beta_offset_div2) const { return 0; }
    // (read on rdSao's saoslow path only, which is compiled but never taken)
    int operator[](slice_deblocking_filter_disabled_flag) const { return 1; }
    int operator[](PicOrderCntVal) const { return 0; }
    int operator[](SubWidthC) const { return 2; }
    int operator[](SubHeightC) const { return 2; }
    int operator[](pps_cb_qp_offset) const { return 0; }
    int operator[](pps_cr_qp_offset) const { return 0; }
    int &operator[](sao_merge_left_flag) { return st->mergeLeft; }
    int &operator[](sao_merge_up_flag) { return st->mergeUp; }
    auto &operator[](SaoTypeIdx e) { return static_cast<ValueHolder<SaoTypeIdx> &>(ctu(e.rx, e.ry)).get(e); }
    auto &operator[](SaoEoClass e) { return static_cast<ValueHolder<SaoEoClass> &>(ctu(e.rx, e.ry)).get(e); }
    auto &operator[](sao_band_position e) { return static_cast<ValueHolder<sao_band_position> &>(ctu(e.rx, e.ry)).get(e); }
    auto &operator[](sao_offset_abs e) { return static_cast<ValueHolder<sao_offset_abs> &>(ctu(e.rx, e.ry)).get(e); }
    auto &operator[](sao_offset_sign e) { return static_cast<ValueHolder<sao_offset_sign> &>(ctu(e.rx, e.ry)).get(e); }

    operator StateEncode *() { return st->enc; }
    operator StateEncodePicture *() { return st->pic; }
    template <typename Sample> operator Candidate<Sample> *() { return static_cast<Candidate<Sample> *>(st->candidate); }
    operator Contexts *() { return st->cc; }
    operator StateEstimateRate *() { return st->cc; }
    operator StateSpatial *() { return &st->spatial; }
    operator sao *() { return &st->s; }
};

template <typename Sample>
void load(ThreePlanes<Sample> &p, const Sample *const planes[3], const intptr_t strides[3], int W, int H)
{
    for (int c = 0; c < 3; ++c)
    {
        const int w = c ? W / 2 : W, h = c ? H / 2 : H;
        for (int y = -1; y <= h; ++y)
            for (int x = -1; x <= w; ++x) p[c](x, y) = planes[c][y * strides[c] + x];
    }
}

uint8_t merge_state(ContextsAndCost &c) { return c.get<sao_merge_X_flag>(0).state; }
uint8_t type_state(ContextsAndCost &c) { return c.get<sao_type_idx_X>(0).state; }

template <typename Sample>
void run(const Sample *const src[3], const Sample *const rec[3], Sample *const dst[3], const intptr_t strides[3], int W, int H, int log2, int bd,
         int32_t lambda_q16, int flags, int slice_qp, int init_type, int32_t *out)
{
    PictureWrap<Sample> org(W, H, 1, 16, 16, 32);
    StateReconstructedPicture<Sample> recPic;
    recPic.picture.reset(new Picture<Sample>(W, H, 1, 16, 16, 32));
    recPic.saoPicture.reset(new Picture<Sample>(W, H, 1, 16, 16, 32));
    load<Sample>(org, src, strides, W, H);
    load<Sample>(*recPic.picture, rec, strides, W, H);
    load<Sample>(*recPic.saoPicture, rec, strides, W, H);

    std::vector<unsigned char> enc(sizeof(StateEncode)), pic(sizeof(StateEncodePicture)), cand(sizeof(Candidate<Sample>));
    State *st = new State();
    st->enc = reinterpret_cast<StateEncode *>(enc.data());
    st->pic = reinterpret_cast<StateEncodePicture *>(pic.data());
    st->pic->reciprocalLambda.value = lambda_q16;
    st->candidate = cand.data();
    st->cc = new (static_cast<ContextsAndCost *>(reinterpret_cast<Candidate<Sample> *>(cand.data()))) ContextsAndCost();
    st->wctb = (W + (1 << log2) - 1) >> log2;
    const int hctb = (H + (1 << log2) - 1) >> log2;
    st->log2 = log2;
    st->W = W;
    st->H = H;
    st->bd = bd;
    st->flags = flags & 3;
    Turing::Rectangle rectangle{ 0, 0, st->wctb, hctb };
    st->spatial.snakeSaoCtuData.resize(rectangle, 0);
    Handle<Search<void>> h{ st };

    Contexts initial, wpp;
    initial.initialize(slice_qp, init_type);
    static_cast<Contexts &>(*st->cc) = initial;
    for (int a = 0; a < st->wctb * hctb; ++a, out += 32)
    {
        const int rx = a % st->wctb, ry = a / st->wctb;
        st->addr = a;
        st->s.rx = rx;
        st->s.ry = ry;
        if (rx == 0 && ry > 0 && (flags & 4))
            static_cast<Contexts &>(*st->cc) = st->wctb >= 2 ? wpp : initial;
        st->cc->resetZero();
        st->spatial.snakeSaoCtuData.commit(SaoCtuData(), rx, ry, 0);
        st->mergeLeft = st->mergeUp = 0;
        const uint8_t mBefore = merge_state(*st->cc), tBefore = type_state(*st->cc);
        int dist;
        if (flags & 3)
        {
            EncSao().rdSao<Sample>(h, org, &recPic, rx, ry);
            // computeSaoDistortion writes only the components that are not type 0 (EncSao.h:861-934: one that is off is measured against
            // the reconstruction and saoPicture keeps what the last candidate left there): start the CTU from the reconstruction, so that
            // saoPicture holds it in the form its distortion was measured in
            for (int c = 0; c < 3; ++c)
            {
                const int sh = c ? 1 : 0, x0 = (rx << log2) >> sh, y0 = (ry << log2) >> sh;
                const int x1 = std::min((rx + 1) << log2, W) >> sh, y1 = std::min((ry + 1) << log2, H) >> sh;
                for (int y = y0; y < y1; ++y)
                    for (int x = x0; x < x1; ++x) (*recPic.saoPicture)[c](x, y) = (*recPic.picture)[c](x, y);
            }
            dist = EncSao().computeSaoDistortion<Sample>(h, org, &recPic, rx, ry);
            Search<sao>::go(st->s, h);           // the final syntax through the context-updating EstimateRate
        }
        else
            dist = EncSao().computeSaoDistortion<Sample>(h, org, &recPic, rx, ry);
        // out per CTU: the final SaoCtuData as the reference holds it (luma, Cb: type, class, band, offset_abs[4], offset_sign[4]; stale
        // fields of a type-0 component included), merge flags, distortion, -, the four context states, 1, then Cr's type, class, band
        for (int c = 0; c < 2; ++c)
        {
            int32_t *o = out + 11 * c;
            o[0] = h[SaoTypeIdx(c, rx, ry)];
            o[1] = h[SaoEoClass(c, rx, ry)];
            o[2] = h[sao_band_position(c, rx, ry)];
            for (int i = 0; i < 4; ++i) o[3 + i] = h[sao_offset_abs(c, rx, ry, i)], o[7 + i] = h[sao_offset_sign(c, rx, ry, i)];
        }
        out[22] = st->mergeLeft;
        out[23] = st->mergeUp;
        out[24] = dist;
        out[25] = -2;
        out[26] = mBefore | tBefore << 8 | merge_state(*st->cc) << 16 | type_state(*st->cc) << 24;
        out[27] = 1;
        out[28] = h[SaoTypeIdx(2, rx, ry)];
        out[29] = h[SaoEoClass(2, rx, ry)];
        out[30] = h[sao_band_position(2, rx, ry)];
        out[31] = 0;
        if (rx == 1) wpp = *st->cc;          // the storage process after the second CTU of a row (9.3.2.2)
    }
    for (int c = 0; c < 3; ++c)
    {
        const int w = c ? W / 2 : W, hh = c ? H / 2 : H;
        for (int y = 0; y < hh; ++y)
            for (int x = 0; x < w; ++x) dst[c][y * strides[c] + x] = (*recPic.saoPicture)[c](x, y);
    }
    st->cc->~ContextsAndCost();
    delete st;
}

} // namespace

// planes: padded planar pictures, each plane's pointer at its sample (0, 0); flags: bit 0 luma, bit 1 chroma, bit 2 WPP; out: 32 int32 per CTU
extern "C" void sao_merge_picture_u8(const uint8_t *const src[3], const uint8_t *const rec[3], uint8_t *const dst[3], const intptr_t strides[3], int W, int H,
                                     int log2, int bd, int32_t lambda_q16, int flags, int slice_qp, int init_type, int32_t *out)
{ run<uint8_t>(src, rec, dst, strides, W, H, log2, bd, lambda_q16, flags, slice_qp, init_type, out); }
extern "C" void sao_merge_picture_u16(const uint16_t *const src[3], const uint16_t *const rec[3], uint16_t *const dst[3], const intptr_t strides[3], int W,
                                      int H, int log2, int bd, int32_t lambda_q16, int flags, int slice_qp, int init_type, int32_t *out)
{ run<uint16_t>(src, rec, dst, strides, W, H, log2, bd, lambda_q16, flags, slice_qp, init_type, out); }

// the two SAO contexts after Contexts::initialize(slice_qp, init_type): out[0] sao_merge_X_flag, out[1] sao_type_idx_X
extern "C" void sao_context_states(int slice_qp, int init_type, int32_t *out)
{
    ContextsAndCost c;
    c.initialize(slice_qp, init_type);
    out[0] = merge_state(c);
    out[1] = type_state(c);
}

// measureEncodeDecision (Write.h:476-492) from every state and bin: out[2 state + bin] = new state | Q16 rate << 8
extern "C" void sao_bin_table(int64_t *out)
{
    for (int s = 0; s < 128; ++s)
        for (int b = 0; b < 2; ++b)
        {
            ContextModel m;
            m.state = (uint8_t)s;
            const Cost r = measureEncodeDecision(m, b);
            out[2 * s + b] = m.state | r.value << 8;
        }
}
