// TEST INFRASTRUCTURE ONLY.  The reference's own in-loop SAO of a picture: LoopFilter::Picture (turing/LoopFilter.h) instantiated over a
// small stand-in handle, in both of the reference's forms.  Compiled with oracle/Makefile's TURFLAGS into a temporary directory by
// tests/sao_apply_tools.py and linked with the havoc objects oracle/Makefile's `ref` target builds; nothing of the reference is stored.
//
// Per CTU in raster order the reference's own processCtu runs -- Ctu::set on the SAO syntax the handle answers (SaoTypeIdx, SaoEoClass,
// sao_band_position, sao_offset_abs / sign per CTU; Cr answers Cb's values, as one chroma record drives both), and the bounds and corner
// flags of neighbourCtuAvailable from the slice addresses and slice_loop_filter_across_slices_enabled_flag the handle answers (one tile).
// The deblocking bytes go into LoopFilter::Picture::blocks.  Then both forms:
//   encoder  TaskSao.cpp:96-121: per CTU, copy the window [rx, rx + 2) x [ry, ry + 2) of the picture into saoPicture, then applySaoCTU
//            (filterBlockSao from saoPicture into the picture);
//   decoder  applySao2 (LoopFilter.h:780-791) from the picture into a separate saoPicture.
// Type-0 CTUs go through havocGetPredUni, its table populated by the reference's own havocPopulatePredUni.  The pictures are allocated
// over the whole CTU grid: the reference writes chroma beyond the picture's right and bottom edges (LoopFilter.h:895-897).
#include "turing/StatePicture.h"
#include "turing/LoopFilter.h"
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

struct State
{
    int addr, wctb, hctb, log2, W, H, bd, flags;
    const int32_t *params;           // per CTU: luma then chroma, 11 int32 each (type, eo_class, band_position, offset_abs[4], offset_sign[4])
    const int32_t *slice_addr, *across;
    void *predUni;
    void *recPic;
};

struct Handle
{
    State *st;

    int comp(int cIdx, int rx, int ry, int k) const { return st->params[(ry * st->wctb + rx) * 22 + (cIdx ? 11 : 0) + k]; }

    int operator[](CtbAddrInRs) const { return st->addr; }
    int operator[](CtbAddrInTs) const { return st->addr; }
    int operator[](CtbAddrRsToTs e) const { return e.ctbAddrRS; }
    int operator[](TileId) const { return 0; }
    int operator[](loop_filter_across_tiles_enabled_flag) const { return 1; }
    int operator[](SliceAddrRs) const { return st->slice_addr[st->addr]; }
    int operator[](slice_loop_filter_across_slices_enabled_flag) const { return st->across[st->addr]; }
    int operator[](PicWidthInCtbsY) const { return st->wctb; }
    int operator[](PicHeightInCtbsY) const { return st->hctb; }
    int operator[](PicSizeInCtbsY) const { return st->wctb * st->hctb; }
    int operator[](CtbLog2SizeY) const { return st->log2; }
    int operator[](CtbSizeY) const { return 1 << st->log2; }
    int operator[](pic_width_in_luma_samples) const { return st->W; }
    int operator[](pic_height_in_luma_samples) const { return st->H; }
    int operator[](BitDepthY) const { return st->bd; }
    int operator[](BitDepthC) const { return st->bd; }
    int operator[](xCtb) const { return (st->addr % st->wctb) << st->log2; }
    int operator[](yCtb) const { return (st->addr / st->wctb) << st->log2; }
    int operator[](SubWidthC) const { return 2; }
    int operator[](SubHeightC) const { return 2; }
    int operator[](slice_sao_luma_flag) const { return st->flags & 1; }
    int operator[](slice_sao_chroma_flag) const { return (st->flags >> 1) & 1; }
    int operator[](slice_tc_offset_div2) const { return 0; }
    int operator[](slice_beta_offset_div2) const { return 0; }
    int operator[](SaoTypeIdx e) const { return comp(e.cIdx, e.rx, e.ry, 0); }
    int operator[](SaoEoClass e) const { return comp(e.cIdx, e.rx, e.ry, 1); }
    int operator[](sao_band_position e) const { return comp(e.cIdx, e.rx, e.ry, 2); }
    int operator[](sao_offset_abs e) const { return comp(e.cIdx, e.rx, e.ry, 3 + e.i); }
    int operator[](sao_offset_sign e) const { return comp(e.cIdx, e.rx, e.ry, 7 + e.i); }

    template <typename Sample> operator HavocTablePredUni<Sample> *() { return static_cast<HavocTablePredUni<Sample> *>(st->predUni); }
    template <typename Sample> operator StateReconstructedPicture<Sample> *() { return static_cast<StateReconstructedPicture<Sample> *>(st->recPic); }
};

template <typename Sample>
void run(const Sample *const rec[3], Sample *const enc[3], Sample *const dec[3], const intptr_t strides[3], int W, int H, int log2, int bd, int flags,
         const int32_t *params, const int32_t *slice_addr, const int32_t *across, const int8_t *block_data, intptr_t block_stride)
{
    State st{};
    st.wctb = (W + (1 << log2) - 1) >> log2;
    st.hctb = (H + (1 << log2) - 1) >> log2;
    st.log2 = log2, st.W = W, st.H = H, st.bd = bd, st.flags = flags;
    st.params = params, st.slice_addr = slice_addr, st.across = across;
    const int GW = st.wctb << log2, GH = st.hctb << log2;

    havoc_code code = havoc_new_code((havoc_instruction_set)(HAVOC_C_REF | HAVOC_C_OPT), 1 << 20);
    HavocTablePredUni<Sample> predUni;
    havocPopulatePredUni<Sample>(&predUni, code);
    st.predUni = &predUni;

    StateReconstructedPicture<Sample> recPic;
    recPic.picture.reset(new Picture<Sample>(GW, GH, 1, 16, 16, 32));
    recPic.saoPicture.reset(new Picture<Sample>(GW, GH, 1, 16, 16, 32));
    Picture<Sample> decPicture(GW, GH, 1, 16, 16, 32), decSao(GW, GH, 1, 16, 16, 32);
    st.recPic = &recPic;
    for (int c = 0; c < 3; ++c)
    {
        const int w = c ? W / 2 : W, h = c ? H / 2 : H;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) (*recPic.picture)[c](x, y) = decPicture[c](x, y) = rec[c][y * strides[c] + x];
    }

    Handle h{ &st };
    LoopFilter::Picture pic(h);
    for (int y = 0; y < GH / 8; ++y)
        for (int x = 0; x < GW / 8; ++x)
            pic.blockAt(x, y).data = (block_data && x < (W + 7) / 8 && y < (H + 7) / 8) ? block_data[y * block_stride + x] : 0;
    for (int a = 0; a < st.wctb * st.hctb; ++a)
    {
        st.addr = a;
        pic.processCtu(h, coding_tree_unit());
    }

    // the encoder's form (TaskSao.cpp:96-121, sample_adaptive_offset_enabled_flag set)
    for (int ry = 0; ry < st.hctb; ++ry)
        for (int rx = 0; rx < st.wctb; ++rx)
        {
            st.addr = ry * st.wctb + rx;
            for (int cIdx = 0; cIdx < 3; cIdx++)
            {
                int xBegin = rx << log2, yBegin = ry << log2;
                int xEnd = std::min((rx + 2) << log2, W), yEnd = std::min((ry + 2) << log2, H);
                if (cIdx != 0) xBegin >>= 1, yBegin >>= 1, xEnd >>= 1, yEnd >>= 1;
                for (int y = yBegin; y < yEnd; ++y)
                    for (int x = xBegin; x < xEnd; ++x) (*recPic.saoPicture)[cIdx](x, y) = (*recPic.picture)[cIdx](x, y);
            }
            pic.applySaoCTU<Sample>(h, rx, ry);
        }
    // the decoder's form
    pic.applySao2<Sample>(h, decSao, decPicture);

    for (int c = 0; c < 3; ++c)
    {
        const int w = c ? W / 2 : W, hh = c ? H / 2 : H;
        for (int y = 0; y < hh; ++y)
            for (int x = 0; x < w; ++x)
            {
                enc[c][y * strides[c] + x] = (*recPic.picture)[c](x, y);
                dec[c][y * strides[c] + x] = decSao[c](x, y);
            }
    }
    havoc_delete_code(code);
}

} // namespace

// planes: each plane's pointer at its sample (0, 0), strides[3] in samples (the outputs share them); params: 22 int32 per CTU in raster
// order; slice_addr / across: per CTU, the address of its slice's first CTU and that slice's slice_loop_filter_across_slices_enabled_flag;
// block_data: (QpY << 1) | disabled per 8x8 luma region, row stride block_stride, or null
extern "C" void sao_apply_u8(const uint8_t *const rec[3], uint8_t *const enc[3], uint8_t *const dec[3], const intptr_t strides[3], int W, int H, int log2,
                             int bd, int flags, const int32_t *params, const int32_t *slice_addr, const int32_t *across, const int8_t *block_data,
                             intptr_t block_stride)
{ run<uint8_t>(rec, enc, dec, strides, W, H, log2, bd, flags, params, slice_addr, across, block_data, block_stride); }
extern "C" void sao_apply_u16(const uint16_t *const rec[3], uint16_t *const enc[3], uint16_t *const dec[3], const intptr_t strides[3], int W, int H,
                              int log2, int bd, int flags, const int32_t *params, const int32_t *slice_addr, const int32_t *across,
                              const int8_t *block_data, intptr_t block_stride)
{ run<uint16_t>(rec, enc, dec, strides, W, H, log2, bd, flags, params, slice_addr, across, block_data, block_stride); }

// processCtu's LoopFilter::Ctu bounds of every CTU: out[8 a ..] = left, top, right, bottom, corners (bit 0 TL, 1 TR, 2 BL, 3 BR)
extern "C" void sao_apply_bounds(int W, int H, int log2, const int32_t *slice_addr, const int32_t *across, int32_t *out)
{
    State st{};
    st.wctb = (W + (1 << log2) - 1) >> log2;
    st.hctb = (H + (1 << log2) - 1) >> log2;
    st.log2 = log2, st.W = W, st.H = H, st.bd = 8, st.flags = 0;
    std::vector<int32_t> zeros(22 * st.wctb * st.hctb);
    st.params = zeros.data(), st.slice_addr = slice_addr, st.across = across;
    Handle h{ &st };
    LoopFilter::Picture pic(h);
    for (int a = 0; a < st.wctb * st.hctb; ++a)
    {
        st.addr = a;
        pic.processCtu(h, coding_tree_unit());
    }
    for (int a = 0; a < st.wctb * st.hctb; ++a)
    {
        const LoopFilter::Ctu &c = pic.ctus[a];
        int32_t *o = out + 8 * a;
        o[0] = c.left, o[1] = c.top, o[2] = c.right, o[3] = c.bottom;
        o[4] = c.topLeft | c.topRight << 1 | c.bottomLeft << 2 | c.bottomRight << 3;
        o[5] = o[6] = o[7] = 0;
    }
}
