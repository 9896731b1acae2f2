// TEST INFRASTRUCTURE ONLY.  The reference's own SAO parameter estimation and distortion (turing/EncSao.h:286-947:
// saoRdEstimateLuma, saoRdEstimateChroma, computeSaoDistortion), instantiated over a small stand-in handle.  Compiled with
// oracle/Makefile's TURFLAGS into a temporary directory by tests/sao_decision_tools.py; nothing of the reference is stored.
//
// The stand-in answers the syntax elements those functions read and write, and converts to StateEncode* (only `saoslow` is
// read: false, the estimation reads the reconstruction) and to StateEncodePicture* (only `reciprocalLambda` is read).  Both
// are zeroed storage of the right size: neither object is constructed, so nothing else of the encoder is linked.
#include "turing/StateEncode.h"
#include "turing/Measure.h"
#include "turing/EncSao.h"
#include "turing/sao.h"
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

struct Handle
{
    int addr, wctb, log2, W, H, bd, flags;
    int type[3], eo[3], band[3], oabs[3][4], osign[3][4];
    alignas(64) unsigned char enc[sizeof(StateEncode)];
    alignas(64) unsigned char pic[sizeof(StateEncodePicture)];

    int operator[](CtbAddrInRs) const { return addr; }
    int operator[](PicWidthInCtbsY) const { return wctb; }
    int operator[](CtbLog2SizeY) const { return log2; }
    int operator[](pic_width_in_luma_samples) const { return W; }
    int operator[](pic_height_in_luma_samples) const { return H; }
    int operator[](BitDepthY) const { return bd; }
    int operator[](BitDepthC) const { return bd; }
    int operator[](xCtb) const { return (addr % wctb) << log2; }
    int operator[](yCtb) const { return (addr / wctb) << log2; }
    int operator[](slice_sao_luma_flag) const { return flags & 1; }
    int operator[](slice_sao_chroma_flag) const { return (flags >> 1) & 1; }
    int operator[](slice_tc_offset_div2) const { return 0; }
    int operator[](slice_beta_offset_div2) const { return 0; }
    int &operator[](SaoTypeIdx e) { return type[e.cIdx]; }
    int &operator[](SaoEoClass e) { return eo[e.cIdx]; }
    int &operator[](sao_band_position e) { return band[e.cIdx]; }
    int &operator[](sao_offset_abs e) { return oabs[e.cIdx][e.i]; }
    int &operator[](sao_offset_sign e) { return osign[e.cIdx][e.i]; }
    operator StateEncode *() { return reinterpret_cast<StateEncode *>(enc); }
    operator StateEncodePicture *() { return reinterpret_cast<StateEncodePicture *>(pic); }
};

// samples of the padded planar layout (Y, then Cb, then Cr; pad samples on every side of each plane) into a reference picture,
// one sample beyond the picture included (what the edge filter reads at the picture's border)
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

template <typename Sample>
void run(const Sample *const src[3], const Sample *const rec[3], Sample *const dst[3], const intptr_t strides[3], int W, int H, int log2, int bd,
         int32_t lambda_q16, int flags, int32_t *out)
{
    PictureWrap<Sample> org(W, H, 1, 16, 16, 32);
    StateReconstructedPicture<Sample> recPic;
    recPic.picture.reset(new Picture<Sample>(W, H, 1, 16, 16, 32));
    recPic.saoPicture.reset(new Picture<Sample>(W, H, 1, 16, 16, 32));
    load<Sample>(org, src, strides, W, H);
    load<Sample>(*recPic.picture, rec, strides, W, H);
    load<Sample>(*recPic.saoPicture, rec, strides, W, H);     // a component that is off keeps the reconstruction

    std::vector<Handle> hs(1);
    Handle &h = hs[0];
    std::memset(&h, 0, sizeof h);
    h.wctb = (W + (1 << log2) - 1) >> log2;
    h.log2 = log2;
    h.W = W;
    h.H = H;
    h.bd = bd;
    h.flags = flags;
    reinterpret_cast<StateEncodePicture *>(h.pic)->reciprocalLambda.value = lambda_q16;
    const int nctus = h.wctb * ((H + (1 << log2) - 1) >> log2);
    for (int a = 0; a < nctus; ++a, out += 32)
    {
        h.addr = a;
        std::memset(h.type, 0, sizeof h.type + sizeof h.eo + sizeof h.band + sizeof h.oabs + sizeof h.osign);
        EncSao est;
        if (flags & 1) est.saoRdEstimateLuma(h, org, &recPic);
        if (flags & 2) est.saoRdEstimateChroma(h, org, &recPic);
        // out per CTU: for luma and chroma type, eo class, band position, offset_abs[4], offset_sign[4] (2 x 11), dist_sao, dist_off
        for (int c = 0; c < 2; ++c)
        {
            const int ci = c ? 1 : 0;
            int32_t *o = out + 11 * c;
            o[0] = h.type[ci];
            o[1] = h.eo[ci];
            o[2] = h.band[ci];
            for (int i = 0; i < 4; ++i) o[3 + i] = h.oabs[ci][i], o[7 + i] = h.osign[ci][i];
        }
        const int rx = a % h.wctb, ry = a / h.wctb;
        out[22] = EncSao().computeSaoDistortion(h, org, &recPic, rx, ry);
        const int keep[3] = { h.type[0], h.type[1], h.type[2] };
        h.type[0] = h.type[1] = h.type[2] = 0;
        out[23] = EncSao().computeSaoDistortion(h, org, &recPic, rx, ry);
        h.type[0] = keep[0], h.type[1] = keep[1], h.type[2] = keep[2];
    }
    for (int c = 0; c < 3; ++c)
    {
        const int w = c ? W / 2 : W, hh = c ? H / 2 : H;
        for (int y = 0; y < hh; ++y)
            for (int x = 0; x < w; ++x) dst[c][y * strides[c] + x] = (*recPic.saoPicture)[c](x, y);
    }
}

} // namespace

// planes: padded planar pictures, each plane's pointer at its sample (0, 0); out: 32 int32 per CTU in raster order
extern "C" void sao_rd_picture_u8(const uint8_t *const src[3], const uint8_t *const rec[3], uint8_t *const dst[3], const intptr_t strides[3], int W, int H,
                                  int log2, int bd, int32_t lambda_q16, int flags, int32_t *out)
{ run<uint8_t>(src, rec, dst, strides, W, H, log2, bd, lambda_q16, flags, out); }
extern "C" void sao_rd_picture_u16(const uint16_t *const src[3], const uint16_t *const rec[3], uint16_t *const dst[3], const intptr_t strides[3], int W, int H,
                                   int log2, int bd, int32_t lambda_q16, int flags, int32_t *out)
{ run<uint16_t>(src, rec, dst, strides, W, H, log2, bd, lambda_q16, flags, out); }
