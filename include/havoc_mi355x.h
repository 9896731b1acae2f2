/*
 * havoc_mi355x.h -- C ABI of libhavoc_mi355x.so, the MI355X (gfx950) implementation of the `havoc`
 * primitive layer of the Turing HEVC encoder.
 *
 * Each batch entry point evaluates MANY independent calls of one reference primitive in one kernel launch.
 * A "job" carries what the reference passes per call as pointers (here: sample offsets into planes that
 * already live in HBM) and block geometry; strides and bit depth are per launch.  Results are bit-identical
 * to the reference function cited next to each entry point.
 *
 * Conventions
 *   - every `d_*` pointer is DEVICE memory (hipMalloc / torch.cuda); nothing is copied to or from the host
 *     unless the name says so (`*_h2d`, `*_d2h`, and the classic per-block API in havoc_classic.hpp);
 *   - `S` = bytes per sample: 1 (uint8_t, 8-bit) or 2 (uint16_t, 9/10-bit), the reference's `Sample` type;
 *   - offsets and strides are in SAMPLES (int16 elements for coefficient buffers), exactly like the
 *     reference's pointer arithmetic (havoc/sad.h:58 etc.); offsets are relative to the plane base pointer
 *     passed to the call and may address the 96-sample picture padding (turing/StatePictures.h:155-156);
 *   - launches are asynchronous on the context's HIP stream; call havoc_mi355x_sync() before reading results
 *     on the host.  Every function returns 0 on success or a negative hipError_t / HAVOC_MI355X_E* code;
 *     havoc_mi355x_last_error() gives the text.  The reference has no error channel: a
 *     failure here means the launch did not happen, never that a CPU path was taken.
 */
#ifndef HAVOC_MI355X_H
#define HAVOC_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HAVOC_MI355X_EINVAL (-10001) /* bad argument (S, taps, bit depth, size) */
#define HAVOC_MI355X_ENODEV (-10002) /* no gfx950 device / HIP runtime unavailable */
#define HAVOC_MI355X_EDEVICE (-10003) /* a kernel reported that it could not finish (havoc_mi355x_search_picture_uni: a wait gave up) */

typedef struct havoc_mi355x_ctx havoc_mi355x_ctx;

/* ---- context: replaces havoc_new_code / havoc_delete_code (havoc/havoc.h:138-147, havoc.cpp:144-155).
 * `stream` is a hipStream_t (NULL = the device's default stream; pass torch's current stream to order
 * launches with torch ops).  Fails with ENODEV when there is no GPU: there is no CPU fallback. */
#define HAVOC_MI355X_NEW_STREAM ((void *)(intptr_t)-1) /* create(): make and own a private non-blocking stream */
int havoc_mi355x_create(havoc_mi355x_ctx **ctx, int device, void *stream);
void havoc_mi355x_destroy(havoc_mi355x_ctx *ctx);
int havoc_mi355x_set_stream(havoc_mi355x_ctx *ctx, void *stream);
int havoc_mi355x_sync(havoc_mi355x_ctx *ctx);
/* the same wait for a caller that queued microseconds of work and needs it now (a table call of libhavoc_classic.so): the stream writes a sequence number into pinned
 * memory behind the queued work and the calling thread POLLS it (bounded: falls back to havoc_mi355x_sync after ~2 ms, and with forked lanes) */
int havoc_mi355x_sync_spin(havoc_mi355x_ctx *ctx);
const char *havoc_mi355x_last_error(void);
const char *havoc_mi355x_version(void);
/* device properties for roofline accounting: [0]=CUs [1]=clock kHz [2]=memory clock kHz [3]=bus width bits
 * [4]=L2 bytes [5]=wavefront size [6]=LDS bytes per workgroup [7]=total global memory MiB */
int havoc_mi355x_device_info(havoc_mi355x_ctx *ctx, int64_t info[8]);

/* plain device-memory helpers so that a C/C++ host (the encoder) needs no HIP headers */
int havoc_mi355x_malloc(havoc_mi355x_ctx *ctx, void **d_ptr, size_t bytes);
int havoc_mi355x_free(havoc_mi355x_ctx *ctx, void *d_ptr);
int havoc_mi355x_h2d(havoc_mi355x_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int havoc_mi355x_d2h(havoc_mi355x_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
/* timing on the context's stream with HIP events (used by bench.py for per-kernel durations) */
int havoc_mi355x_timer_start(havoc_mi355x_ctx *ctx);
int havoc_mi355x_timer_stop_ms(havoc_mi355x_ctx *ctx, float *ms); /* records, synchronises, returns elapsed */

/* pinned host memory the device can address: *h_ptr for the host, *d_ptr for kernels (results a host loop reads right after
 * havoc_mi355x_sync() without a copy); asynchronous and pitched copies on the context's stream */
int havoc_mi355x_host_alloc(havoc_mi355x_ctx *ctx, size_t bytes, void **h_ptr, void **d_ptr);
int havoc_mi355x_host_free(havoc_mi355x_ctx *ctx, void *h_ptr);
int havoc_mi355x_h2d_async(havoc_mi355x_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int havoc_mi355x_d2h_async(havoc_mi355x_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
int havoc_mi355x_copy_2d(havoc_mi355x_ctx *ctx, void *dst, size_t dst_pitch, const void *src, size_t src_pitch, size_t row_bytes, size_t rows,
                         int to_device);

/* HIP-graph capture of a fixed sequence of batch launches (one picture's launches are the same sequence with the same
 * buffers for every CTU row / picture of a size): begin, issue the launches (they are recorded, not run), end, then
 * replay with graph_launch.  Needs a context that owns its stream (HAVOC_MI355X_NEW_STREAM) or an explicit
 * non-default stream: the legacy default stream cannot be captured. */
typedef struct havoc_mi355x_graph havoc_mi355x_graph;
int havoc_mi355x_graph_begin(havoc_mi355x_ctx *ctx);
int havoc_mi355x_graph_end(havoc_mi355x_ctx *ctx, havoc_mi355x_graph **graph);
int havoc_mi355x_graph_launch(havoc_mi355x_ctx *ctx, havoc_mi355x_graph *graph);
void havoc_mi355x_graph_destroy(havoc_mi355x_graph *graph);

/* Fork / join: batches that do not depend on each other (integer ME of one list, sub-pel candidates of another PU
 * class, the intra stage, each transform size ...) are small, latency-bound launches; issued on separate HIP streams
 * they overlap on the 256 CUs.  fork(n) makes n lanes (lane 0 = the context's stream; lanes 1..n-1 are side streams
 * that start after everything already queued), lane(k) selects where the following launches go (launches on one
 * lane stay ordered), join() makes the context's stream wait for every lane.  Works inside graph capture: the graph
 * then holds the parallel branches. */
int havoc_mi355x_fork(havoc_mi355x_ctx *ctx, int nlanes); /* 1..8 */
int havoc_mi355x_lane(havoc_mi355x_ctx *ctx, int lane);
int havoc_mi355x_join(havoc_mi355x_ctx *ctx);

/* ------------------------------------------------------------------------------------------------------- */
/* job descriptors (plain 32-bit little-endian fields, no padding surprises: sizes asserted in the .cpp)    */
/* ------------------------------------------------------------------------------------------------------- */

/* two blocks of w x h samples: SAD(src, ref), SSD(a, b), SATD(a, b), residual(src, pred) */
typedef struct {
    int32_t a_off;   /* src / srcA */
    int32_t b_off;   /* ref / srcB */
    int32_t w, h;
} havoc_mi355x_pair_job; /* 16 bytes */

/* one source block against four candidate reference positions (havoc/sad.h:100) */
typedef struct {
    int32_t src_off;
    int32_t ref_off[4];
    int32_t w, h;
    int32_t reserved;
} havoc_mi355x_sad4_job; /* 32 bytes */

/* one source block against every integer candidate of a (2R+1) x (2R+1) window centred on ref_off */
typedef struct {
    int32_t src_off;
    int32_t ref_off;   /* candidate (dx, dy) = 0: the sample offset of the centre position in the reference plane */
    int32_t w, h;      /* w a multiple of 4 */
    int32_t out_off;   /* index of the surface's first int32 (dx = dy = -R) in d_out */
    int32_t reserved[3];
} havoc_mi355x_surface_job; /* 32 bytes */

/* one block against up to 16 candidate blocks (the 8 half- + 8 quarter-sample candidates of a PU and list) */
typedef struct {
    int32_t a_off;
    int32_t w, h;
    int32_t count;       /* 1..16 candidates used */
    int32_t b_off[16];
} havoc_mi355x_satd_multi_job; /* 80 bytes */

/* fractional-sample interpolation of one prediction block (havoc/pred_inter.h:35) */
typedef struct {
    int32_t dst_off;
    int32_t ref_off;  /* integer-sample position of the block inside the padded reference plane */
    int32_t w, h;
    int32_t xFrac, yFrac; /* quarter (8-tap luma) or eighth (4-tap chroma) sample phase */
    int32_t reserved[2];
} havoc_mi355x_pred_uni_job; /* 32 bytes */

/* bi-prediction from two positions of planes sharing one stride (havoc/pred_inter.h:63) */
typedef struct {
    int32_t dst_off;
    int32_t ref0_off, ref1_off;
    int32_t w, h;
    int32_t xFrac0, yFrac0, xFrac1, yFrac1;
    int32_t reserved[3];
} havoc_mi355x_pred_bi_job; /* 48 bytes */

/* dst = clip(2*src - pred) (havoc/pred_inter.h:87) */
typedef struct {
    int32_t dst_off, pred_off, src_off;
    int32_t w, h;
    int32_t reserved[3];
} havoc_mi355x_subtract_bi_job; /* 32 bytes */

/* one intra prediction block (havoc/pred_intra.h:32-52).  nb_off addresses neighbours[0] = p(0,-1):
 * neighbours[-1] is the corner, [-2 .. -1-2n] the left column top->bottom, [0 .. 2n-1] the top row
 * (havoc/pred_intra.cpp:43-51).  `edge` = (cIdx == 0): the DC / mode-10 / mode-26 edge filters are applied
 * when edge && log2 < 5, as Table::lookup does.  The block size is a launch parameter (the reference's table is
 * indexed by log2TrafoSize); `log2` here is informational and must equal it. */
typedef struct {
    int32_t dst_off;
    int32_t nb_off;
    int32_t log2;    /* 2..5 */
    int32_t mode;    /* 0 planar, 1 DC, 2..34 angular */
    int32_t edge;
    int32_t reserved[3];
} havoc_mi355x_intra_job; /* 32 bytes */

/* one transform unit; size and type are launch parameters (the reference picks one function per
 * (trType, log2TrafoSize), havoc/transform.h:72-84, :128-140).  Unused fields are ignored by each entry point. */
typedef struct {
    int32_t coef_off;  /* n*n contiguous int16 coefficients (index into the coefficient buffer) */
    int32_t res_off;   /* int16 residual block: forward input (row stride = stride_res argument), or n*n
                          contiguous output of inverse_transform / input of quantize_reconstruct */
    int32_t pred_off;  /* prediction samples (inverse+add input) */
    int32_t dst_off;   /* reconstructed samples (inverse+add output); may equal pred_off on the same plane */
} havoc_mi355x_tu_job; /* 16 bytes */

/* one (de)quantisation call over n contiguous int16 values (havoc/quantize.h:42,63) */
typedef struct {
    int32_t dst_off, src_off;
    int32_t n;        /* multiple of 16, as the reference requires */
    int32_t scale, shift, offset; /* offset ignored by the inverse quantiser */
    int32_t reserved[2];
} havoc_mi355x_quant_job; /* 32 bytes */

/* ------------------------------------------------------------------------------------------------------- */
/* picture-level helper next to the path                                                                     */
/* ------------------------------------------------------------------------------------------------------- */

/* Padding::padBlock<Sample> (turing/Padding.h:60-97; all four flags set = Padding::padImage :33-57): replicate the edge
 * samples of the width x height block whose sample (0, 0) sits at d_plane[origin_off] into a border of `pad` samples on
 * the requested sides, in place.  What TaskDeblock.cpp:151-159 does to a reconstructed picture before it is used
 * as a reference (and what the owner runs before the frame-parallel broadcast). */
int havoc_mi355x_pad_block(havoc_mi355x_ctx *ctx, int S, void *d_plane, int64_t origin_off, int width, int height,
                           intptr_t stride, int pad, int top, int bottom, int left, int right);

/* In-loop deblocking of a whole 4:2:0 picture, in place: LoopFilter::Picture::deblock<EDGE_VER> then
 * <EDGE_HOR> (turing/LoopFilter.h:229-400, 739-777) over every 8x8 region, which is what the reference's CTU-by-CTU order
 * (turing/TaskDeblock.cpp:105-127) amounts to.  d_luma / d_cb / d_cr point at sample (0, 0) of each plane.  The boundary
 * strengths and QPs -- the encoder's decisions (LoopFilter.h:480-737) -- come as the two arrays of LoopFilter::Block on its
 * grid of ((width + 63) / 64 * 8 + 1) x ((height + 63) / 64 * 8 + 1) regions: d_block_data[i] = (QpY << 1) | filter-disabled,
 * d_block_bs[i] = 2-bit strengths, bits 0-1 / 2-3 = the region's left edge rows 0-3 / 4-7, bits 4-5 / 6-7 = its top edge
 * columns 0-3 / 4-7 (chroma uses the first of each pair, as the reference does).  One slice: the offsets are per picture.
 * A picture may be filtered in horizontal bands, top to bottom, one call per band: the plane pointers at the band's first row, height =
 * the band's rows, d_block_data / d_block_bs advanced by (first row / 8) grid rows, width unchanged.  A band must start on a multiple of
 * 16 luma rows (the chroma horizontal edges are found from the band-local row index), and a call whose first grid row carries top-edge
 * strengths reads four sample rows (two chroma rows) and one grid row of d_block_data above what it was given and rewrites up to three
 * (one) of those sample rows: the bands together leave what one call on the whole picture leaves. */
int havoc_mi355x_deblock(havoc_mi355x_ctx *ctx, int S, int bitDepth, void *d_luma, intptr_t stride_luma, void *d_cb, void *d_cr, intptr_t stride_chroma,
                         int width, int height, const int8_t *d_block_data, const uint8_t *d_block_bs, int tc_offset_div2, int beta_offset_div2,
                         int cb_qp_offset, int cr_qp_offset);

/* The boundary strengths and QP bytes havoc_mi355x_deblock reads, DERIVED on the device from the picture's block structure
 * (LoopFilter::Picture::processCu / processPu / processTu / processRc, turing/LoopFilter.h:541-737, and sameMotion, :402-422) -- the
 * encoder's decisions as a map of 4x4 luma cells, which is what a device-side encoder holds after mode decision:
 *   a transform block edge on the 8-sample grid gets strength 2 where the block on either side is intra, 1 where either side is an
 *   inter block with coded luma coefficients; the left / top edge of an inter prediction unit gets 1 where the motion across it differs
 *   (different pictures, or a vector component 4 or more quarter samples apart, lists matched either way round); the maximum stands.
 * A cell outside the picture counts as "no motion" (what the reference's unavailable neighbour is); edges on the picture's left and top
 * boundary end with strength 0 (processCtu, LoopFilter.h:484-510, runs after the CTU's units; one slice per picture).  PCM units are not modelled (the
 * reference's encoder never emits them).  Writes the whole grid of ((width + 63) / 64 * 8 + 1) x ((height + 63) / 64 * 8 + 1) regions. */
typedef struct {
    int16_t mv[2][2];     /* [list][x, y], quarter samples */
    int8_t dpb_index[2];  /* which decoded picture each list predicts from; -1 = list unused (both -1: intra / no motion) */
    uint8_t flags;        /* HAVOC_CELL_* */
    int8_t qp_y;
    uint8_t tu_log2;      /* log2 size of the luma transform block holding the cell (2..5) */
    uint8_t reserved[3];
} havoc_mi355x_cell; /* 16 bytes */
enum {
    HAVOC_CELL_INTRA = 1,      /* CuPredMode == MODE_INTRA */
    HAVOC_CELL_CODED = 2,      /* cbf_luma of its transform block */
    HAVOC_CELL_NO_FILTER = 4,  /* cu_transquant_bypass_flag (Block::packData's disable bit) */
    HAVOC_CELL_PU_LEFT = 8,    /* the cell lies on the left edge of its prediction unit */
    HAVOC_CELL_PU_TOP = 16     /* ... on its top edge */
};
int havoc_mi355x_derive_bs(havoc_mi355x_ctx *ctx, const havoc_mi355x_cell *d_cells, intptr_t cells_stride, int width, int height, int8_t *d_block_data,
                           uint8_t *d_block_bs);

/* Device-side picture store + input upload.  A picture = the three planes of Picture<Sample>
 * (turing/Picture.cpp:91-125) in ONE HBM allocation: per plane `pad` samples of border (chroma: pad / 2), row stride rounded
 * up to `alignment` bytes (the reference: pad 96, alignment 32, turing/StatePictures.h:155-156; this library's kernels are
 * indifferent, 64 keeps rows on 64-byte boundaries).  4:2:0 only, as every configuration of BASELINE.json. */
typedef struct havoc_mi355x_picture havoc_mi355x_picture;
int havoc_mi355x_picture_create(havoc_mi355x_ctx *ctx, int S, int bit_depth, int width, int height, int pad, int alignment,
                                havoc_mi355x_picture **pic);
void havoc_mi355x_picture_destroy(havoc_mi355x_ctx *ctx, havoc_mi355x_picture *pic);
/* plane geometry: *d_base = the picture's allocation (one for the three planes), *origin_off = sample offset of sample (0, 0)
 * of plane cIdx from d_base (what a job's offsets are relative to), *stride in samples; any out pointer may be NULL */
int havoc_mi355x_picture_plane(havoc_mi355x_picture *pic, int cIdx, void **d_base, int64_t *origin_off, intptr_t *stride, int *width, int *height,
                               int *pad);
/* one input frame as the reference reads it (turing/encode.cpp:600-640): planar Y, U, V, tightly packed, src_S bytes per sample
 * (16-bit: little-endian words); stored << shift (encode.cpp:397: 8-bit input on the 16-bit path, shift 2); pad_after != 0
 * replicates the borders afterwards (Padding::padImage, turing/Padding.h:33-57) */
int havoc_mi355x_picture_upload_yuv(havoc_mi355x_ctx *ctx, havoc_mi355x_picture *pic, const void *h_yuv, int src_S, int shift, int pad_after);
/* one plane from / to a host Picture plane: h_origin = its sample (0, 0), h_stride in samples; with_padding != 0 moves the
 * `pad` border as well (the host plane must have one at least as wide).  download synchronises. */
int havoc_mi355x_picture_upload_plane(havoc_mi355x_ctx *ctx, havoc_mi355x_picture *pic, int cIdx, const void *h_origin, intptr_t h_stride,
                                      int with_padding);
int havoc_mi355x_picture_download_plane(havoc_mi355x_ctx *ctx, havoc_mi355x_picture *pic, int cIdx, void *h_origin, intptr_t h_stride,
                                        int with_padding);
int havoc_mi355x_picture_pad(havoc_mi355x_ctx *ctx, havoc_mi355x_picture *pic);
/* the 16 fractional-sample luma planes of the picture (havoc_mi355x_interp_planes; slot 0 = the luma plane), made on first
 * request after the picture changed and kept with it.  Phase k, sample (x, y):
 *   d_planes[k * plane_elems + (luma origin_off - *luma_first) + y * stride + x]   (luma plane's origin_off / stride). */
int havoc_mi355x_picture_phase_planes(havoc_mi355x_ctx *ctx, havoc_mi355x_picture *pic, void **d_planes, intptr_t *plane_elems, int64_t *luma_first);

/* ------------------------------------------------------------------------------------------------------- */
/* distortion metrics                                                                                        */
/* ------------------------------------------------------------------------------------------------------- */

/* havoc_sad<Sample> (havoc/sad.h:58, C reference havoc/sad.cpp:432-449): d_out[i] = SAD, 16-bit >> 2 */
int havoc_mi355x_sad(havoc_mi355x_ctx *ctx, int S, const void *d_src, intptr_t stride_src, const void *d_ref,
                     intptr_t stride_ref, const havoc_mi355x_pair_job *d_jobs, int njobs, int32_t *d_out);
/* havoc_sad_multiref<Sample>, ways = 4 (havoc/sad.h:100, havoc/sad.cpp:513-542): d_out[4*i + k] */
int havoc_mi355x_sad4(havoc_mi355x_ctx *ctx, int S, const void *d_src, intptr_t stride_src, const void *d_ref,
                      intptr_t stride_ref, const havoc_mi355x_sad4_job *d_jobs, int njobs, int32_t *d_out);
/* The same calls BY RUNS: a run = consecutive havoc_sad_multiref calls of one motion search (turing/Search.hpp:2224-2297 -> considerPattern :1447-1482: ~112 calls
 * sharing the source block and moving around one centre).  A workgroup stages the run's source block and the bounding box of all its candidates in LDS once and the
 * calls read them there; d_out as havoc_mi355x_sad4.  d_runs must tile the jobs the caller wants computed: the d_out entries of a job in no run are LEFT AS THEY ARE
 * (clear d_out first if that matters), and runs must not overlap (two workgroups would write the same entries).  havoc_mi355x_sad4_make_runs' output tiles [0, njobs).  Runs change the speed,
 * never a result: a run whose calls differ in source / size, whose box does not fit LDS or does not hold every candidate, is computed call by call.
 *   box_off / box_w / box_h: the rectangle of the reference plane (sample offset of its top-left from d_ref, width in samples, rows) that holds every candidate BLOCK of
 *   the run -- staged at once, each candidate then checked against it; box_w = 0: the kernel finds the box itself (one more pass over the run's jobs).
 * havoc_mi355x_sad4_make_runs (host code, no device) cuts a HOST copy of a job table into runs and gives them their boxes: consecutive jobs with equal src_off, w, h whose
 * box fits the kernel's window (16 KB x S), at most max_run calls (1 .. 128; <= 0: by block size -- 16 calls of a 64x64 block, 48 of a 32x32, 128 below: what keeps a
 * workgroup's work even, profiles/r05/sad4_run_policy.txt); stride_ref = the reference plane's row stride in samples (the boxes are rectangles of that plane).
 * Returns the number of runs written to `runs` (capacity njobs), or -1. */
typedef struct {
    int32_t first_job;
    int32_t count;
    int32_t box_off, box_w, box_h;
    int32_t reserved[3];
} havoc_mi355x_sad4_run; /* 32 bytes */
int havoc_mi355x_sad4_runs(havoc_mi355x_ctx *ctx, int S, const void *d_src, intptr_t stride_src, const void *d_ref,
                           intptr_t stride_ref, const havoc_mi355x_sad4_job *d_jobs, int njobs,
                           const havoc_mi355x_sad4_run *d_runs, int nruns, int32_t *d_out);
int havoc_mi355x_sad4_make_runs(const havoc_mi355x_sad4_job *jobs, int njobs, int max_run, intptr_t stride_ref, int S, havoc_mi355x_sad4_run *runs);
/* Full-pel SAD surface: the super-set serving the havoc_sad / havoc_sad_multiref calls of the integer motion search
 * (turing/Search.hpp:1447-1482 considerPattern, :1585-1623 bi grid, :2224-2290 star / raster / refinement) as look-ups.
 * d_out[out_off + (dy + range) * (2*range + 1) + (dx + range)] = havoc_sad(src, ref + dy*stride_ref + dx) for every
 * dx, dy in [-range, range], range 0..96 (the reference pads its pictures by 96 samples); every value is the one havoc_mi355x_sad returns for that candidate.
 * max_w / max_h: upper bounds on the block sizes of the batch.  Reads at most 3 bytes beyond a candidate row. */
int havoc_mi355x_sad_surface(havoc_mi355x_ctx *ctx, int S, int range, int max_w, int max_h, const void *d_src,
                             intptr_t stride_src, const void *d_ref, intptr_t stride_ref,
                             const havoc_mi355x_surface_job *d_jobs, int njobs, int32_t *d_out);
/* havoc_ssd<Sample> (havoc/ssd.h:33, havoc/ssd.cpp:28-43): uint32 accumulate, 16-bit >> 4 */
int havoc_mi355x_ssd(havoc_mi355x_ctx *ctx, int S, const void *d_a, intptr_t stride_a, const void *d_b,
                     intptr_t stride_b, const havoc_mi355x_pair_job *d_jobs, int njobs, uint32_t *d_out);
/* havoc_hadamard_satd<Sample> tiled over a w x h block exactly as measureSatd does (turing/Measure.h:97-135;
 * one 2x2 / 4x4 / 8x8 Hadamard = havoc/hadamard.cpp:58-98 when w == h == n).  max_w / max_h: upper bounds on the
 * block sizes of this batch (64, 64 always valid): they choose how many lanes share a job. */
int havoc_mi355x_satd(havoc_mi355x_ctx *ctx, int S, int max_w, int max_h, const void *d_a, intptr_t stride_a, const void *d_b,
                      intptr_t stride_b, const havoc_mi355x_pair_job *d_jobs, int njobs, int32_t *d_out);
/* The same measure for one block `a` against `count` candidate blocks `b` (costDistortionMv's candidates of one PU,
 * turing/Search.hpp:1965-1998): d_out[16*i + k], k < count, each equal to what havoc_mi355x_satd returns for that pair.
 * A count outside 1..16 is clamped: with count <= 0 nothing is written for the job, a count above 16 acts as 16; the
 * entries d_out[16*i + k], k >= count, are never written, and the b_off slots past count must still hold offsets inside d_b. */
int havoc_mi355x_satd_multi(havoc_mi355x_ctx *ctx, int S, int max_w, int max_h, const void *d_a, intptr_t stride_a,
                            const void *d_b, intptr_t stride_b, const havoc_mi355x_satd_multi_job *d_jobs, int njobs,
                            int32_t *d_out);
/* havoc_ssd_linear (havoc/diff.h:35, havoc/diff.cpp:29-39): one linear 8-bit run, *d_out = int32 sum */
int havoc_mi355x_ssd_linear(havoc_mi355x_ctx *ctx, const uint8_t *d_a, const uint8_t *d_b, int size, int32_t *d_out);

/* ------------------------------------------------------------------------------------------------------- */
/* inter prediction                                                                                          */
/* ------------------------------------------------------------------------------------------------------- */

/* HavocPredUni<Sample> (havoc/pred_inter.h:35, C reference havoc/pred_inter.cpp:76-202); taps = 8 | 4.
 * Writes exactly w x h samples per job (the JIT's licence to over-write to the right is not used).  max_w / max_h:
 * upper bounds on the block sizes of this batch -- the reference's table is indexed by width class
 * (havoc/pred_inter.h:47-50); 64, 64 is always valid.  Every job reads the full (w+taps-1) x (h+taps-1) window
 * around its block whatever the phase (the zero phase is evaluated with the {..,64,..} filter). */
int havoc_mi355x_pred_uni(havoc_mi355x_ctx *ctx, int S, int taps, int bitDepth, int max_w, int max_h, void *d_dst, intptr_t stride_dst,
                          const void *d_ref, intptr_t stride_ref, const havoc_mi355x_pred_uni_job *d_jobs, int njobs);
/* HavocPredBi<Sample> (havoc/pred_inter.h:63, havoc/pred_inter.cpp:1207-1252) */
int havoc_mi355x_pred_bi(havoc_mi355x_ctx *ctx, int S, int taps, int bitDepth, int max_w, int max_h, void *d_dst, intptr_t stride_dst,
                         const void *d_ref, intptr_t stride_ref, const havoc_mi355x_pred_bi_job *d_jobs, int njobs);
/* The same two primitives for a job table that holds ALL size classes, in ONE launch: the table is sorted by class -- count[0] jobs whose
 * larger side is <= 8, then count[1] jobs <= 16, count[2] <= 32, count[3] <= 64 -- the width class being a property of the job, as the
 * reference's havocGetPredUni / havocGetPredBi index it (havoc/pred_inter.h:47-50, 72-76).  Results identical to the per-class launches. */
int havoc_mi355x_pred_uni_classes(havoc_mi355x_ctx *ctx, int S, int taps, int bitDepth, void *d_dst, intptr_t stride_dst, const void *d_ref,
                                  intptr_t stride_ref, const havoc_mi355x_pred_uni_job *d_jobs, const int32_t count[4]);
int havoc_mi355x_pred_bi_classes(havoc_mi355x_ctx *ctx, int S, int taps, int bitDepth, void *d_dst, intptr_t stride_dst, const void *d_ref,
                                 intptr_t stride_ref, const havoc_mi355x_pred_bi_job *d_jobs, const int32_t count[4]);
/* havoc::SubtractBi<Sample> (havoc/pred_inter.h:87, havoc/pred_inter.cpp:2063-2080) */
int havoc_mi355x_subtract_bi(havoc_mi355x_ctx *ctx, int S, int bitDepth, void *d_dst, intptr_t stride_dst,
                             const void *d_pred, intptr_t stride_pred, const void *d_src, intptr_t stride_src,
                             const havoc_mi355x_subtract_bi_job *d_jobs, int njobs);

/* The 15 fractional-sample luma planes of a reference picture, computed once per picture: for every (xFrac, yFrac)
 * in 0..3 x 0..3 except (0,0) and every sample (x, y) of the rectangle [x0, x0+width) x [y0, y0+height) of the
 * padded picture,   d_planes[(4*yFrac + xFrac) * plane_elems + y*stride + x] = the sample HavocPredUni (8-tap,
 * havoc/pred_inter.cpp:113-202) produces at (x, y) for that phase.  A sub-pel candidate's prediction block is then a
 * block of one plane and its cost a plain havoc_mi355x_satd job against it (plane 0 is not written: use d_ref).
 * The rectangle must leave >= 4 rows and >= 12 samples of the allocation around it (the picture padding does). */
int havoc_mi355x_interp_planes(havoc_mi355x_ctx *ctx, int S, int bitDepth, void *d_planes, intptr_t plane_elems, const void *d_ref,
                               intptr_t stride, int x0, int y0, int width, int height);

/* One sub-pel motion candidate, fused: HavocPredUni of the PU at (ref_off, xFrac, yFrac) followed by measureSatd
 * against the source PU -- costDistortionMv (turing/Search.hpp:1965-1998 -> havoc/pred_inter.cpp:113-202 +
 * turing/Measure.h:97-135).  Jobs are havoc_mi355x_pred_uni_job with `dst_off` naming the SOURCE block in d_src;
 * d_cost[i] = the PU SATD (8x8 / 4x4 / 2x2 tiles by PU shape); the prediction is not written.  max_w / max_h are
 * upper bounds on the PU sizes in this batch (the reference's table is indexed by width class,
 * havoc/pred_inter.h:47-50); 64, 64 is always valid, tighter bounds pick a kernel with less LDS per PU. */
int havoc_mi355x_subpel_satd(havoc_mi355x_ctx *ctx, int S, int taps, int bitDepth, int max_w, int max_h, const void *d_src,
                             intptr_t stride_src, const void *d_ref, intptr_t stride_ref, const havoc_mi355x_pred_uni_job *d_jobs,
                             int njobs, int32_t *d_cost);

/* ------------------------------------------------------------------------------------------------------- */
/* intra prediction                                                                                          */
/* ------------------------------------------------------------------------------------------------------- */

/* havoc::intra::Function<Sample> via Table::lookup (havoc/pred_intra.h:32-52, pred_intra.cpp:20282-20401) */
int havoc_mi355x_intra(havoc_mi355x_ctx *ctx, int S, int bitDepth, int log2TrafoSize, void *d_dst, intptr_t stride_dst,
                       const void *d_neighbours, const havoc_mi355x_intra_job *d_jobs, int njobs);

/* The 35-mode luma SATD stage of one intra partition, fused: for every mode m = 0..34 the prediction
 * (havoc/pred_intra.cpp:20282-20401, from the filtered neighbour array when bit m of filt_lo/filt_hi is set, else the
 * unfiltered one -- the caller's filterFlag, turing/Reconstruct.cpp:659) is measured against the source block with
 * the Hadamard SATD (8x8 tiles; one 4x4 for 4x4 blocks) exactly as PredictIntraLumaBlock does
 * (turing/Reconstruct.cpp:630-701) inside the mode loop of searchIntraPartition (turing/Search.hpp:113-142).
 * d_cost[35*i + m] = SATD; no prediction is written to memory. */
typedef struct {
    int32_t src_off;   /* top-left of the source block in d_src */
    int32_t nb_off;    /* unfiltered neighbours[0] (same layout as havoc_mi355x_intra_job) in d_neighbours */
    int32_t nbf_off;   /* filtered neighbours[0] */
    uint32_t filt_lo;  /* bit m: mode m (0..31) predicts from the filtered array */
    uint32_t filt_hi;  /* bits 0..2: modes 32..34 */
    int32_t edge;      /* cIdx == 0 (edge filters apply when log2TrafoSize < 5) */
    int32_t reserved[2];
} havoc_mi355x_intra_search_job; /* 32 bytes */
int havoc_mi355x_intra_satd35(havoc_mi355x_ctx *ctx, int S, int bitDepth, int log2TrafoSize, const void *d_src, intptr_t stride_src,
                              const void *d_neighbours, const havoc_mi355x_intra_search_job *d_jobs, int njobs, int32_t *d_cost);

/* ------------------------------------------------------------------------------------------------------- */
/* residual, transforms, quantisation                                                                        */
/* ------------------------------------------------------------------------------------------------------- */

/* res = src - pred, int16 (turing/Reconstruct.cpp:258-260, 1274-1286).  job: a = src, b = pred;
 * the residual of job i is written at d_res + res_off[i] with row stride stride_res. */
int havoc_mi355x_residual(havoc_mi355x_ctx *ctx, int S, int16_t *d_res, intptr_t stride_res, const int32_t *d_res_off,
                          const void *d_src, intptr_t stride_src, const void *d_pred, intptr_t stride_pred,
                          const havoc_mi355x_pair_job *d_jobs, int njobs);
/* havoc::Transform via get_transform<bitDepth> (havoc/transform.h:117-140, transform.cpp:3087-3397) */
int havoc_mi355x_transform(havoc_mi355x_ctx *ctx, int bitDepth, int trType, int log2TrafoSize, int16_t *d_coeffs,
                           const int16_t *d_res, intptr_t stride_res, const havoc_mi355x_tu_job *d_jobs, int njobs);
/* havoc::inverse_transform (havoc/transform.h:33-57, transform.cpp:339-355): d_res n*n contiguous at res_off */
int havoc_mi355x_inverse_transform(havoc_mi355x_ctx *ctx, int bitDepth, int trType, int log2TrafoSize, int16_t *d_res,
                                   const int16_t *d_coeffs, const havoc_mi355x_tu_job *d_jobs, int njobs);
/* havoc::inverse_transform_add<Sample> (havoc/transform.h:61-84, transform.cpp:358-401); d_pred may be d_dst */
int havoc_mi355x_inverse_transform_add(havoc_mi355x_ctx *ctx, int S, int bitDepth, int trType, int log2TrafoSize,
                                       void *d_dst, intptr_t stride_dst, const void *d_pred, intptr_t stride_pred,
                                       const int16_t *d_coeffs, const havoc_mi355x_tu_job *d_jobs, int njobs);
/* The TU chain of the reference's reconstruction, fused on either side of the host's quantiser decision (at
 * speed=medium RDOQ, which is not havoc, runs between the two; turing/Reconstruct.cpp:258-353 and :766-856):
 *   tu_forward     : residual = src - pred (Reconstruct.cpp:258-260), then havoc::Transform -> d_coeffs[coef_off ..]
 *   tu_reconstruct : havoc_quantize_inverse(levels, scale, shift), then havoc::inverse_transform_add onto the
 *                    prediction -> d_rec[rec_off ..] (row stride stride_rec), then havoc_ssd(src, rec) -> d_ssd[i].
 * Residual and de-quantised coefficients are never written.  Bit-identical to calling the separate entry points. */
typedef struct {
    int32_t coef_off;  /* n*n contiguous int16: coefficients (forward) / levels (reconstruct) */
    int32_t src_off;   /* source block in d_src */
    int32_t pred_off;  /* prediction block in d_pred */
    int32_t rec_off;   /* reconstructed block in d_rec (may be the prediction's own location) */
} havoc_mi355x_tu_fused_job; /* 16 bytes */
int havoc_mi355x_tu_forward(havoc_mi355x_ctx *ctx, int S, int bitDepth, int trType, int log2TrafoSize, int16_t *d_coeffs, const void *d_src,
                            intptr_t stride_src, const void *d_pred, intptr_t stride_pred, const havoc_mi355x_tu_fused_job *d_jobs, int njobs);
/* The 35-mode stage of ONE intra partition in one launch (round 6; what libhavoc_classic.so's serve layer precomputes when a partition's first prediction / SATD /
 * transform call arrives -- turing/Search.hpp:113-142, Reconstruct.cpp:244-353): job i = mode slot i, its prediction block (pred_off, row stride stride_pred) against
 * the partition's source block (src_off); coef_off / rec_off = where its n*n coefficients / reconstructed samples (n x n, contiguous) go.  Per job, each bit-identical to
 * the entry point named:
 *   d_satd[i * tiles + t]    havoc_mi355x_satd of tile t (8x8 tiles in raster order; one 4x4 tile for a 4x4 partition), only if with_satd
 *   d_coeffs                 havoc_mi355x_tu_forward, DST-VII for 4x4 / DCT above (the luma rule, Reconstruct.cpp:263)
 *   d_coeffs_dct             4x4 only: havoc_mi355x_tu_forward with trType 0 (a 4x4 chroma block)
 *   d_rec0, d_ssd0[i]        havoc_mi355x_tu_reconstruct on a block of ZERO levels: the reconstruction (= the clipped prediction) and its SSD against the source */
int havoc_mi355x_intra_measure(havoc_mi355x_ctx *ctx, int S, int bitDepth, int log2TrafoSize, int16_t *d_coeffs, int16_t *d_coeffs_dct, int32_t *d_satd, void *d_rec0,
                               uint32_t *d_ssd0, const void *d_src, intptr_t stride_src, const void *d_pred, intptr_t stride_pred, const havoc_mi355x_tu_fused_job *d_jobs,
                               int njobs, int with_satd);
int havoc_mi355x_tu_reconstruct(havoc_mi355x_ctx *ctx, int S, int bitDepth, int trType, int log2TrafoSize, int scale, int shift, void *d_rec,
                                intptr_t stride_rec, const void *d_pred, intptr_t stride_pred, const void *d_src, intptr_t stride_src,
                                const int16_t *d_levels, const havoc_mi355x_tu_fused_job *d_jobs, int njobs, uint32_t *d_ssd);

/* What a rate estimate reads of a block of quantised levels, without the levels crossing the link: d_out[2 * i] = number of non-zero
 * levels, d_out[2 * i + 1] = sum of |level| of the block d_jobs[2 * i] (int16 offset, multiple of 2) of d_jobs[2 * i + 1] values (multiple
 * of 2).  Not a reference primitive: the reference's EstimateRate<residual_coding> (turing/EstimateRate.h) walks the levels on the host; a
 * batch client that chooses between transform-tree candidates (libhavoc_search.so: havoc_search_rqt) reads these instead. */
int havoc_mi355x_level_stats(havoc_mi355x_ctx *ctx, const int16_t *d_levels, const int32_t *d_jobs, int njobs, int32_t *d_out);

/* havoc_quantize (havoc/quantize.h:63, quantize.cpp:278-304): d_cbf[i] = OR of the job's outputs */
int havoc_mi355x_quantize(havoc_mi355x_ctx *ctx, int16_t *d_dst, const int16_t *d_src,
                          const havoc_mi355x_quant_job *d_jobs, int njobs, int32_t *d_cbf);
/* havoc_quantize_inverse (havoc/quantize.h:42, quantize.cpp:37-46) */
int havoc_mi355x_quantize_inverse(havoc_mi355x_ctx *ctx, int16_t *d_dst, const int16_t *d_src,
                                  const havoc_mi355x_quant_job *d_jobs, int njobs);
/* havoc_quantize_reconstruct (havoc/quantize.h:84, quantize.cpp:538-549), 8-bit only:
 * rec = clip8(pred + res); job: dst_off = rec, pred_off, res_off (n*n contiguous) */
int havoc_mi355x_quantize_reconstruct(havoc_mi355x_ctx *ctx, int log2TrafoSize, uint8_t *d_rec, intptr_t stride_rec,
                                      const uint8_t *d_pred, intptr_t stride_pred, const int16_t *d_res,
                                      const havoc_mi355x_tu_job *d_jobs, int njobs);

/* ------------------------------------------------------------------------------------------------------- */
/* sample-adaptive offset primitives                                                      */
/* ------------------------------------------------------------------------------------------------------- */
/* The statistics the encoder's SAO decision reads (turing/EncSao.h:111-283: edge_offset_stats_class0..3, band_offset_luma_stats)
 * over one block (a CTU of one colour component; the joint band statistics of Cb and Cr, EncSao.h:62-109: havoc_mi355x_sao_band_chroma).
 * d_out: 105 int64 per job -- for edge class c = 0..3 the sums of (original - reconstruction) per category at [10c .. 10c+4] and the
 * sample counts at [10c+5 .. 10c+9]; the sums per band at [40..71], the counts per band at [72..103]; [104] = the band position the
 * reference's function returns.  The block's outermost ring of samples is not counted, as in the reference (w, h >= 3). */
typedef struct {
    int32_t src_off, rec_off; /* the block in the original / reconstructed plane */
    int32_t w, h;
} havoc_mi355x_sao_stats_job; /* 16 bytes */
int havoc_mi355x_sao_stats(havoc_mi355x_ctx *ctx, int S, int bitDepth, const void *d_src, intptr_t stride_src, const void *d_rec, intptr_t stride_rec,
                           const havoc_mi355x_sao_stats_job *d_jobs, int njobs, int64_t *d_out);
/* band_offset_chroma_stats (turing/EncSao.h:62-109): the band statistics of the Cb and the Cr block of a CTU TOGETHER -- one histogram over
 * both interiors -- as the encoder's chroma SAO decision reads them.  d_src / d_rec: the planes holding both chroma components (offsets in
 * samples; one stride each).  d_out[65 * i]: E[32], count[32], the band position the reference's function returns. */
typedef struct {
    int32_t src_u, src_v;   /* the CTU's Cb / Cr block in the source chroma */
    int32_t rec_u, rec_v;   /* ... in the deblocked reconstruction */
    int32_t w, h;
    int32_t reserved[2];
} havoc_mi355x_sao_chroma_job; /* 32 bytes */
int havoc_mi355x_sao_band_chroma(havoc_mi355x_ctx *ctx, int S, int bitDepth, const void *d_src, intptr_t stride_src, const void *d_rec, intptr_t stride_rec,
                                 const havoc_mi355x_sao_chroma_job *d_jobs, int njobs, int64_t *d_out);
/* sao_filter_band / sao_filter_edge (turing/sao.h, sao.cpp:33-92) on one block: d_dst and d_src are different pictures; the edge
 * filter reads one sample beyond the block on every side.  type 0 copies (SAO off for the block), 1 = band offset with
 * offsets[] = the 32-entry table LoopFilter.h:994-1004 builds, 2 = edge offset with offsets[0..4] = SaoOffsetVal. */
typedef struct {
    int32_t dst_off, src_off, w, h;
    int32_t type, eo_class;
    int16_t offsets[32];
    int32_t reserved[2];
} havoc_mi355x_sao_job; /* 96 bytes */
int havoc_mi355x_sao_filter(havoc_mi355x_ctx *ctx, int S, int bitDepth, void *d_dst, intptr_t stride_dst, const void *d_src, intptr_t stride_src,
                            const havoc_mi355x_sao_job *d_jobs, int njobs);

/* The SAO parameters of a picture's CTUs and their distortion: EncSao::saoRdEstimateLuma / saoRdEstimateChroma (turing/EncSao.h:286-797)
 * and EncSao::computeSaoDistortion (EncSao.h:800-947), in one call on the context's stream (no host synchronisation, no allocation:
 * capturable into a graph).  Per CTU:
 *   1. statistics -- havoc_mi355x_sao_stats on Y, on Cb and on Cr (summed per class and category, EncSao.h:586-587), the joint
 *      chroma band histogram of havoc_mi355x_sao_band_chroma;
 *   2. estimation -- luma and chroma each decided over off, edge classes 0..3 and band positions startBand..0 exactly as the
 *      reference's sequential loop: double arithmetic without fused multiply-add, strict `<` (the first candidate wins a tie), the
 *      search starting from a cost of 0.0 (a type is chosen only below 0), a type whose four offsets are all 0 is off.  The reference's
 *      quirks are kept: roundSao by bit depth (EncSao.h:42-48), the vertical class rounding an INTEGER quotient (EncSao.h:369),
 *      estSaoDist shifting the magnitude (EncSao.h:49-59), the offset limit (1 << (min(bitDepth, 10) - 5)) - 1, band offsets
 *      estimated from bands bandPosition .. bandPosition + 3 where startBand is one past the densest four-band window (EncSao.h:106,
 *      :485).  One difference: at band position 29 the reference reads one element past its int64[32] band arrays (EncSao.h:485,
 *      :749, band 32); here band 32 is empty.  bitDepth is both BitDepthY and BitDepthC (the chroma edge clamp's else-branch reads
 *      BitDepthY, EncSao.h:590; the chroma filters get BitDepthY, EncSao.h:921-929).
 *   3. apply and measure -- the CTU's Y, Cb, Cr filtered with the estimated parameters into d_dst_* (LoopFilter.h:134-160
 *      SaoOffsetVal; the band table of EncSao.h:866-877, whose four entries wrap at band 31; a component that is off is copied),
 *      and EncSao::ssd against the source: uint32 accumulation that wraps, >> 4 for 16-bit samples whatever the bit depth.
 * lambda: reciprocal_lambda_q16 is the encoder's reciprocal lambda, FixedPoint<int32_t, 16> (turing/Cost.h:34, Measure.h:44), > 0;
 * the search uses 1 / (reciprocal_lambda_q16 / 65536.0).  flags: bit 0 = slice_sao_luma_flag, bit 1 = slice_sao_chroma_flag; a
 * disabled component is type 0.  Pictures are 4:2:0: a luma plane and one chroma plane holding Cb and Cr (offsets in samples, one
 * stride per plane and picture).  The edge filter reads one sample beyond the CTU on every side, from the reconstruction: every
 * plane needs that margin around the picture.  d_dst_* must differ from d_rec_*.  A CTU record whose w or h is odd or outside
 * 8..64 gets an all-zero parameter record and nothing of it is written.
 * d_work: havoc_mi355x_sao_workspace(nctus) bytes of device scratch, 16-byte aligned, private to the call until it completes. */
typedef struct {
    int32_t src_y, src_cb, src_cr;   /* the CTU's Y / Cb / Cr block in the source planes */
    int32_t rec_y, rec_cb, rec_cr;   /* ... in the (deblocked) reconstruction */
    int32_t dst_y, dst_cb, dst_cr;   /* ... in the destination */
    int32_t w, h;                    /* luma size clipped to the picture, even, 8..64; chroma is (w / 2) x (h / 2) */
    int32_t reserved;
    /* where the chroma statistics are read (source, reconstruction): the CTU's own blocks (= src_cb .. rec_cr), or, to reproduce the
     * reference bit for bit, where saoRdEstimateChroma reads them: EncSao.h:534-546 passes chroma coordinates to ThreePlanes::operator()
     * (Picture.h:179-187), which halves them again -- the block at (x / 4, y / 4) of the chroma planes. */
    int32_t stat_src_cb, stat_src_cr, stat_rec_cb, stat_rec_cr;
} havoc_mi355x_sao_ctu; /* 64 bytes */
typedef struct {
    int32_t type;                    /* SaoTypeIdx: 0 off, 1 band offset, 2 edge offset */
    int32_t eo_class;                /* SaoEoClass when type 2, else 0 */
    int32_t band_position;           /* sao_band_position when type 1, else 0 */
    int32_t offset_abs[4];           /* sao_offset_abs (EncSao.h:519-524) */
    int32_t offset_sign[4];          /* sao_offset_sign when type 1, else 0 */
} havoc_mi355x_sao_component; /* 44 bytes */
typedef struct {
    havoc_mi355x_sao_component comp[2];   /* [0] luma, [1] chroma (Cb and Cr share type, class, band and offsets) */
    int32_t dist_sao;                /* computeSaoDistortion with these parameters: ssd_sao[0] + 4 ssd_sao[1] + 4 ssd_sao[2] (mod 2^32) */
    int32_t dist_off;                /* ... with both types 0 */
    uint32_t ssd_sao[3], ssd_off[3]; /* EncSao::ssd per plane Y, Cb, Cr (unscaled): source vs destination / vs reconstruction */
    int32_t reserved[2];
} havoc_mi355x_sao_params; /* 128 bytes */
size_t havoc_mi355x_sao_workspace(int nctus);
int havoc_mi355x_sao_estimate(havoc_mi355x_ctx *ctx, int S, int bitDepth, int32_t reciprocal_lambda_q16, int flags,
                              const void *d_src_y, const void *d_src_c, intptr_t stride_src_y, intptr_t stride_src_c,
                              const void *d_rec_y, const void *d_rec_c, intptr_t stride_rec_y, intptr_t stride_rec_c,
                              void *d_dst_y, void *d_dst_c, intptr_t stride_dst_y, intptr_t stride_dst_c,
                              const havoc_mi355x_sao_ctu *d_ctus, int nctus, void *d_work, size_t work_bytes, havoc_mi355x_sao_params *d_params);

/* The final SAO parameters of a picture's CTUs: the last step of EncSao::rdSao (turing/EncSao.h:1017-1120), in one call on the context's
 * stream (no host synchronisation, no allocation: capturable into a graph).  Per CTU in raster order, four candidates priced as
 * rate + distortion x reciprocal_lambda_q16 (Cost = FixedPoint<int64_t, 16>; a context-coded bin costs measureEncodeDecision,
 * Write.h:476-492, a bypass bin 1 << 16): the estimate of havoc_mi355x_sao_estimate (dist_sao), all off (dist_off; tried only when
 * the luma or chroma estimate is not type 0), merge-up (when ry > 0) and merge-left (when rx > 0), each merge with the neighbour's
 * FINAL parameters.  A later candidate wins only with a strictly lower cost.  The rates are Search<sao>::go's (Search.hpp:641-705):
 * merge-up codes sao_merge_left_flag = 0 first when rx > 0; sao_offset_abs is truncated unary with cMax = (1 << (min(bitDepth, 10) - 5)) - 1;
 * the second bin of sao_type_idx, the signs, the band position (5 bins) and the edge class (2 bins) are bypass; Cr is not priced
 * at all (the reference's rate under-counts it).  After the choice the two contexts move with the bins the encoder writes.
 *   Inputs: the planes, strides and CTU table given to havoc_mi355x_sao_estimate (raster order, ctus_x CTUs per row, nctus / ctus_x
 * rows, 1 <= ctus_x <= 512) and what it wrote to d_params; the destination planes as it left them.  reciprocal_lambda_q16 as there.
 * flags: bit 0 slice_sao_luma_flag, bit 1 slice_sao_chroma_flag (as given to the estimate), bit 2 entropy_coding_sync_enabled_flag
 * (WPP: a row starts from the states after CTU (1, r - 1), or from the slice's when that CTU does not exist; without it a row starts
 * where the row above ended).  ctx_sao_merge / ctx_sao_type: ContextModel::state (2 pStateIdx + valMps, turing/Cabac.cpp:26-37) of
 * sao_merge_X_flag and sao_type_idx_X at the slice start.  One slice starting at CTU 0, one tile, 4:2:0.  With flags & 3 == 0 no sao()
 * is coded (SyntaxCtu.hpp:40): every record is all off and the states do not move.
 *   Outputs: one record per CTU, and the destination rewritten for every CTU whose final parameters differ from its estimate, so that it
 * holds every CTU filtered with its final parameters (computeSaoDistortion's form).  A CTU record that the estimate reports off (odd
 * or out-of-range size) is never written and takes part with distortion 0.
 * d_work: havoc_mi355x_sao_decide_workspace(nctus) bytes of device scratch, 16-byte aligned, private to the call until it completes.
 * The call waits inside the device on the row above (bounded waits); if one gives up, every record has decided = 0. */
typedef struct {
    havoc_mi355x_sao_component comp[2];   /* the final parameters; a type-0 component is all zeros (the reference's SaoCtuData keeps the
                                             estimate's stale fields there, which nothing reads) */
    int32_t merge_left, merge_up;    /* sao_merge_left_flag, sao_merge_up_flag */
    int32_t dist;                    /* computeSaoDistortion with the final parameters */
    int32_t source;                  /* the CTU whose estimate the final parameters are (merges followed to their origin); -1: all off */
    uint8_t ctx_merge_before, ctx_type_before;   /* the two context states before this CTU's SAO syntax ... */
    uint8_t ctx_merge_after, ctx_type_after;     /* ... and after it */
    int32_t decided;                 /* 1; 0 when a wait inside the call gave up (then no record of the call is a decision) */
    int32_t reserved[4];
} havoc_mi355x_sao_decision; /* 128 bytes */
size_t havoc_mi355x_sao_decide_workspace(int nctus);
int havoc_mi355x_sao_decide(havoc_mi355x_ctx *ctx, int S, int bitDepth, int32_t reciprocal_lambda_q16, int flags,
                            const void *d_src_y, const void *d_src_c, intptr_t stride_src_y, intptr_t stride_src_c,
                            const void *d_rec_y, const void *d_rec_c, intptr_t stride_rec_y, intptr_t stride_rec_c,
                            void *d_dst_y, void *d_dst_c, intptr_t stride_dst_y, intptr_t stride_dst_c,
                            const havoc_mi355x_sao_ctu *d_ctus, int nctus, int ctus_x, const havoc_mi355x_sao_params *d_params,
                            int ctx_sao_merge, int ctx_sao_type, void *d_work, size_t work_bytes, havoc_mi355x_sao_decision *d_decisions);

/* In-loop SAO of a whole 4:2:0 picture, the pass a picture goes through before it becomes a reference: per CTU, what the encoder's
 * TaskSao (turing/TaskSao.cpp:96-121) leaves in the picture -- LoopFilter::Picture::applySaoCTU -> filterBlockSao (turing/LoopFilter.h:
 * 795-811, 886-1008) from a copy of the deblocked picture -- in one launch on the context's stream (no host synchronisation, no
 * allocation: capturable into a graph).  Per CTU and colour component:
 *   - the offsets of Ctu::set (LoopFilter.h:114-162): SaoOffsetVal[i + 1] = sign x sao_offset_abs << (bitDepth - min(bitDepth, 10)),
 *     edge signs + + - -, SaoOffsetVal[0] = 0 (every band outside the four);
 *   - band or edge filter (turing/sao.cpp:33-92), or a copy for type 0;
 *   - restoreUnfilteredRegions (LoopFilter.h:850-877): the 8x8 luma / 4x4 chroma regions whose deblocking byte has the disabled bit;
 *   - edge only: the undoT / undoL / undoR / undoB copies of filterBlockSao (LoopFilter.h:913-986) where a neighbour CTU is not
 *     available, from the CTU's bounds and corner flags (processCtu, LoopFilter.h:475-537), right / bottom clamped to the CTU.
 * d_rec_* / d_dst_*: sample (0, 0) of each plane; the destination must not overlap the source (filtering reads the deblocked
 * neighbours, as the encoder's saoPicture copy does).  flags: bit 0 slice_sao_luma_flag, bit 1 slice_sao_chroma_flag; a component whose
 * flag is 0 is copied.  d_decisions: one record per CTU in raster order, as havoc_mi355x_sao_decide writes them; comp[1] drives Cb and
 * Cr; a record with decided == 0 is applied as all off.  d_bounds: one record per CTU in raster order, or NULL for one slice and one
 * tile (the picture's edges only).  d_block_data: havoc_mi355x_deblock's (QpY << 1) | disabled bytes, row stride block_stride >=
 * (width + 7) / 8, at least (height + 7) / 8 rows; NULL: no disabled regions.
 * Writes every sample of [0, width) x [0, height) (luma) and [0, width / 2) x [0, height / 2) (Cb, Cr), and nothing outside: the
 * reference filters chroma beyond the right and bottom picture edges (filterBlockSao clips chroma CTUs against the LUMA picture size,
 * LoopFilter.h:895-897), into samples that padBlock overwrites before anything reads them (TaskSao.cpp:129-154).  Reads only inside
 * the picture: a sample whose neighbour lies outside is always one the reference restores.
 * EINVAL: overlapping planes, ctb_log2 outside 4..6, width / height not a positive multiple of 8, a bit depth outside 8..10 or not
 * matching S, a null d_decisions, a block_stride too small. */
typedef struct {
    int32_t left, top, right, bottom; /* LoopFilter::Ctu's bounds in luma samples (processCtu, LoopFilter.h:476-535) */
    int32_t corners;                  /* bit 0 topLeft, 1 topRight, 2 bottomLeft, 3 bottomRight */
    int32_t reserved[3];
} havoc_mi355x_sao_bounds; /* 32 bytes */
int havoc_mi355x_sao_apply(havoc_mi355x_ctx *ctx, int S, int bitDepth, int flags, int width, int height, int ctb_log2,
                           const void *d_rec_y, const void *d_rec_cb, const void *d_rec_cr, intptr_t stride_rec_y, intptr_t stride_rec_c,
                           void *d_dst_y, void *d_dst_cb, void *d_dst_cr, intptr_t stride_dst_y, intptr_t stride_dst_c,
                           const havoc_mi355x_sao_decision *d_decisions, const havoc_mi355x_sao_bounds *d_bounds,
                           const int8_t *d_block_data, intptr_t block_stride);

/* ------------------------------------------------------------------------------------------------------- */
/* rate-distortion optimised quantisation                                                 */
/* ------------------------------------------------------------------------------------------------------- */
/* Rdoq::runQuantisation (turing/Rdoq.cpp:37-454), the quantiser the reference's speed=medium uses between the forward
 * transform and the reconstruction (turing/Reconstruct.cpp:289-312 intra, :794-812 inter).  One job = one transform block of
 * the launch's size.  The CABAC probability states are read, never updated, so the entropy coder is a frozen snapshot of
 * state bytes (ContextModel::state, turing/ContextModel.h:29-31) in this layout, 128 bytes per snapshot: */
enum {
    HAVOC_RDOQ_CTX_ROOT_CBF = 0,   /* rqt_root_cbf [1] */
    HAVOC_RDOQ_CTX_CBF_LUMA = 1,   /* cbf_luma [2] */
    HAVOC_RDOQ_CTX_CBF_CHROMA = 3, /* cbf_cb / cbf_cr [4] */
    HAVOC_RDOQ_CTX_LAST_X = 8,     /* last_sig_coeff_x_prefix [18] */
    HAVOC_RDOQ_CTX_LAST_Y = 26,    /* last_sig_coeff_y_prefix [18] */
    HAVOC_RDOQ_CTX_CSBF = 44,      /* coded_sub_block_flag [4] */
    HAVOC_RDOQ_CTX_SIG = 48,       /* sig_coeff_flag [44] */
    HAVOC_RDOQ_CTX_GREATER1 = 92,  /* coeff_abs_level_greater1_flag [24] */
    HAVOC_RDOQ_CTX_GREATER2 = 116, /* coeff_abs_level_greater2_flag [6] */
    HAVOC_RDOQ_CTX_BYTES = 128
};
typedef struct {
    int32_t dst_off, src_off;          /* n*n contiguous int16 levels (out) / coefficients (in); multiples of 4 (8-byte rows) */
    int32_t quant_scale, quant_shift;  /* runQuantisation's quantiserScale / quantiserShift */
    int32_t inv_scale;                 /* the constructor's invQuantScale */
    int32_t lambda_q16, sdh_factor;    /* from havoc_mi355x_rdoq_lambda */
    int32_t ctx_index;                 /* which 128-byte snapshot of d_states */
    uint8_t c_idx, scan_idx;           /* rc.cIdx (0..2), scanIdx (0 diagonal, 1 horizontal, 2 vertical) */
    uint8_t is_intra, sdh;             /* isIntra, isSdhEnabled */
    int32_t reserved[3];
} havoc_mi355x_rdoq_job; /* 48 bytes */
/* the two integers the Rdoq constructor derives from the floating-point lambda (turing/Rdoq.h:163-167); host-side, no device work */
void havoc_mi355x_rdoq_lambda(double lambda, int inv_scale, int32_t *lambda_q16, int32_t *sdh_factor);
/* d_cbf[i] = runQuantisation's return value (OR of the kept absolute levels).  d_dst and d_src are different buffers, as in the
 * reference (quantizedCoefficients vs coefficients, Reconstruct.cpp:276-277); every level of a job's block is written. */
/* d_work: havoc_mi355x_rdoq_workspace(njobs) bytes of device scratch, 16-byte aligned, private to the launch until it completes
 * (per block: which 4x4 groups are non-zero, the block's energy; the order the blocks are walked in: densest first, so that
 * the 64 blocks a wavefront walks finish together). */
size_t havoc_mi355x_rdoq_workspace(int njobs);
int havoc_mi355x_rdoq(havoc_mi355x_ctx *ctx, int bitDepth, int log2TrafoSize, int16_t *d_dst, const int16_t *d_src, const uint8_t *d_states,
                      const havoc_mi355x_rdoq_job *d_jobs, int njobs, int32_t *d_cbf, void *d_work, size_t work_bytes);

/* ---- the CABAC rate of residual_coding per transform block (csrc/kernels_residual_rate.hip) ----
 * The bits the reference's EstimateRate verb measures for one residual_coding (turing/EncodeResidual.hpp:36-301 with H::Tag == EstimateRate<void>, over what
 * CodedData::storeResidual packs from the n x n raster of levels), bit for bit, as a Cost (Q16, int64).  One job = a chain of `count` blocks of the launch's size, walked in
 * order from the job's snapshot with the contexts carried from one block to the next: the reference walks the four depth-1 luma blocks of a unit in z-order that way, and
 * luma residual contexts are moved by luma residuals only, so a chain of four gives the luma residual bits of that tree from the unit's snapshot.
 *   - a context-coded bin costs the Q15 table entry (turing/Write.h:413-422) shifted to Q16 and MOVES its context (measureEncodeDecision, Write.h:476-492): every bin is
 *     priced from the state the previous bins of the chain left; a bypass bin costs 1 << 16;
 *   - sign bits are popcount(sigCoeffFlags) - signHidden whole bits per sub-block; signHidden only with `sdh` and a significant coefficient at scan position >= 3;
 *   - coeff_abs_level_greater2_flag is priced inside the greater1 loop (the EstimateRate tag), at most 8 greater1 flags per sub-block, the base level of the later
 *     coefficients from the reference's countdown arithmetic; ctxSet from greater1Ctx / lastGreater1Flag as the previously VISITED sub-block left them (-1 / 1 at the
 *     start of a block);
 *   - coded_sub_block_flag only for sub-blocks other than the last and sub-block 0, its context from the right / below neighbours (the `snake` word); the DC sig flag of
 *     such a sub-block is inferred when no other coefficient of it is significant; sub-block 0 is always visited (empty: its sig flags are priced as zeros);
 *   - the last position's own sig flag is not priced; scan_idx 2 swaps the x and y of the last position;
 *   - an all-zero block costs 0 and touches no context (IfCbf).
 * transform_skip_enabled_flag = 0 and cu_transquant_bypass_flag = 0.  scan_idx != 0 only with log2TrafoSize <= 3, c_idx != 0 only with log2TrafoSize <= 4 (4:2:0).
 * A job with count outside 1..4, c_idx > 2, scan_idx > 2 or an excluded (size, scan / component) pair is not walked: no level is read, d_rate[rate_index .. rate_index +
 * min(max(count, 1), 4) - 1] = -1 and its d_states_out is its input snapshot.  level_off, ctx_index and rate_index are trusted, as in havoc_mi355x_rdoq.
 * d_states is never written.  d_states_out: NULL, or njobs x 128 bytes: the job's snapshot after its last block (bytes outside the residual contexts copied).
 * d_levels and d_rate 8-byte aligned.  No allocation, no synchronisation, no workspace: capturable into a HIP graph. */
typedef struct {
    int32_t level_off;   /* first of `count` blocks of n*n contiguous int16 levels (raster, as havoc_mi355x_rdoq writes them); block k at level_off + k*n*n; multiple of 4 */
    int32_t ctx_index;   /* the 128-byte snapshot of d_states (HAVOC_RDOQ_CTX_* layout) block 0 starts from */
    int32_t rate_index;  /* block k's rate -> d_rate[rate_index + k] */
    uint8_t c_idx, scan_idx, sdh, count;   /* count 1..4: the blocks are walked in order, the contexts carried from one to the next */
    int32_t reserved[4];
} havoc_mi355x_residual_rate_job;   /* sizeof: 32 */
int havoc_mi355x_residual_rate(havoc_mi355x_ctx *ctx, int log2TrafoSize, const int16_t *d_levels, const uint8_t *d_states, const havoc_mi355x_residual_rate_job *d_jobs,
                               int njobs, int64_t *d_rate, uint8_t *d_states_out);

/* ---- the CABAC rate of one refined intra candidate (csrc/kernels_residual_rate.hip: k_intra_rate) ----
 * What searchIntraPartition measures for a challenger with EstimateRateLuma "since the partition began" (turing/Search.hpp:199, 242-246): Syntax<IntraPartition>
 * (turing/SyntaxCtu.hpp:704-722) from the contexts the partition started with, luma only (turing/EstimateRate.h:114-119 nulls cbf_cb, cbf_cr, the chroma residuals and
 * intra_chroma_pred_mode).  One job = one candidate = one transform block of the launch's size; in the syntax's order
 *   - prev_intra_luma_pred_flag, one context (turing/Binarization.h:395-452): 1 when the mode is in candModeList;
 *   - mpm_idx, truncated Rice with cMax 2, bypass: 1 bit for 0, 2 bits for 1 or 2 (:454-487) -- else rem_intra_luma_pred_mode, 5 bypass bits (:489-502);
 *   - split_transform_flag = 0 (a candidate is one transform block), ctxInc = 5 - log2TrafoSize (:617-634), where transform_tree codes it (SyntaxCtu.hpp:330-337):
 *     the caller says so per job (HAVOC_INTRA_RATE_SPLIT_FLAG_CODED; libhavoc_search.so: havoc_search_intra_rate_flags has the rule);
 *   - cbf_luma, always coded for intra, ctxInc = trafoDepth == 0 ? 1 : 0 (:637-651), at HAVOC_RDOQ_CTX_CBF_LUMA of the 128-byte snapshot;
 *   - when the block has a level: its residual_coding with c_idx 0, exactly the walk of havoc_mi355x_residual_rate.
 * Context-coded bins cost the Q15 table entry shifted to Q16 and move their context, bypass bins 1 << 16.  prev_intra_luma_pred_flag and split_transform_flag are not
 * in the 128-byte snapshot: d_syntax_states holds them, HAVOC_INTRA_SYNTAX_CTX_BYTES per snapshot, indexed by the same ctx_index: */
enum {
    HAVOC_INTRA_SYNTAX_CTX_PREV_INTRA_LUMA_PRED_FLAG = 0,   /* prev_intra_luma_pred_flag [1] */
    HAVOC_INTRA_SYNTAX_CTX_SPLIT_TRANSFORM_FLAG = 1,        /* split_transform_flag [3], by ctxInc = 5 - log2TrafoSize */
    HAVOC_INTRA_SYNTAX_CTX_BYTES = 4
};
enum {
    HAVOC_INTRA_RATE_SPLIT_FLAG_CODED = 1,   /* split_transform_flag is coded (as 0) */
    HAVOC_INTRA_RATE_DEPTH_NONZERO = 2       /* trafoDepth != 0: the blocks of an NxN unit */
};
typedef struct {
    int32_t level_off;   /* the block's n*n contiguous int16 levels (raster, as havoc_mi355x_rdoq writes them); multiple of 4 */
    int32_t ctx_index;   /* the snapshot of d_states (128 bytes) and of d_syntax_states (4 bytes) the candidate starts from */
    int32_t rate_index;  /* the candidate's rate -> d_rate[rate_index] */
    uint8_t scan_idx, sdh;   /* as in havoc_mi355x_residual_rate_job */
    uint8_t mpm_idx;     /* 0..2: the first x with mode == candModeList[x]; 3: rem_intra_luma_pred_mode */
    uint8_t flags;       /* HAVOC_INTRA_RATE_* */
    int32_t reserved[4];
} havoc_mi355x_intra_rate_job;   /* sizeof: 32 */
/* A job with mpm_idx > 3, scan_idx > 2, scan_idx != 0 with log2TrafoSize > 3, or HAVOC_INTRA_RATE_SPLIT_FLAG_CODED with log2TrafoSize == 2 is not walked: no level
 * is read, d_rate[rate_index] = -1 and its output snapshots are its input snapshots.  An all-zero block still pays its prefix and cbf_luma = 0 and moves only those
 * contexts.  level_off, ctx_index and rate_index are trusted.  d_states and d_syntax_states are never written.  d_states_out: NULL, or njobs x 128 bytes;
 * d_syntax_states_out: NULL, or njobs x 4 bytes: the snapshot as candidate j left it -- what a chain from partition to partition would carry on from the champion.
 * d_levels and d_rate 8-byte aligned.  No allocation, no synchronisation, no workspace: capturable into a HIP graph. */
int havoc_mi355x_intra_rate(havoc_mi355x_ctx *ctx, int log2TrafoSize, const int16_t *d_levels, const uint8_t *d_states, const uint8_t *d_syntax_states,
                            const havoc_mi355x_intra_rate_job *d_jobs, int njobs, int64_t *d_rate, uint8_t *d_states_out, uint8_t *d_syntax_states_out);

/* ---- the CABAC rate of an inter unit's whole transform tree at one depth (csrc/kernels_residual_rate.hip: k_tree_rate) ----
 * What the inter transform-tree decision compares (turing/Reconstruct.cpp:1296-1428): EstimateRate<void> over `if (rqt_root_cbf) transform_tree` of an inter 2Nx2N coding
 * unit of log2 size L = log2CbSize in {3, 4, 5} (6: below), coded at `depth` 0 (one transform unit) or 1 (four), with ONE CABAC state running through split_transform_flag, cbf_cb,
 * cbf_cr, cbf_luma and the Y, Cb and Cr residual_coding (Syntax<transform_tree>, turing/SyntaxCtu.hpp:329-379; Syntax<transform_unit>, :411-502; the writers,
 * turing/Binarization.h:617-666).  rqt_root_cbf itself is NOT priced.  Preconditions (turing/Encoder.cpp:662-666 with the residual quadtree on): MaxTrafoDepth 1 for
 * inter, MinTbLog2SizeY 2, MaxTbLog2SizeY >= L, 4:2:0, CuPredMode MODE_INTER, scanIdx 0, and cu_qp_delta_enabled_flag, cu_chroma_qp_offset_enabled_flag,
 * cross_component_prediction_enabled_flag, transform_skip_enabled_flag, cu_transquant_bypass_flag all 0.  One launch = one (L, depth); one job = one candidate tree:
 *   depth 0: split_transform_flag = 0 (ctxInc 5 - L) where coded; cbf_cb, cbf_cr (ctxInc 0); cbf_luma (ctxInc 1) ONLY when cbf_cb || cbf_cr (else inferred 1, no bin);
 *            residual_coding of the Y block (log2 L), the Cb block and the Cr block (log2 max(L - 1, 2));
 *   depth 1: split_transform_flag = 1 (ctxInc 5 - L) where coded; the parent's cbf_cb, cbf_cr (ctxInc 0): the OR of the children's, for L == 3 the one 4x4 block's own;
 *            per child k = 0..3 in z-order, without a split flag: for L > 3 cbf_cb (ctxInc 1) only if the parent's is 1, the same for cbf_cr; cbf_luma (ctxInc 0), always;
 *            the child's Y block (log2 L - 1); for L > 3 its Cb and then its Cr block (log2 L - 2); for L == 3 after child 3 ONLY the parent's 4x4 Cb and then Cr block.
 * cbf_cb and cbf_cr share the contexts at HAVOC_RDOQ_CTX_CBF_CHROMA, Cb and Cr residuals the chroma residual contexts: the order Cb0 Cr0 Cb1 Cr1 ... is the syntax's.
 * A tree with no level in any plane (rqt_root_cbf = 0) costs 0 and moves no context.  split_transform_flag's contexts are in the 4-byte syntax snapshot
 * (HAVOC_INTRA_SYNTAX_CTX_SPLIT_TRANSFORM_FLAG; its first byte passes through), everything else in the 128-byte one.
 * d_rate[out_index]: the Q16 Cost.  d_cbf[out_index]: bit k = Y block k has a level, bit 4 + k = Cb block k, bit 8 + k = Cr block k (depth 0, and the chroma of L == 3, use
 * k = 0 only).  d_states_out / d_syntax_states_out: NULL, or njobs x 128 / njobs x 4 bytes: job j's snapshots as its walk left them (an all-zero tree: its input).
 * (6, 1) is accepted as well: a 64x64 unit lies above MaxTbLog2SizeY (5), so its transform depth and its split are inferred (turing/Reconstruct.cpp:1300-1310) and it has ONE
 * tree -- depth 1 as above WITHOUT the split_transform_flag bin: cbf_cb, cbf_cr (ctxInc 0), then per child cbf_cb / cbf_cr (ctxInc 1, only when the parent's is 1),
 * cbf_luma (ctxInc 0), Y 32x32, Cb and Cr 16x16.  (6, 0) does not exist.
 * For L in {3, 4, 5} the syntax can code split_transform_flag at every size, so no flag value is impossible; a job whose `flags` has a bit other than
 * HAVOC_TREE_RATE_SPLIT_FLAG_CODED cannot be walked: no level of it is read, d_rate = -1, d_cbf = 0, its output snapshots are its input.  For L == 6 the flag is never
 * coded: HAVOC_TREE_RATE_SPLIT_FLAG_CODED is an impossible value there and is refused in the same way, like an unknown bit.  Below 6 the flag itself is TRUSTED: the
 * kernel sees neither MaxTbLog2SizeY nor MaxTrafoDepth, so a caller who sets it for a unit whose split is inferred (a 32x32 unit above MaxTbLog2SizeY, interSplitFlag) gets
 * the price of a bin the syntax does not code, and no refusal.  The offsets and indices are trusted: luma_off, cb_off and cr_off are multiples of 4 (the levels are read
 * as 8-byte rows).  The inputs are never written.  d_luma_levels, d_chroma_levels and d_rate 8-byte aligned, d_cbf 4-byte.  EINVAL: log2CbSize outside 3..6, depth outside 0..1, log2CbSize 6 at depth 0,
 * njobs < 0, a null input or d_rate / d_cbf, an output snapshot table that is its input.  No allocation, no synchronisation, no workspace: capturable into a HIP graph. */
enum { HAVOC_TREE_RATE_SPLIT_FLAG_CODED = 1 };   /* split_transform_flag of the unit is coded (as `depth`) */
typedef struct {
    int32_t luma_off;        /* in d_luma_levels: depth 0 the unit's n*n block; depth 1 four (n/2)^2 blocks, contiguous, z-order; int16 raster; multiple of 4 */
    int32_t cb_off, cr_off;  /* in d_chroma_levels: depth 0, or n == 8: one block of c*c, c = max(n/2, 4); depth 1 and n > 8: four (n/4)^2 blocks, contiguous, z-order; multiples of 4 */
    int32_t ctx_index;       /* the snapshot of d_states (128 bytes) and of d_syntax_states (4 bytes) the tree starts from */
    int32_t out_index;       /* d_rate[out_index], d_cbf[out_index] */
    uint8_t sdh, flags, pad[2];   /* sign_data_hiding_enabled_flag; HAVOC_TREE_RATE_* */
    int32_t reserved[2];
} havoc_mi355x_tree_rate_job;   /* sizeof: 32 */
int havoc_mi355x_tree_rate(havoc_mi355x_ctx *ctx, int log2CbSize, int depth, const int16_t *d_luma_levels, const int16_t *d_chroma_levels, const uint8_t *d_states,
                           const uint8_t *d_syntax_states, const havoc_mi355x_tree_rate_job *d_jobs, int njobs, int64_t *d_rate, uint32_t *d_cbf,
                           uint8_t *d_states_out, uint8_t *d_syntax_states_out);

/* ---- the CABAC rate of a prediction unit's candidates and the inter mode decision (csrc/kernels_pu_rate.hip: k_pu_rate, k_pu_decide) ----
 * What measurePuCost measures for every candidate go2 tries for a prediction unit (turing/Search.hpp:1656-1706, 1844-1902): Syntax<prediction_unit>
 * (turing/SyntaxCtu.hpp:267-314) under Measure<void> from the contexts the unit started with.  One job = one candidate; in the syntax's order
 *   - HAVOC_PU_RATE_SKIP (cu_skip_flag): only merge_idx, when MaxNumMergeCand > 1;
 *   - else merge_flag, one context (turing/Binarization.h:538-547); HAVOC_PU_RATE_MERGE: merge_idx when MaxNumMergeCand > 1 -- truncated Rice with cMax =
 *     MaxNumMergeCand - 1, bin 0 context-coded, the others bypass (:549-582);
 *   - not merged: inter_pred_idc in B slices only (:585-612): with nPbW + nPbH != 12 bi is one bin 1 at ctxInc cqt_depth, uni is 0 there and then the list at ctxInc 4;
 *     with nPbW + nPbH == 12 only the list bin at ctxInc 4.  Then for list 0 unless pred is L1, and for list 1 unless pred is L0: ref_idx_lX when
 *     num_ref_idx_lX_active_minus1 > 0; mvd_coding (SyntaxCtu.hpp:382-405: greater0(x), greater0(y), greater1(x), greater1(y), then per component abs_mvd_minus2 --
 *     EG1, bypass -- and the sign, bypass; Binarization.h:745-809), skipped for list 1 when mvd_l1_zero_flag is set and pred is BI; mvp_lX_flag (:811-831).
 * ref_idx_l0 / ref_idx_l1 share two contexts, the two abs_mvd_greater0_flag bins one, the two abs_mvd_greater1_flag bins one, mvp_l0_flag / mvp_l1_flag one
 * (turing/Cabac.h:112-126), so every bin is priced from the state the previous bins left.  ref_idx_lX: the reference has NO writer for it (its generic writer,
 * Binarization.h:52-59, asserts in a debug build and writes nothing in a release one; its encoder searches refIdx 0 of lists of one picture, Search.hpp:1883-1884).
 * It is priced here for every value the syntax allows as the inverse of the reference's reader (ReadRefIdx, turing/Read.h:1864-1888; H.265 9.3.4.2): truncated Rice with
 * cMax = num_ref_idx_lX_active_minus1, bins 0 and 1 context-coded with ctxInc = binIdx, the rest bypass.  With num_ref_idx_lX_active_minus1 == 0 -- all the reference
 * encoder produces -- every bit is the reference's own.
 * Context-coded bins cost the Q15 table entry shifted to Q16 and move their context (measureEncodeDecision, turing/Write.h:476-506), bypass bins 1 << 16 (:559-567).
 * These contexts are in neither the 128-byte snapshot nor the 4-byte intra one: d_syntax_states holds HAVOC_PU_SYNTAX_CTX_BYTES per snapshot, each byte a
 * ContextModel::state, indexed by the job's ctx_index: */
enum {
    HAVOC_PU_SYNTAX_CTX_MERGE_FLAG = 0,         /* merge_flag [1] */
    HAVOC_PU_SYNTAX_CTX_MERGE_IDX = 1,          /* merge_idx [1] */
    HAVOC_PU_SYNTAX_CTX_INTER_PRED_IDC = 2,     /* inter_pred_idc [5]: ctxInc cqtDepth 0..3, 4 = the list bin */
    HAVOC_PU_SYNTAX_CTX_REF_IDX = 7,            /* ref_idx_lX [2] */
    HAVOC_PU_SYNTAX_CTX_ABS_MVD_GREATER0 = 9,   /* abs_mvd_greater0_flag [1] */
    HAVOC_PU_SYNTAX_CTX_ABS_MVD_GREATER1 = 10,  /* abs_mvd_greater1_flag [1] */
    HAVOC_PU_SYNTAX_CTX_MVP_FLAG = 11,          /* mvp_lX_flag [1] */
    HAVOC_PU_SYNTAX_CTX_BYTES = 16              /* 12..15 reserved: passed through */
};
enum {
    HAVOC_PU_RATE_MERGE = 1,   /* merge_flag = 1 */
    HAVOC_PU_RATE_SKIP = 2     /* cu_skip_flag = 1 (merge_flag is not coded; HAVOC_PU_RATE_MERGE beside it changes nothing) */
};
enum { HAVOC_PU_PRED_L0 = 0, HAVOC_PU_PRED_L1 = 1, HAVOC_PU_PRED_BI = 2 };   /* = PRED_L0, PRED_L1, PRED_BI */
typedef struct {
    int32_t ctx_index;       /* the snapshot of d_syntax_states (16 bytes) the candidate starts from */
    int32_t out_index;       /* the candidate's rate -> d_rate[out_index] */
    int16_t mvd[2][2];       /* [list][x, y]: the motion vector difference, quarter samples; read for the lists `pred` uses */
    uint8_t merge_idx;       /* read when merged or skipped */
    uint8_t pred;            /* HAVOC_PU_PRED_*: inter_pred_idc; read when not merged */
    uint8_t mvp_flag[2];     /* mvp_l0_flag, mvp_l1_flag */
    uint8_t ref_idx[2];      /* ref_idx_l0, ref_idx_l1 */
    uint8_t w, h;            /* nPbW, nPbH: only w + h == 12 (8x4 / 4x8) is looked at */
    uint8_t cqt_depth;       /* cqtDepth of the coding quadtree the unit belongs to, 0..3 */
    uint8_t flags;           /* HAVOC_PU_RATE_* */
    uint8_t pad[2];
    int32_t reserved;
} havoc_mi355x_pu_rate_job;   /* sizeof: 32 */
typedef struct {
    int32_t slice_b;                        /* slice_type == B (else P: inter_pred_idc is not coded) */
    int32_t max_num_merge_cand;             /* MaxNumMergeCand, 1..5 */
    int32_t mvd_l1_zero_flag;
    int32_t num_ref_idx_active_minus1[2];   /* num_ref_idx_l0_active_minus1, num_ref_idx_l1_active_minus1, 0..15 */
    int32_t reserved[3];
} havoc_mi355x_pu_slice;   /* sizeof: 32; read on the host at the call, passed by value */
/* A job the syntax cannot code is not walked: d_rate[out_index] = -1 and its output snapshot is its input snapshot.  That is: a `flags` bit other than HAVOC_PU_RATE_*;
 * merged or skipped with merge_idx >= MaxNumMergeCand; not merged with pred > 2, with pred BI and w + h == 12, with pred other than L0 in a P slice, with cqt_depth > 3
 * (it indexes the contexts), or -- for a list pred uses -- mvp_flag > 1 or ref_idx > num_ref_idx_lX_active_minus1.  ctx_index and out_index are trusted; w and h are
 * trusted (whether a unit of that shape exists is the caller's).  d_syntax_states is never written.  d_syntax_out: NULL, or njobs x 16 bytes: the snapshot as candidate j
 * left it.  All device pointers 8-byte aligned.  EINVAL: a null d_syntax_states, d_jobs, slice or d_rate; njobs < 0; MaxNumMergeCand outside 1..5;
 * num_ref_idx_lX_active_minus1 outside 0..15; d_syntax_out == d_syntax_states.  No allocation, no synchronisation, no workspace: capturable into a HIP graph. */
int havoc_mi355x_pu_rate(havoc_mi355x_ctx *ctx, const uint8_t *d_syntax_states, const havoc_mi355x_pu_rate_job *d_jobs, int njobs, const havoc_mi355x_pu_slice *slice,
                         int64_t *d_rate, uint8_t *d_syntax_out);
/* go2's comparison (turing/Search.hpp:1829-1842) of n prediction units, a lane per unit.  Unit i's candidates are the contiguous entries [d_first[i], d_first[i] +
 * d_count[i]) of d_rate (havoc_mi355x_pu_rate with out_index = job index), d_satd_y / _cb / _cr and d_syntax_after (havoc_mi355x_pu_rate's d_syntax_out), in the order the
 * reference tries them: merge 0..N-1 for units that are not 2Nx2N, then L0, L1, BI.  WHICH candidates exist is the caller's (L0 / L1 only when that list has a
 * reference; BI only when both uni candidates exist and nPbW + nPbH != 12, Search.hpp:1883-1891).  d_cost[t] = d_rate[t] + int64(int32(satdY + satdCb + satdCr)) *
 * reciprocal_sqrt_lambda_q16 (measurePuCost, :1705; FixedPoint<int32_t, 16> * int32_t, turing/FixedPoint.h:79; the lambda is Lambda::set(double): int32(d * 65536 + 0.5)),
 * or -1 for a candidate whose rate is -1, which is never chosen.  d_best[i]: the first of the cheapest, as an index within the unit (a later candidate replaces the best
 * only when cost < bestCost), or -1 when the unit has no valid candidate; d_best_cost[i]: its cost, or -1.  d_best_syntax: NULL, or n x 16 bytes: the winner's snapshot
 * from d_syntax_after (bestContextsAndCost), 16 zero bytes for a unit without a winner.  d_first and d_count are trusted.  The inputs are never written.  d_rate, d_cost,
 * d_best_cost, d_syntax_after and d_best_syntax 8-byte aligned.  EINVAL: a null pointer other than d_syntax_after / d_best_syntax, d_best_syntax without d_syntax_after,
 * n < 0, a negative lambda, an output that is one of the inputs.  No allocation, no synchronisation, no workspace: capturable into a HIP graph. */
int havoc_mi355x_pu_decide(havoc_mi355x_ctx *ctx, const int32_t *d_first, const int32_t *d_count, int n, const int64_t *d_rate, const int32_t *d_satd_y,
                           const int32_t *d_satd_cb, const int32_t *d_satd_cr, int32_t reciprocal_sqrt_lambda_q16, const uint8_t *d_syntax_after, int64_t *d_cost,
                           int32_t *d_best, int64_t *d_best_cost, uint8_t *d_best_syntax);

/* The same two steps with the scan of the coefficients done where they are produced (16x16 / 32x32 blocks; round 3):
 *   tu_forward_scan  = tu_forward + the first pass of the device RDOQ (which 4x4 groups hold a rounded level, the block's energy -> d_work;
 *                      the level block of d_rdoq_jobs[i].dst_off zeroed).  d_rdoq_jobs[i] describes the same block as d_jobs[i]
 *                      (src_off = the job's coef_off).
 *   rdoq_prescanned  = the rest of havoc_mi355x_rdoq on that workspace: levels and flags identical to havoc_mi355x_rdoq on the coefficients.
 * Saves a kernel that re-reads every coefficient per block size (2 x 47 MB and 47 us of launches per 1080p picture). */
int havoc_mi355x_tu_forward_scan(havoc_mi355x_ctx *ctx, int S, int bitDepth, int log2TrafoSize, int16_t *d_coeffs, const void *d_src, intptr_t stride_src,
                                 const void *d_pred, intptr_t stride_pred, const havoc_mi355x_tu_fused_job *d_jobs, int njobs,
                                 const havoc_mi355x_rdoq_job *d_rdoq_jobs, int16_t *d_levels, void *d_work, size_t work_bytes);
int havoc_mi355x_rdoq_prescanned(havoc_mi355x_ctx *ctx, int bitDepth, int log2TrafoSize, int16_t *d_dst, const int16_t *d_src, const uint8_t *d_states,
                                 const havoc_mi355x_rdoq_job *d_jobs, int njobs, int32_t *d_cbf, void *d_work, size_t work_bytes);

/* ---- the intra decisions that are data-parallel (one lane per partition), taken on the device between the launches they separate ----
 * Not reference primitives: the reference takes them inline in searchIntraPartition (turing/Search.hpp:40-255).  A batch client that
 * refines a picture's intra partitions (libhavoc_search.so: havoc_search_intra_device) chains
 *     intra_satd35 -> intra_order -> intra_expand -> intra -> tu_forward -> rdoq -> tu_reconstruct -> level_stats -> intra_decide -> tu_reconstruct
 * (havoc_search_intra_device_rated: ... -> tu_reconstruct -> intra_rate_jobs -> intra_rate -> intra_decide_rated -> tu_reconstruct, the reference's CABAC bits as the rate)
 * so that neither the 35 costs per partition nor the job records per candidate cross the link. */
#define HAVOC_MI355X_INTRA_MAX_ORDER 12
typedef struct
{
    int32_t cand_mode_list[3];     /* candModeList (Search.hpp:55-98) */
    int32_t neighbour_modes;       /* how many of them are forced into the refinement if not selected (Search.hpp:170-180) */
    int32_t max_refine;            /* selections before that happens; max_refine + neighbour_modes <= HAVOC_MI355X_INTRA_MAX_ORDER */
    int32_t reserved;
    int64_t rate_a_minus_c, rate_b_minus_c;   /* Q16 rate offsets of candModeList[0] / [1], [2] relative to a mode outside the list */
} havoc_mi355x_intra_mpm;          /* 40 bytes; = havoc_search_intra_ctx */
typedef struct
{
    int32_t mode, index, evaluated, reserved;
    int64_t cost;                  /* Q16: mode rate + residual rate + ssd * reciprocal lambda */
    int32_t cbf;
    uint32_t ssd;
    int32_t nonzero, sum_abs;
} havoc_mi355x_intra_choice;       /* 40 bytes; = havoc_intra_rd_result */
/* Search.hpp:55-98, 143-190: costs = rate offsets + lambda_q16 * d_satd35[35 * i + mode] (64-bit), then the order the modes are refined in:
 * d_order[HAVOC_MI355X_INTRA_MAX_ORDER * i + k], k < d_count[i]; d_slot[i] = the partition's first candidate slot;
 * d_total[0] = slots handed out; d_total[1]: bit 0 = some partition wanted more than HAVOC_MI355X_INTRA_MAX_ORDER (its order is cut), bit 1 = some record was out of
 * range (a mode outside 0..34, neighbour_modes outside 0..3, max_refine < 1: brought into range, nothing is written outside the partition's slots) -- results are
 * then not to be used. */
int havoc_mi355x_intra_order(havoc_mi355x_ctx *ctx, const int32_t *d_satd35, const havoc_mi355x_intra_mpm *d_mpm, int n, int32_t lambda_q16, int32_t *d_order,
                             int32_t *d_count, int32_t *d_slot, int32_t *d_total);
/* the job records of every candidate c = d_slot[i] + k: prediction into piece c (n x n, stride n) from the filtered / unfiltered neighbours as
 * the partition's mask says, residual + forward transform, Rdoq (intra, scan by mode: Global.h:1212-1227), level statistics; d_owner[c] = i */
int havoc_mi355x_intra_expand(havoc_mi355x_ctx *ctx, const havoc_mi355x_intra_search_job *d_parts, const int32_t *d_order, const int32_t *d_count, const int32_t *d_slot,
                              const int32_t *d_ctx_index, int n, int log2TrafoSize, int quant_scale, int quant_shift, int inv_scale, int lambda_q16, int sdh_factor, int sdh,
                              havoc_mi355x_intra_job *d_intra_jobs, havoc_mi355x_tu_fused_job *d_tu_jobs, havoc_mi355x_rdoq_job *d_rdoq_jobs, int32_t *d_stat_jobs,
                              int32_t *d_owner);
/* Search.hpp:143-255: the first candidate with the smallest   mode rate + (1 + (cbf ? 2 * nonzero + sum_abs : 0) << 16) + reciprocal_lambda_q16 * ssd.
 * The RATE here is a stand-in, not the reference's (havoc_mi355x_intra_decide_rated below takes the reference's: havoc_mi355x_intra_rate measures them on the
 * device): the reference's RD stage charges every mode -- candModeList[0] included -- the bits EstimateRateLuma measures in the CABAC state of
 * that moment (prev_intra_luma_pred_flag, mpm_idx / rem_intra_luma_pred_mode, the residual), where this uses the first stage's offsets (rate_a_minus_c is 0 rate for
 * candModeList[0]) and a count of levels.  The order of evaluation, the Q16 arithmetic and the strict comparison are the reference's (pinned with the encoder's own rates:
 * tests/test_trace_pin.py); a caller with an entropy coder supplies real rates through the host form (search/tu_decision.hpp: decideIntraRd with a rate functor);
 * d_final[i] = the champion's tu job with rec_off = i << (2 * log2TrafoSize) (the block it reconstructs into) */
int havoc_mi355x_intra_decide(havoc_mi355x_ctx *ctx, const havoc_mi355x_intra_mpm *d_mpm, const int32_t *d_order, const int32_t *d_count, const int32_t *d_slot,
                              const int32_t *d_cbf, const uint32_t *d_ssd, const int32_t *d_stats, const havoc_mi355x_tu_fused_job *d_tu_jobs, int n, int log2TrafoSize,
                              int32_t reciprocal_lambda_q16, havoc_mi355x_intra_choice *d_out, havoc_mi355x_tu_fused_job *d_final);
/* the records of havoc_mi355x_intra_rate for the candidates havoc_mi355x_intra_expand laid out, one lane per candidate slot: job c = slot c (d_slot[i] + k) with
 * level_off = d_rdoq_jobs[c].dst_off, its ctx_index, scan_idx and sdh, rate_index = c, mpm_idx = the first x with d_order[..][k] == cand_mode_list[x] (3: none) and the
 * launch's flags (HAVOC_INTRA_RATE_*: one size of one kind of unit per launch) */
int havoc_mi355x_intra_rate_jobs(havoc_mi355x_ctx *ctx, const havoc_mi355x_intra_mpm *d_mpm, const int32_t *d_order, const int32_t *d_count, const int32_t *d_slot,
                                 const havoc_mi355x_rdoq_job *d_rdoq_jobs, int n, int flags, havoc_mi355x_intra_rate_job *d_jobs);
/* havoc_mi355x_intra_decide with the rate supplied: cost = d_rates[s] + reciprocal_lambda_q16 * ssd[s] for candidate slot s (havoc_mi355x_intra_rate: mode bits,
 * split_transform_flag, cbf_luma and the residual in their CABAC state, in place of the first stage's offsets and the stand-in).  The reference measures a challenger's
 * rate only when its distortion alone is below the champion's cost (Search.hpp:242-246); rates are never negative, so measuring every candidate and comparing whole
 * costs with `<` in refinement order picks the same champion at the same cost.  The order of evaluation, the count == 0 guard, the final job records and the 40-byte
 * results are havoc_mi355x_intra_decide's.  d_stats may be NULL: nonzero / sum_abs of the results are then 0. */
int havoc_mi355x_intra_decide_rated(havoc_mi355x_ctx *ctx, const havoc_mi355x_intra_mpm *d_mpm, const int32_t *d_order, const int32_t *d_count, const int32_t *d_slot,
                                    const int32_t *d_cbf, const uint32_t *d_ssd, const int32_t *d_stats, const int64_t *d_rates,
                                    const havoc_mi355x_tu_fused_job *d_tu_jobs, int n, int log2TrafoSize, int32_t reciprocal_lambda_q16, havoc_mi355x_intra_choice *d_out,
                                    havoc_mi355x_tu_fused_job *d_final);

/* ---- the transform-tree decision of inter units and the picture's block structure on the device (round 4; csrc/kernels_decide.hip) ----
 * reconstructInter's choice between one transform block and four (turing/Reconstruct.cpp:1296-1428; turingcodec_amd/search/tu_decision.hpp: decideRqt) from the outcomes of a
 * unit's five candidate blocks, evaluated by the caller's chain tu_forward -> rdoq -> tu_reconstruct (into pieces) -> level_stats: the split tree first; none of its blocks
 * coded -> the unit stays unsplit without residual and depth 0 is never considered; else the cheaper of  rate + ssd * reciprocal_lambda  wins, depth 0 on `<` (rate = the
 * stand-in of tu_decision.hpp: (1 + (cbf ? 2 * nonzero + sum_abs : 0)) << 16 per block; havoc_mi355x_rqt_decide_rated below takes the reference's residual bits instead).  Candidate j of size s has its outcome at sizes[s - 2].d_cbf / d_ssd / d_stats [j] and its
 * job at d_jobs[j]; unit i's depth-0 candidate is d_zero_at[i] of its size, its four depth-1 candidates d_one_at[i] .. + 3 of the next smaller size.  d_final[j] = the job that
 * reconstructs candidate j again: into the picture (rec_off = rec_origin + y * rec_stride + x) when it belongs to the chosen tree -- a unit without residual through its four
 * depth-1 blocks -- else at dump_off (any block-sized area of the same allocation nobody reads: the launches after the decision have a fixed size). */
typedef struct { int32_t x0, y0, log2_size, ctx_index; } havoc_mi355x_rqt_unit;                 /* = havoc_rqt_cu */
typedef struct { int32_t cbf; uint32_t ssd; int32_t nonzero, sum_abs; } havoc_mi355x_tu_outcome;   /* = havoc_tu_outcome */
typedef struct { int32_t depth, tried_zero; havoc_mi355x_tu_outcome zero, one[4]; int64_t cost_zero, cost_one; } havoc_mi355x_rqt_choice;      /* 104 bytes; = havoc_rqt_result */
typedef struct { const int32_t *d_cbf; const uint32_t *d_ssd; const int32_t *d_stats; const havoc_mi355x_tu_fused_job *d_jobs; havoc_mi355x_tu_fused_job *d_final; } havoc_mi355x_rqt_size;
int havoc_mi355x_rqt_decide(havoc_mi355x_ctx *ctx, const havoc_mi355x_rqt_unit *d_units, int n, const int32_t *d_zero_at, const int32_t *d_one_at, const havoc_mi355x_rqt_size sizes[4],
                            int64_t rec_origin, intptr_t rec_stride, int32_t dump_off, int32_t reciprocal_lambda_q16, havoc_mi355x_rqt_choice *d_out);
/* The same decision with the residual term supplied: d_rates[s - 2][j] = the Q16 rate of candidate j of transform size s (havoc_mi355x_residual_rate: the reference's
 * bits of its residual_coding) in place of the stand-in; a size with tables has its rates.  Order of evaluation, the uncoded short-cut, the Q16 arithmetic, `cost_zero < cost_one`,
 * the final job records and the 104-byte results are havoc_mi355x_rqt_decide's.  sizes[k].d_stats may be NULL: nonzero / sum_abs of the results are then 0.  With real
 * residual rates the costs still leave out what the reference charges beside them: cbf_luma, split_transform_flag and the chroma residuals of the tree, and weigh luma
 * distortion only; havoc_mi355x_rqt_decide_tree below compares what the reference compares. */
int havoc_mi355x_rqt_decide_rated(havoc_mi355x_ctx *ctx, const havoc_mi355x_rqt_unit *d_units, int n, const int32_t *d_zero_at, const int32_t *d_one_at,
                                  const havoc_mi355x_rqt_size sizes[4], const int64_t *const d_rates[4], int64_t rec_origin, intptr_t rec_stride, int32_t dump_off,
                                  int32_t reciprocal_lambda_q16, havoc_mi355x_rqt_choice *d_out);
/* The reference's own decision over three planes (turing/Reconstruct.cpp:1325-1424): depth 1 first; its rqt_root_cbf 0 -- no level in ANY of Y, Cb, Cr -- leaves the unit
 * unsplit without residual and depth 0 untried; else  cost_d = rate_d + (ssdY + 4 ssdCb + 4 ssdCr) * reciprocal_lambda  with the sum in int32 (StateEncodeSubstream::ssd) and
 * depth 0 winning on cost_zero < cost_one.  rate_d = d_tree_rate[2 * i + d], the whole transform_tree's bits of unit i at depth d, and d_tree_cbf[2 * i + d] its mask, both as
 * havoc_mi355x_tree_rate writes them (out_index = 2 * i + d).  Luma candidates: sizes / d_zero_at / d_one_at as in havoc_mi355x_rqt_decide (d_stats may be NULL).  Chroma
 * candidates: csizes[c - 2] holds the Cb and Cr candidates of chroma transform size c the same way (d_cbf, d_ssd, d_jobs, d_final; d_stats is not read); d_chroma_at[i] says
 * where unit i's are: its depth-0 Cb / Cr candidate in csizes[max(L - 1, 2) - 2], and for L > 3 the first of its four depth-1 Cb / Cr candidates (z-order, one after the
 * other) in csizes[L - 4]; an 8x8 unit's one 4x4 block per component is the same candidate at both depths (cb_one / cr_one are not read).
 *   d_out: havoc_mi355x_rqt_choice as before -- the luma outcomes, depth, tried_zero -- with cost_zero / cost_one the whole-tree costs; havoc_mi355x_block_cells reads it
 * unchanged.  d_tree_out: the masks and the sums ssdCb + ssdCr of both depths (depth 0's are 0 when it was not tried).  d_final of every luma AND chroma candidate: a
 * candidate of the chosen tree goes into the picture (luma: rec_origin + y * rec_stride + x; Cb / Cr: cb_origin / cr_origin + (y / 2) * c_stride + x / 2), every other to
 * dump_off / c_dump_off; a unit left without residual is reconstructed through its depth-1 candidates, whose levels are all zero. */
typedef struct { int32_t cb_zero, cr_zero, cb_one, cr_one; } havoc_mi355x_rqt_chroma_at;     /* 16 bytes */
typedef struct { uint32_t mask_zero, mask_one; int32_t chroma_ssd_zero, chroma_ssd_one; } havoc_mi355x_rqt_tree_choice;     /* 16 bytes */
int havoc_mi355x_rqt_decide_tree(havoc_mi355x_ctx *ctx, const havoc_mi355x_rqt_unit *d_units, int n, const int32_t *d_zero_at, const int32_t *d_one_at,
                                 const havoc_mi355x_rqt_size sizes[4], const havoc_mi355x_rqt_size csizes[4], const havoc_mi355x_rqt_chroma_at *d_chroma_at,
                                 const int64_t *d_tree_rate, const uint32_t *d_tree_cbf, int64_t rec_origin, intptr_t rec_stride, int32_t dump_off,
                                 int64_t cb_origin, int64_t cr_origin, intptr_t c_stride, int32_t c_dump_off, int32_t reciprocal_lambda_q16,
                                 havoc_mi355x_rqt_choice *d_out, havoc_mi355x_rqt_tree_choice *d_tree_out);
/* The same decision for units that OVERLAP one another -- the searched 2Nx2N units of every size of a coding quadtree, each with the tree of its own prediction -- which
 * cannot all be reconstructed into one picture: which of them are is the quadtree's decision.  It writes NO final job record and takes no reconstruction argument:
 * sizes[k].d_final, d_jobs and d_stats (and csizes') may be NULL and are never touched.  For units of log2_size 3..5 d_out and d_tree_out are
 * havoc_mi355x_rqt_decide_tree's on the same tables, byte for byte.  log2_size 6 is accepted: a 64x64 unit lies above MaxTbLog2SizeY, its split is inferred
 * (turing/Reconstruct.cpp:1300-1310) and only its depth-1 candidates exist -- four 32x32 luma blocks at d_one_at[i] .. + 3 of sizes[3], four Cb and four Cr 16x16 blocks at
 * cb_one / cr_one .. + 3 of csizes[2], the rate and mask at d_tree_rate / d_tree_cbf [2 i + 1] (havoc_mi355x_tree_rate at (6, 1)); d_zero_at[i], cb_zero, cr_zero and
 * entry 2 i are not read.  Its record: one[], cost_one, mask_one and chroma_ssd_one as for any unit; tried_zero = 0 and the zero fields 0, as an untried depth 0 is
 * recorded; depth = 1 when mask_one != 0, else 0 -- the "unsplit without residual" record.  (The reference calls this tree rqtdepth 0; it is recorded as the depth that
 * is coded, so that havoc_mi355x_cu_close's d = (depth == 0 && tried_zero) ? 0 : 1 reads the right tree.)  A unit of another size: depth = -1, nothing else.
 * The tables, offsets and indices are trusted; the inputs are never written.  EINVAL: n < 0; null sizes / csizes; with n > 0 a null d_units, d_zero_at, d_one_at,
 * d_chroma_at, d_tree_rate, d_tree_cbf, d_out or d_tree_out; a negative reciprocal_lambda_q16; a size table with one of d_cbf / d_ssd and not the other.  No allocation,
 * no synchronisation, no workspace: capturable into a HIP graph. */
int havoc_mi355x_rqt_decide_units(havoc_mi355x_ctx *ctx, const havoc_mi355x_rqt_unit *d_units, int n, const int32_t *d_zero_at, const int32_t *d_one_at,
                                  const havoc_mi355x_rqt_size sizes[4], const havoc_mi355x_rqt_size csizes[4], const havoc_mi355x_rqt_chroma_at *d_chroma_at,
                                  const int64_t *d_tree_rate, const uint32_t *d_tree_cbf, int32_t reciprocal_lambda_q16, havoc_mi355x_rqt_choice *d_out,
                                  havoc_mi355x_rqt_tree_choice *d_tree_out);
/* the 4x4 cells havoc_mi355x_derive_bs reads, made from the decisions: every unit one inter 2Nx2N prediction unit from list 0 (decoded picture dpb_index0) at the vector d_field
 * (int16 [2][height / 4][width / 4][2]) holds at its origin, coded flags and transform sizes as decided; cells outside the units: no motion coded, qp, tu_log2 = 2 */
int havoc_mi355x_block_cells(havoc_mi355x_ctx *ctx, int width, int height, int qp, int dpb_index0, const int16_t *d_field, const havoc_mi355x_rqt_unit *d_units,
                             const havoc_mi355x_rqt_choice *d_decisions, int n, havoc_mi355x_cell *d_cells);
/* ... the cells of n more units into cells that hold other units' already (a picture decided band by band: havoc_mi355x_block_cells with n = 0 blanks them once) */
int havoc_mi355x_block_cells_add(havoc_mi355x_ctx *ctx, int width, int height, int qp, int dpb_index0, const int16_t *d_field, const havoc_mi355x_rqt_unit *d_units,
                                 const havoc_mi355x_rqt_choice *d_decisions, int n, havoc_mi355x_cell *d_cells);

/* ---- closing an inter coding unit: the CU's own bits and the residual / no-residual decision (csrc/kernels_cu_rate.hip: k_cu_close, k_unit_pred_ssd) ----
 * Search<IfCbf<rqt_root_cbf, transform_tree>>::go (turing/Search.hpp:2362-2568): once the transform tree of an inter coding unit is decided, the reference prices the
 * CU preamble with the values it now knows -- cu_skip_flag, pred_mode_flag, part_mode, rqt_root_cbf (Syntax<coding_unit>, turing/SyntaxCtu.hpp:143-264; writers
 * turing/Binarization.h:283-375 and the generic flag writer) -- turns a merged 2Nx2N unit without residual into a skipped CU, and compares the coded unit with the same
 * unit left at its prediction.  One job = one candidate CU, a lane each.  Preconditions: a P or B slice; transquant_bypass_enabled_flag 0 (cu_transquant_bypass_flag is
 * not coded); no PCM; CuPredMode is MODE_INTER on entry (pred_mode_flag is 0, part_mode takes the inter binarisation).
 * With haveResidual = (the chosen tree's cbf mask != 0) and merged = HAVOC_CU_CLOSE_MERGE_2Nx2N, in the reference's order (all rates Q16, relative to the CU's start):
 *   - the coded candidate: rate = the PU rate + cu_skip_flag(0) + pred_mode_flag(0) + part_mode + rqt_root_cbf(1) unless merged (SyntaxCtu.hpp:251-255) + the tree's
 *     rate; lambdaDistortion = int32(ssdY + ssdCb + ssdCr) * reciprocal_lambda -- the UNWEIGHTED sum reconstructInter returns (turing/Reconstruct.cpp:1427), not the
 *     ssdY + 4 ssdCb + 4 ssdCr the depth decision inside it compares: the reference's quirk, kept;
 *   - !haveResidual and merged: a skipped CU (Search.hpp:2421-2441): contexts AND rate go back to those before the CU -- the PU rate is dropped -- then merge_idx when
 *     MaxNumMergeCand > 1 (priced from the prediction-unit contexts BEFORE the CU), then cu_skip_flag(1); the distortion stays that of the reconstruction;
 *   - !haveResidual, not merged: PU rate + preamble + rqt_root_cbf(0), no tree;
 *   - haveResidual: the unit is priced without residual as well (:2462-2531): merged -> cu_skip_flag(1) + merge_idx from the contexts before the CU; not merged -> the
 *     state after the preamble + rqt_root_cbf(0).  Its lambdaDistortion = lambda * ssdPrediction[0] + lambda * ssdPrediction[1] + lambda * ssdPrediction[2], three
 *     products.  It replaces the coded candidate on cost < cost (strict: equal costs keep the residual), and the coded residual is then dropped.
 * part_mode (Binarization.h:311-375): 2Nx2N one bin 1 at ctxInc 0; else 0 at ctxInc 0, bin (~mode >> 1 & 1) at ctxInc 1, then at log2CbSize == MinCbLog2SizeY a third
 * bin (~mode >> 2 & 1) at ctxInc 2 when log2CbSize > 3 and the mode is not 2NxN -- the reference writes 1 there for NxN as for Nx2N (the standard's NxN has 0): priced
 * as the reference writes it -- and above MinCbLog2SizeY with amp_enabled_flag the bin (~mode >> 2 & 1) at ctxInc 3 and for an AMP mode one bypass bin.
 * The context families are pairwise disjoint (turing/Cabac.h:96-136: prediction unit / cu_skip_flag, pred_mode_flag, part_mode, rqt_root_cbf / the tree's), so the sum
 * of the three rates is the rate of the syntax's interleaved order.
 * d_cu_syntax holds HAVOC_CU_SYNTAX_CTX_BYTES per snapshot, each byte a ContextModel::state (counts: Cabac.h:96-129): */
enum {
    HAVOC_CU_SYNTAX_CTX_SPLIT_CU_FLAG = 0,      /* split_cu_flag [3]: the quadtree step's, passed through */
    HAVOC_CU_SYNTAX_CTX_CU_SKIP_FLAG = 3,       /* cu_skip_flag [3] */
    HAVOC_CU_SYNTAX_CTX_PRED_MODE_FLAG = 6,     /* pred_mode_flag [1] */
    HAVOC_CU_SYNTAX_CTX_PART_MODE = 7,          /* part_mode [4] */
    HAVOC_CU_SYNTAX_CTX_RQT_ROOT_CBF = 11,      /* rqt_root_cbf [1] */
    HAVOC_CU_SYNTAX_CTX_BYTES = 16              /* 12..15 reserved: passed through */
};
enum {
    HAVOC_CU_CLOSE_MIN_CB = 1,          /* log2CbSize == MinCbLog2SizeY */
    HAVOC_CU_CLOSE_AMP = 2,             /* amp_enabled_flag */
    HAVOC_CU_CLOSE_MERGE_2Nx2N = 4      /* PartMode 2Nx2N with merge_flag: rqt_root_cbf is not coded, the unit may become a skipped CU */
};
enum { HAVOC_CU_OUTCOME_REFUSED = -1, HAVOC_CU_OUTCOME_CODED = 0, HAVOC_CU_OUTCOME_NO_RESIDUAL = 1, HAVOC_CU_OUTCOME_SKIPPED = 2 };
typedef struct {
    int32_t ctx_index;          /* the snapshot of d_cu_syntax (16 bytes) the CU starts from */
    int32_t unit_index;         /* i: d_choice[i], d_tree_choice[i], d_tree_rate[2 i + depth], d_pred_ssd[3 i ..] */
    int32_t pu_rate_index;      /* d_pu_rate[..]: the Q16 rate of the CU's prediction units, summed (havoc_mi355x_pu_rate's of the chosen candidates) */
    int32_t pu_before_index;    /* the snapshot of d_pu_before (HAVOC_PU_SYNTAX_CTX_*, 16 bytes) before the CU */
    int32_t pu_after_index;     /* the snapshot of d_pu_after after the CU's prediction units */
    uint8_t log2_cb_size;       /* 3..6 */
    uint8_t part_mode;          /* PartMode: 0 2Nx2N, 1 2NxN, 2 Nx2N, 3 NxN, 4 2NxnU, 5 2NxnD, 6 nLx2N, 7 nRx2N */
    uint8_t skip_ctx_inc;       /* cu_skip_flag's ctxInc, 0..2: the left and upper neighbours' cu_skip_flag summed (Binarization.h:283-295): the caller's */
    uint8_t merge_idx;          /* read with HAVOC_CU_CLOSE_MERGE_2Nx2N */
    uint8_t flags;              /* HAVOC_CU_CLOSE_* */
    uint8_t pad[3];
    int32_t reserved;
} havoc_mi355x_cu_close_job;   /* sizeof: 32 */
typedef struct {
    int32_t outcome;            /* HAVOC_CU_OUTCOME_* */
    int32_t have_residual;      /* the chosen tree's cbf mask != 0 (0 for a refused job) */
    int64_t rate;               /* the winner's: Q16 bits of the whole CU, -1 refused */
    int64_t lambda_distortion;  /* the winner's Q16 lambdaDistortion */
    int64_t cost;               /* rate + lambda_distortion (cost2) */
    int64_t cost_coded;         /* the coded candidate's cost; -1 when the tree has no residual (there is then one candidate only) */
    int64_t cost_no_residual;   /* the cost of the unit left at its prediction (skipped, or rqt_root_cbf 0) */
} havoc_mi355x_cu_choice;      /* sizeof: 48; every int64 is -1 for a refused job */
/* The tree is read where havoc_mi355x_rqt_decide_tree left it: with d = (d_choice[i].depth == 0 && d_choice[i].tried_zero) ? 0 : 1 the chosen tree's mask is
 * d_tree_choice[i].mask_zero / mask_one, its rate d_tree_rate[2 i + d] (read only with a residual), ssdY = zero.ssd or the sum of one[0..3].ssd, ssdCb + ssdCr =
 * chroma_ssd_zero / chroma_ssd_one (a unit left without residual at depth 1 has d = 1 and mask_one = 0).  d_pred_ssd[3 i + c]: SSD(source, prediction) of the unit
 * in plane c (havoc_mi355x_unit_pred_ssd), read only with a residual.
 * A job the syntax cannot code is refused: outcome and every int64 of its record -1, d_cu_syntax_out its input snapshot, d_pu_syntax_out its pu_after snapshot.  That
 * is: a `flags` bit other than HAVOC_CU_CLOSE_*; skip_ctx_inc > 2; log2_cb_size outside 3..6, or 3 without HAVOC_CU_CLOSE_MIN_CB (MinCbLog2SizeY >= 3); part_mode > 7;
 * NxN without HAVOC_CU_CLOSE_MIN_CB or at log2_cb_size 3 (the writer asserts / gives Nx2N's bins); an AMP mode (4..7) with HAVOC_CU_CLOSE_MIN_CB or without
 * HAVOC_CU_CLOSE_AMP (gives 2NxN's / Nx2N's bins); HAVOC_CU_CLOSE_MERGE_2Nx2N with part_mode != 0 or merge_idx >= max_num_merge_cand; pu_rate_index < 0 or a negative
 * (refused) d_pu_rate entry; a residual whose tree rate is negative.  The other indices are trusted.
 * Outputs per job j: d_out[j]; d_cu_syntax_out[16 j ..]: the CU snapshot as the winner left it (the split_cu_flag and reserved bytes as they came); d_pu_syntax_out
 * [16 j ..]: the prediction-unit snapshot as the winner left it (pu_after; for a skipped CU pu_before with merge_idx moved).  Whether the tree's own contexts (the 128-byte
 * and 4-byte snapshots of havoc_mi355x_tree_rate) stand is the outcome: they do only for HAVOC_CU_OUTCOME_CODED.
 * The inputs are never written.  All device pointers 8-byte aligned.  EINVAL: a null pointer; njobs < 0; max_num_merge_cand outside 1..5; a negative lambda; an output
 * that is one of the inputs.  No allocation, no synchronisation, no workspace: capturable into a HIP graph. */
int havoc_mi355x_cu_close(havoc_mi355x_ctx *ctx, const uint8_t *d_cu_syntax, const uint8_t *d_pu_before, const uint8_t *d_pu_after, const int64_t *d_pu_rate,
                          const havoc_mi355x_rqt_choice *d_choice, const havoc_mi355x_rqt_tree_choice *d_tree_choice, const int64_t *d_tree_rate,
                          const int32_t *d_pred_ssd, const havoc_mi355x_cu_close_job *d_jobs, int njobs, int max_num_merge_cand, int32_t reciprocal_lambda_q16,
                          havoc_mi355x_cu_choice *d_out, uint8_t *d_cu_syntax_out, uint8_t *d_pu_syntax_out);
/* ssdPrediction of n units in one launch (turing/Reconstruct.cpp:856 summed over the transform blocks of a unit = SSD(source, prediction) of the unit's block per
 * plane): d_out[3 i + c] for plane c of unit i, accumulated in int32 as the reference does (wrapping).  Unit i is (1 << log2_size)^2 luma samples at d_src_y +
 * src_off[0] (rows src_stride apart) against d_pred_y + pred_off[0] (rows pred_stride apart), and half that size in Cb, Cr at d_src_c + src_off[1], [2] (rows
 * src_stride_c apart) against d_pred_c + pred_off[1], [2] (rows pred_stride_c apart); offsets and strides in samples of 1 (bit_depth 8) or 2 bytes.  log2_size 3..6,
 * sizes mixed freely.  No alignment is asked of offsets or strides (rows are read in unaligned 8-byte pieces); the records are trusted. */
typedef struct { int32_t src_off[3], pred_off[3], log2_size, reserved; } havoc_mi355x_pred_ssd_job;     /* sizeof: 32 */
/* EINVAL: a null pointer, n < 0, a bit depth outside 8..16, a stride that is not positive, d_out one of the inputs.  No allocation, no synchronisation:
 * capturable into a HIP graph. */
int havoc_mi355x_unit_pred_ssd(havoc_mi355x_ctx *ctx, int bit_depth, const void *d_src_y, intptr_t src_stride, const void *d_src_c, intptr_t src_stride_c,
                               const void *d_pred_y, intptr_t pred_stride, const void *d_pred_c, intptr_t pred_stride_c, const havoc_mi355x_pred_ssd_job *d_jobs, int n,
                               int32_t *d_out);
/* The winner's prediction of n searched units in one launch: what go2 leaves behind for reconstructInter (turing/Search.hpp:1829-1842, then :2362-2568 on that
 * prediction).  havoc_mi355x_pu_decide leaves unit u's winner in d_best[u] (0, 1, 2: the first, second, third candidate of the unit -- L0, L1, bi; -1: none), and the
 * candidates' predictions lie as contiguous blocks, candidate k of a unit (1 << 2 * log2) samples behind candidate k - 1 in each plane (log2 = log2_size in luma,
 * log2_size - 1 in Cb and Cr).  Per job: the winner's Y block from d_cand_y + cand_off[0] + (best << 2 log2_size) to d_dst_y + dst_off[0] (rows dst_stride apart), its
 * Cb and Cr blocks from d_cand_c + cand_off[1], [2] + (best << 2 (log2_size - 1)) to d_dst_c + dst_off[1], [2] (rows dst_stride_c apart); offsets and strides in
 * samples of 1 (bit_depth 8) or 2 bytes.  d_unit_cand[unit] = d_first[unit] + best, d_unit_rate[unit] = d_rate[that candidate] (havoc_mi355x_pu_rate's): what
 * havoc_mi355x_cu_close charges as the unit's PU rate.  A unit without a winner (best < 0, or a value above 2, which pu_decide does not write for three candidates):
 * d_unit_rate = d_unit_cand = -1 and NOTHING of it is copied.  log2_size 3..6, sizes mixed freely; destination blocks of different jobs must not overlap.
 * Alignment: none is required of offsets or strides (rows move in unaligned 8-byte pieces, 4-byte pieces for an 8-bit 4x4 chroma block); a caller who keeps every
 * block and plane at a multiple of 8 bytes -- a picture width that is a multiple of 8 with blocks at their picture positions does -- gets one aligned access per
 * piece.  The records are trusted: offsets, log2_size and unit are not checked. */
typedef struct { int32_t cand_off[3], dst_off[3], log2_size, unit; } havoc_mi355x_pred_select_job;     /* sizeof: 32 */
/* The inputs are never written.  EINVAL: a null pointer, n < 0, a bit depth outside 8..16, a stride that is not positive, d_rate or d_unit_rate not 8-byte aligned, an
 * output that is an input or another output.  No allocation, no synchronisation, no workspace: capturable into a HIP graph. */
int havoc_mi355x_unit_pred_select(havoc_mi355x_ctx *ctx, int bit_depth, const void *d_cand_y, const void *d_cand_c, void *d_dst_y, intptr_t dst_stride, void *d_dst_c,
                                  intptr_t dst_stride_c, const int32_t *d_first, const int32_t *d_best, const int64_t *d_rate, const havoc_mi355x_pred_select_job *d_jobs,
                                  int n, int64_t *d_unit_rate, int32_t *d_unit_cand);

/* ---- the coding quadtree of every CTU: split_cu_flag's bits and the full / split decision (csrc/kernels_cqt.hip: k_cqt_decide) ----
 * Search<coding_quadtree>::go (turing/Search.hpp:709-887, the decision :808-886) over Syntax<coding_quadtree>::go (turing/SyntaxCtu.hpp:95-139) and the writer of
 * split_cu_flag (turing/Binarization.h:102-122), for a whole picture in one call.  The candidate coding units are the caller's: closed units as
 * havoc_mi355x_cu_close left them, read in place (outcome, rate, lambda_distortion), and a table that says which record, if any, is the candidate of each node.
 * Geometry: a CTU is a quadtree of L = ctb_log2 - min_cb_log2 + 1 levels and N = 1 + 4 + ... + 4^(L - 1) nodes (1, 5, 21 or 85); node (d, z) -- depth d, z its z-order
 * index among the 4^d nodes of that depth -- has index (4^d - 1) / 3 + z; its children are (d + 1, 4 z + 0..3) in the order upper left, upper right, lower left,
 * lower right.  d_node_cu[c * N + k] is the index in d_choice of node k of CTU c (raster order), or -1: no candidate; an index >= n_choice and a record whose
 * outcome is HAVOC_CU_OUTCOME_REFUSED count as no candidate too.
 * A node at depth d, in the reference's order:
 *   - split_cu_flag is coded only when the node lies wholly inside the picture and is larger than MinCb (SyntaxCtu.hpp:97-102); else it is inferred: 1 for a node
 *     that crosses the picture edge (mustSplit, Search.hpp:810-823: the children are walked, nothing is compared), 0 at MinCb.  One context-coded bin, priced as
 *     measureEncodeDecision, ctxInc = (CtDepth left of (x0, y0) > d) + (CtDepth above (x0, y0) > d), three contexts (turing/Cabac.h:96) nothing else uses.
 *   - else the full candidate from the state before the node: split_cu_flag(0) where coded, then the coding unit (its rate and lambdaDistortion; CtDepth of its cells
 *     becomes d).  It is skipped when the node has no candidate: the reference's testFull == false (:794-806, reached there through rcudepth only), generalised.
 *   - the split is tried when there is no full candidate, or when the node is larger than MinCb and not (HAVOC_CQT_ECU and the full candidate is a skipped CU,
 *     :852-855; Speed::trySplit is always true) and some node below it has a candidate.  That last condition is the reference's testSplit == false (:795-801,
 *     reached there through rcudepth only), generalised like testFull: a caller that has no candidate anywhere below a node has nothing to compare the node's
 *     unit with, and the unit stands (HAVOC_CQT_NODE_NO_SPLIT_CANDIDATE).  It starts again from the state before the node: split_cu_flag(1) where coded, then the four children in z-order,
 *     each from the contexts and CtDepth its predecessor left.  A child whose origin lies outside the picture is a Deleted<coding_quadtree> (SyntaxCtu.hpp:119-135):
 *     no bits, no context, no CtDepth.
 *   - the split replaces the full candidate on cost2() < cost2() (:875; strict: equal costs keep the single CU); the winner's contexts, rate, lambdaDistortion and
 *     CtDepth stand.  The reference compares the costs of the whole CTU so far; both candidates carry the same prefix, so comparing the node's own
 *     rate + lambdaDistortion -- cost_full, cost_split below -- is the same comparison.
 * CtDepth as the snake answers it (Neighbourhood::snake, turing/StateSpatial.h:49-54, read at MinCb / 2 resolution; pinned by tests/cqt_shim.cpp): preCtu resets every
 * entry of the picture's upper row and left column to CtDepth -1 at the slice's first CTU (turing/StatePictures.h:1086-1101), so a neighbour outside the picture --
 * left of column 0, above row 0: no other is ever read -- answers -1 and adds nothing to ctxInc, and so does every neighbour at the picture's first row and column; a
 * neighbour inside the picture answers the depth of the coding unit that covers it, across CTU borders (the upper CTU's lowest cells, the left CTU's rightmost).
 * Between CTUs (StatePictures.h:1042-1075, 1108-1115): with HAVOC_CQT_WPP row r starts from the three contexts after CTU (1, r - 1), or from the slice's
 * (d_cu_syntax) when the picture is one CTU wide; without it row r starts where row r - 1 ended.  One slice, one tile.
 * A CTU is refused when a node at MinCb that the walk reaches has no candidate (an ecu stop always has its candidate, the skipped CU: it cannot lack one): decided = 0,
 * every other field of its record and all its node records 0, its CtDepth cells 0, the contexts leave it as they came.
 * Outputs: d_ctu[c]; d_node[c * N + k]; d_depth: one int8 per MinCb cell, (ctus_y << (L - 1)) rows of (ctus_x << (L - 1)) cells -- whole CTUs; a cell outside the
 * picture is 0; d_cu_syntax_out[16 c ..]: the snapshot after CTU c, bytes HAVOC_CU_SYNTAX_CTX_SPLIT_CU_FLAG .. + 2 moved, the other thirteen d_cu_syntax's. */
enum { HAVOC_CQT_WPP = 1, HAVOC_CQT_ECU = 2 };
enum { HAVOC_CQT_NOT_VISITED = 0, HAVOC_CQT_CU = 1, HAVOC_CQT_SPLIT = 2, HAVOC_CQT_DELETED = 3 };
enum {
    HAVOC_CQT_NODE_FINAL = 1,           /* the node belongs to the decided tree (every ancestor's choice is HAVOC_CQT_SPLIT) */
    HAVOC_CQT_NODE_FLAG_CODED = 2,      /* split_cu_flag was coded (priced), at ctx_inc */
    HAVOC_CQT_NODE_MUST_SPLIT = 4,      /* the node crosses the picture edge */
    HAVOC_CQT_NODE_ECU_STOP = 8,        /* HAVOC_CQT_ECU and a skipped CU: the split was not tried */
    HAVOC_CQT_NODE_NO_CANDIDATE = 16,   /* no full candidate: the split was taken without a comparison */
    HAVOC_CQT_NODE_NO_SPLIT_CANDIDATE = 32  /* a full candidate and no candidate at any node below: the split was not tried */
};
typedef struct {
    int32_t decided;            /* 1; 0: the CTU is refused, or a wait of the call gave up (then EVERY record of the call has 0) */
    int32_t n_cus;              /* coding units of the decided tree */
    int64_t rate;               /* Q16 bits of the CTU's coding quadtree: the units' rates and the coded flags */
    int64_t flag_rate;          /* the coded split_cu_flags of the decided tree alone */
    int64_t lambda_distortion;
    int64_t cost;               /* rate + lambda_distortion */
} havoc_mi355x_cqt_ctu;         /* sizeof: 40 */
typedef struct {
    uint8_t choice;             /* HAVOC_CQT_*: the winner at this node */
    uint8_t flags;              /* HAVOC_CQT_NODE_* */
    uint8_t ctx_inc;            /* read with HAVOC_CQT_NODE_FLAG_CODED */
    uint8_t pad[5];
    int64_t cost_full;          /* the node as one coding unit: split_cu_flag(0) where coded + the unit's rate + lambdaDistortion; -1: not tried */
    int64_t cost_split;         /* split_cu_flag(1) where coded + the four children's winners; -1: not tried */
} havoc_mi355x_cqt_node;        /* sizeof: 24 */
/* d_work: havoc_mi355x_cqt_decide_workspace(n_ctus) bytes, 8-byte aligned: one 64-bit word per CTU -- bit 63 done, bits 0..23 the three context states after it,
 * published with an agent-scope release store once the CTU's CtDepth cells are written -- then the row ticket and the give-up word (int32 each).  The call resets it
 * itself.  Rows are taken by ticket in the order workgroups start; every wait on the row above is bounded, and one that gives up raises the give-up word: every
 * d_ctu record then comes back with decided = 0 and nothing else of the call is to be used.
 * The inputs are never written.  EINVAL: a null pointer; width or height that is not a positive multiple of 1 << min_cb_log2; ctb_log2 outside 4..6; min_cb_log2
 * outside 3..ctb_log2; a flags bit other than HAVOC_CQT_*; n_choice < 0; a workspace that is misaligned or too small; an output that is one of the inputs or another
 * output.  No allocation, no synchronisation: capturable into a HIP graph. */
size_t havoc_mi355x_cqt_decide_workspace(int n_ctus);
int havoc_mi355x_cqt_decide(havoc_mi355x_ctx *ctx, int width, int height, int ctb_log2, int min_cb_log2, int flags, const uint8_t *d_cu_syntax,
                            const int32_t *d_node_cu, const havoc_mi355x_cu_choice *d_choice, int n_choice, void *d_work, size_t work_bytes,
                            havoc_mi355x_cqt_ctu *d_ctu, havoc_mi355x_cqt_node *d_node, int8_t *d_depth, uint8_t *d_cu_syntax_out);

/* ---- acting on the decided quadtree: the final coding units into ONE picture and a per-cell field (csrc/kernels_cqt.hip: k_cqt_commit) ----
 * What the reference's picture holds once Search<coding_quadtree>::go has kept a CTU's winner (turing/Search.hpp:808-886 over :2362-2568): of the searched units --
 * which overlap one another, one per node of every CTU's quadtree -- exactly the FINAL coding units of the decided trees, each as havoc_mi355x_cu_close closed it.
 * Nothing is computed: every sample was made by the calls before (havoc_mi355x_unit_pred_select: the winner's prediction; havoc_mi355x_tu_reconstruct: the
 * candidate pieces of both transform depths); this call selects.  One launch over the n searched units, whatever was decided: a fixed size, capturable.
 * Unit p (d_units[p]; index p means the same unit in every table) is committed exactly when
 *   - its CTU c (raster index of (x0 >> ctb_log2, y0 >> ctb_log2)) has d_ctu[c].decided == 1;
 *   - its node k = (4^d - 1) / 3 + z, d = ctb_log2 - log2_size, z the z-order index of its place in the CTU, has d_node_cu[c N + k] == p;
 *   - d_node[c N + k] has HAVOC_CQT_NODE_FINAL and choice == HAVOC_CQT_CU;
 *   - d_cu[p].outcome is HAVOC_CU_OUTCOME_CODED, _NO_RESIDUAL or _SKIPPED.
 * Every other unit writes nothing.  A unit whose origin or size has no node in the table -- log2_size outside min_cb_log2..ctb_log2, an origin that is negative or not
 * a multiple of its size, a block that leaves the picture -- is skipped, not followed.  The final units of a CTU partition it: no two units write the same sample or cell.
 * What is written, by outcome:
 *   - NO_RESIDUAL, SKIPPED: the unit's block of the prediction planes, three planes: (1 << log2_size)^2 samples at d_pred_y + d_pred_off[3 p] (rows pred_stride
 *     apart), half that size at d_pred_c + d_pred_off[3 p + 1] (Cb) and [3 p + 2] (Cr) (rows pred_stride_c apart): havoc_mi355x_pred_select_job's dst_off;
 *   - CODED: the candidate pieces of the depth that stands, t = (log2_size < 6 && d_choice[p].depth == 0 && d_choice[p].tried_zero) ? 0 : 1 (havoc_mi355x_cu_close's
 *     rule; a 64x64 unit has depth-1 pieces only).  Candidate j of transform size s is the contiguous (1 << s)^2 block at  j << 2 s  samples of luma_pieces[s - 2]
 *     (s = 2..5) or chroma_pieces[s - 2] (s = 2..4), where the unit plan's havoc_mi355x_tu_reconstruct launches leave it.  Luma: t == 0 the piece d_zero_at[p] of size
 *     log2_size, t == 1 the four pieces d_one_at[p] .. + 3 of size log2_size - 1 in z-order.  Cb / Cr: t == 0, or an 8x8 unit (whose one 4x4 block per component
 *     serves both depths), the piece cb_zero / cr_zero of size log2_size - 1; else the four pieces cb_one / cr_one .. + 3 of size log2_size - 2.  A block of the
 *     tree with cbf 0 needs no case of its own: its piece is the clipped prediction.  A piece pointer no committed unit needs may be NULL.
 * Destination: luma at d_rec_y + rec_origin + y * rec_stride + x, Cb / Cr at d_rec_c + cb_origin / cr_origin + (y / 2) * c_stride + x / 2; offsets and strides in
 * samples of 1 (bit_depth 8) or 2 bytes; no alignment is asked of them (rows move in unaligned 8-byte pieces, 4-byte pieces for an 8-bit 4x4 block).
 * d_cells: one record per MinCb cell, (height >> min_cb_log2) rows of (width >> min_cb_log2).  The call first sets the WHOLE map to all-ones bytes (an asynchronous
 * fill), then the wavefront that commits a unit writes the unit's cells.  The samples of an undecided CTU are left as they were and its cells stay all-ones (unit -1);
 * when every `decided` is 0 -- a wait of havoc_mi355x_cqt_decide gave up -- nothing but the fill happens.
 * d_cand_mv: int16 [candidates][2 lists][x, y] in quarter samples, indexed by d_unit_cand[p]; may be NULL: the cells then carry zero vectors.  d_best[p]: 0 L0, 1 L1,
 * 2 bi (havoc_mi355x_pu_decide's). */
typedef struct {
    int32_t unit;        /* index of the coding unit that covers the cell; -1: none (its CTU is undecided) */
    int32_t cand;        /* d_unit_cand[unit]: the winning candidate */
    int16_t mv[2][2];    /* [list][x, y]; a list the mode does not use: 0, 0 */
    uint8_t log2_size;   /* of the coding unit */
    uint8_t outcome;     /* HAVOC_CU_OUTCOME_CODED / NO_RESIDUAL / SKIPPED */
    uint8_t pred;        /* 0 L0, 1 L1, 2 bi */
    uint8_t tr_depth;    /* 0 / 1 of the tree that stands; 0 when nothing is coded */
    uint32_t cbf;        /* the standing tree's mask as havoc_mi355x_rqt_tree_choice records it; 0 unless CODED */
} havoc_mi355x_cqt_cell;   /* sizeof: 24 */
typedef struct {
    int32_t bit_depth;                  /* 8..16 */
    int32_t width, height, ctb_log2, min_cb_log2;       /* havoc_mi355x_cqt_decide's rules */
    int32_t n;                          /* searched units */
    const havoc_mi355x_rqt_unit *d_units;
    const int32_t *d_node_cu;           /* as havoc_mi355x_cqt_decide read it */
    const havoc_mi355x_cqt_ctu *d_ctu;  /* ... and wrote them */
    const havoc_mi355x_cqt_node *d_node;
    const havoc_mi355x_cu_choice *d_cu;
    const havoc_mi355x_rqt_choice *d_choice;
    const havoc_mi355x_rqt_tree_choice *d_tree_choice;
    const int32_t *d_zero_at, *d_one_at;
    const havoc_mi355x_rqt_chroma_at *d_chroma_at;
    const void *luma_pieces[4];         /* transform sizes 2..5 */
    const void *chroma_pieces[3];       /* 2..4 */
    const void *d_pred_y, *d_pred_c;
    intptr_t pred_stride, pred_stride_c;
    const int32_t *d_pred_off;          /* [n][3] */
    const int32_t *d_best, *d_unit_cand;
    const int16_t *d_cand_mv;           /* or NULL */
    void *d_rec_y;
    int64_t rec_origin;
    intptr_t rec_stride;
    void *d_rec_c;
    int64_t cb_origin, cr_origin;
    intptr_t c_stride;
    havoc_mi355x_cqt_cell *d_cells;
} havoc_mi355x_cqt_commit_args;         /* sizeof: 288 (LP64) */
/* The inputs are read in place and never written.  The offsets and indices of the tables are trusted.  EINVAL: null args; a bit depth outside 8..16; geometry
 * havoc_mi355x_cqt_decide refuses; n < 0; a null pointer other than d_cand_mv and the piece pointers; a stride that is not positive; a negative origin; a
 * destination (d_rec_y, d_rec_c, d_cells) that is one of the inputs or another destination; d_cells, d_cand_mv, d_node or d_units not 8-byte aligned.  No allocation, no
 * synchronisation, no workspace: capturable into a HIP graph. */
int havoc_mi355x_cqt_commit(havoc_mi355x_ctx *ctx, const havoc_mi355x_cqt_commit_args *args);

/* ---- the committed cells as the loop filter's block structure (csrc/kernels_cqt.hip: k_cqt_block_cells) ----
 * The translation between havoc_mi355x_cqt_commit's record per MinCb cell and the map of 4x4 havoc_mi355x_cell records havoc_mi355x_derive_bs reads: what
 * LoopFilter::Picture::processCu / processPu / processTu / processRc see of the decided picture (turing/LoopFilter.h:541-737), every coding unit one inter 2Nx2N
 * prediction unit.  Behind it havoc_mi355x_derive_bs, havoc_mi355x_deblock and havoc_mi355x_pad_block leave in the committed planes what TaskDeblock.cpp:105-167
 * leaves before the picture is used for prediction.
 * Writes EVERY cell of the (height / 4) x (width / 4) map, rows cells_stride cells apart, once; the bytes between the rows are not touched.  The 4x4 cell at luma
 * position (x, y) reads q = d_cqt_cells[(y >> min_cb_log2) * (width >> min_cb_log2) + (x >> min_cb_log2)]:
 *   - q.unit < 0 (an undecided CTU: all-ones bytes): mv 0, dpb_index {-1, -1}, flags = HAVOC_CELL_NO_FILTER (the samples are nobody's: the filter leaves them alone),
 *     qp_y = qp, tu_log2 = 2, reserved 0; no other field of q is read;
 *   - otherwise, with size = 1 << q.log2_size, ox = x & (size - 1), oy = y & (size - 1) (a coding unit is aligned to its size):
 *       mv = q.mv, both lists as stored;  dpb_index[0] = q.pred != 1 ? dpb_index0 : -1;  dpb_index[1] = q.pred != 0 ? dpb_index1 : -1;
 *       tu_log2 = min(q.log2_size - q.tr_depth, 5)  (a 64x64 unit: 5 either way -- its split is inferred when coded, and the clamp applies when nothing is);
 *       k = q.tr_depth ? (oy >= size / 2) * 2 + (ox >= size / 2) : 0;  HAVOC_CELL_CODED exactly when q.outcome == HAVOC_CU_OUTCOME_CODED && (q.cbf >> k & 1)
 *       (bits 0..3 of the mask: the luma blocks, as havoc_mi355x_tree_rate documents);  HAVOC_CELL_PU_LEFT when ox == 0, HAVOC_CELL_PU_TOP when oy == 0;
 *       never HAVOC_CELL_INTRA;  qp_y = qp, reserved 0.  cand, unit beyond its sign and the chroma bits of cbf are not read.
 * Argument order: ctx, width, height, min_cb_log2, qp, dpb_index0, dpb_index1, d_cqt_cells (in), d_cells (out), cells_stride.
 * The input is trusted and never written.  EINVAL: a null pointer; min_cb_log2 outside 3..6; a width or height that is not a positive multiple of 1 << min_cb_log2;
 * qp outside 0..51; a dpb index outside 0..127; cells_stride < width / 4; d_cells == d_cqt_cells; d_cqt_cells not 8-byte aligned or d_cells not 16-byte aligned.
 * One launch; no allocation, no synchronisation, no workspace: capturable into a HIP graph. */
int havoc_mi355x_cqt_block_cells(havoc_mi355x_ctx *ctx, int width, int height, int min_cb_log2, int qp, int dpb_index0, int dpb_index1,
                                 const havoc_mi355x_cqt_cell *d_cqt_cells, havoc_mi355x_cell *d_cells, intptr_t cells_stride);

/* ---- the committed cells as the collocated motion store (csrc/kernels_cqt.hip: k_cqt_motion_store) ----
 * The other half of a reference picture: beside the deblocked, padded planes (TaskDeblock.cpp:105-167) the motion the NEXT picture's temporal candidate is derived
 * from (turing/StateCollocatedMotion.h:51-122).  The store is (height + 15) / 16 dense rows of (width + 15) / 16 records -- StateCollocatedMotion's own dimensions --
 * and entry (X, Y) holds the motion of the coding unit that CONTAINS luma sample (16 X, 16 Y): fillRectangle (:75-90) writes every X, Y with x0 <= 16 X < x1 and
 * y0 <= 16 Y < y1, so an 8x8 unit whose origin is no multiple of 16 writes no entry, a 64x64 unit writes sixteen, and -- the final units partition a decided CTU --
 * every entry has one writer.  The sample is inside the picture (width and height are multiples of MinCb, 16 X < width, 16 Y < height).
 * Entry (X, Y) reads q = d_cqt_cells[(16 Y >> min_cb_log2) * (width >> min_cb_log2) + (16 X >> min_cb_log2)]:
 *   - q.unit < 0 (an undecided CTU: all-ones bytes): the whole record is zero ("not available", the reference's default PuData; an intra unit would look the same);
 *     no other field of q is read;
 *   - otherwise pred_flag[0] = q.pred != 1, pred_flag[1] = q.pred != 0; for a used list mv[l] = q.mv[l] and ref_poc[l] = ref_poc0 / ref_poc1, for an unused list
 *     both are 0; long_term = 0, reserved = 0.  cand, outcome, tr_depth, cbf and log2_size are not read.
 * Argument order: ctx, width, height, min_cb_log2, poc (the committed picture's own picture order count), ref_poc0, ref_poc1 (of the pictures behind lists 0 and 1,
 * reference index 0), d_cqt_cells (in), d_store (out).
 * The input is trusted and never written.  EINVAL: a null pointer; min_cb_log2 outside 3..6; a width or height that is not a positive multiple of 1 << min_cb_log2;
 * ref_poc0 == poc or ref_poc1 == poc (a picture does not predict from itself: the derivation would divide by zero); poc - ref_poc0 or poc - ref_poc1 outside
 * -32768..32767 (DiffPicOrderCnt); d_store == d_cqt_cells; either pointer not 8-byte aligned.
 * One launch; no allocation, no synchronisation, no workspace: capturable into a HIP graph. */
typedef struct {
    int16_t mv[2][2];       /* [list][x, y], quarter samples; a list without motion: 0, 0 */
    int32_t ref_poc[2];     /* picture order count of the picture the list's vector points into; 0 without motion */
    uint8_t pred_flag[2];   /* neither: not available (intra, or not coded) */
    uint8_t long_term[2];
    uint32_t reserved;      /* 0 */
} havoc_mi355x_col_cell;    /* sizeof: 24; = ColocatedCell of turingcodec_amd/search/amvp.hpp as plain data */
int havoc_mi355x_cqt_motion_store(havoc_mi355x_ctx *ctx, int width, int height, int min_cb_log2, int poc, int ref_poc0, int ref_poc1,
                                  const havoc_mi355x_cqt_cell *d_cqt_cells, havoc_mi355x_col_cell *d_store);

/* ---- the temporal motion vector candidate of a picture's prediction units (csrc/kernels_temporal.hip: k_temporal_candidates) ----
 * What AMVP (turing/Mvp.h:195-436) and the merge list (:486-716) start from: per prediction unit and list, the candidate derived from the collocated picture's motion
 * store (Mvp.h:44-181; HEVC 8.5.3.2.8 / 8.5.3.2.9).  The rule is deriveTemporalCandidate of turingcodec_amd/search/amvp.hpp -- pinned against the traced reference
 * encoder -- compiled into the kernel as it stands.
 * d_store: havoc_mi355x_col_cell records, rows store_stride records apart, (pic_height + 15) / 16 rows of (pic_width + 15) / 16.  d_pus: havoc_picture_pu[n]
 * (turingcodec_amd/search/search_abi.h; x0, y0, w, h are read, nothing else).  d_out[2 * pu + list], like the search results.
 * For the unit (x0, y0, w, h) and list X towards target_poc[X]:
 *   - the bottom-right cell ((x0 + w) >> 4, (y0 + h) >> 4) is consulted only when (y0 >> ctb_log2) == ((y0 + h) >> ctb_log2), y0 + h < pic_height and
 *     x0 + w < pic_width; else, or when it gives nothing, the centre cell ((x0 + w / 2) >> 4, (y0 + h / 2) >> 4).  No cell outside the store is ever read;
 *   - a cell gives nothing when neither pred_flag is set, or its chosen list is long-term, or -- THIS PROJECT'S OWN RULE -- its chosen list has ref_poc == col_poc
 *     (the reference would divide by zero; no conforming stream has the case).  The chosen list: the only one set; with both, list X when all_backwards, else list 1
 *     when collocated_from_l0, else list 0;
 *   - the vector is taken as it is when col_poc - ref_poc == cur_poc - target_poc[X], else scaled by the two distances (8.5.3.2.7: both clipped to -128..127, the
 *     factor to -4096..4095, the components to -32768..32767);
 *   - a unit that is not inside the picture (x0 < 0, y0 < 0, w <= 0, h <= 0, x0 + w > pic_width or y0 + h > pic_height) has no candidate.
 * A candidate that is not available has mv 0, 0 and source 0.
 * Argument order: ctx, params, d_store (in), store_stride, d_pus (in), n, d_out (out).
 * The inputs are trusted and never written.  EINVAL: a null pointer; n < 0; ctb_log2 outside 4..6; a pic_width or pic_height that is not positive;
 * store_stride < (pic_width + 15) / 16; target_poc[l] == cur_poc; all_backwards or collocated_from_l0 outside 0 / 1; a non-zero reserved word; d_store, d_pus or
 * d_out not 8-byte aligned; d_out == d_store or d_out == d_pus.  n == 0: returns 0 without a launch.
 * One launch; no allocation, no synchronisation, no workspace: capturable into a HIP graph. */
typedef struct {
    int32_t pic_width, pic_height, ctb_log2;
    int32_t col_poc;                /* picture order count of the collocated picture (the store's) */
    int32_t cur_poc;                /* ... of the picture the prediction units belong to */
    int32_t target_poc[2];          /* ... of RefPicList0[0] / RefPicList1[0] of that picture */
    int32_t all_backwards;          /* 0 / 1: every reference picture of the current picture precedes it in output order */
    int32_t collocated_from_l0;     /* 0 / 1: collocated_from_l0_flag */
    int32_t reserved[3];            /* 0 */
} havoc_mi355x_temporal_params;     /* sizeof: 48 */
typedef struct {
    int16_t mv[2];          /* x, y in quarter samples; 0, 0 when not available */
    int16_t available;      /* 0 / 1 */
    int16_t source;         /* 0 none, 1 the bottom-right cell, 2 the centre cell */
} havoc_mi355x_temporal_cand;       /* sizeof: 8 */
int havoc_mi355x_temporal_candidates(havoc_mi355x_ctx *ctx, const havoc_mi355x_temporal_params *params, const havoc_mi355x_col_cell *d_store, intptr_t store_stride,
                                     const void *d_pus, int n, havoc_mi355x_temporal_cand *d_out);

/* ---- the merge candidate lists of a committed picture's final coding units (csrc/kernels_merge.hip: k_cqt_merge_lists) ----
 * For every final coding unit of the picture havoc_mi355x_cqt_commit left, the merge candidate list the reference derives for that unit (turing/Mvp.h:486-716; HEVC
 * 8.5.3.2.2 - 8.5.3.2.5), and the lowest merge index whose candidate IS the unit's committed motion.  The rule is deriveMergeCandidateList of
 * turingcodec_amd/search/merge_list.hpp, fetched by cqtMergeList of the same file -- one text compiled into the kernel and into the host clients.
 * d_cqt_cells: havoc_mi355x_cqt_commit's map, (pic_height >> min_cb_log2) dense rows of (pic_width >> min_cb_log2).  d_pus: havoc_picture_pu[n]
 * (turingcodec_amd/search/search_abi.h; x0, y0, w, h are read, nothing else); index p means the unit the cells call `unit == p`.  d_temporal:
 * havoc_mi355x_temporal_cand[2 * n], index 2 * unit + list, as havoc_mi355x_temporal_candidates wrote it for the same d_pus, or NULL: no temporal candidate
 * (slice_temporal_mvp_enabled_flag 0).  d_out[p] is unit p's record.
 * Unit p = (x0, y0, w, h) is FINAL exactly when w == h == 1 << L with min_cb_log2 <= L <= ctb_log2, x0 >= 0, y0 >= 0, x0 + w <= pic_width, y0 + h <= pic_height, x0 and
 * y0 are multiples of w, and the committed cell at (x0, y0) has unit == p and log2_size == L.  A final unit is one inter 2Nx2N prediction unit (partIdx 0).
 * Its five neighbour positions, in list order: A1 (x0 - 1, y0 + h - 1), B1 (x0 + w - 1, y0 - 1), B0 (x0 + w, y0 - 1), A0 (x0 - 1, y0 + h), B2 (x0 - 1, y0 - 1).  A
 * position gives a neighbour only when neighbourPositionAvailable (turingcodec_amd/search/picture_order.hpp: the picture's edges, a CTU that does not precede this
 * one, the next CTU row, z-order inside the CTU) allows it AND the committed cell there has unit >= 0; no cell is read otherwise, never one outside the map.  A
 * neighbour -- and the unit's own motion, from its origin cell -- is pred_flag[0] = pred != 1, pred_flag[1] = pred != 0, ref_idx 0, mv[l] of a used list, 0, 0 for
 * an unused one.  The temporal candidate is available when either of the unit's two records is: pred_flag[l] = available_l, ref_idx 0, that record's vector (0, 0
 * for a list without).
 * The list: a B slice, one active reference per list, picture order counts ref_poc[0] / ref_poc[1] (compared for equality only, by the combined candidates),
 * Log2ParMrgLevel 2, max_cand 1..5 (MaxNumMergeCand): spatial candidates pruned as the standard names the pairs, B2 only while fewer than four were taken, the temporal
 * candidate, combined bi-predictive candidates, zero candidates.  (The 8x4 / 4x8 restriction cannot apply: the smallest unit is 8x8.)
 * A final unit's record: n_cand = max_cand; cand[0 .. max_cand - 1] the list, the rest zero bytes; n_real = the candidates that are not zero candidates (the
 * derivation's return value); match = the lowest k < n_cand whose candidate equals the unit's own motion -- per list the same pred_flag and, where used, the same
 * ref_idx and vector (PuData::operator==) -- or -1.  Any other unit: an all-zero record with match = -1.  Every record is written once, as eight aligned 8-byte
 * stores; nothing outside d_out[0 .. n - 1] is written.
 * Argument order: ctx, params, d_cqt_cells (in), d_pus (in), n, d_temporal (in, or NULL), d_out (out).
 * The inputs are trusted and never written.  EINVAL: a null pointer other than d_temporal; n < 0; ctb_log2 outside 4..6; min_cb_log2 outside 3..ctb_log2; a pic_width
 * or pic_height that is not a positive multiple of 1 << min_cb_log2; max_cand outside 1..5; a non-zero reserved word; a pointer that is not 8-byte aligned; d_out
 * equal to an input.  n == 0: returns 0 without a launch.
 * One launch; no allocation, no synchronisation, no workspace: capturable into a HIP graph. */
typedef struct {
    int16_t mv[2][2];       /* [list][x, y], quarter samples; a list the candidate does not use: 0, 0 */
    uint8_t pred_flag[2];
    int8_t ref_idx[2];      /* 0 */
} havoc_mi355x_merge_cand;          /* sizeof: 12 */
typedef struct {
    havoc_mi355x_merge_cand cand[5];
    int8_t n_cand;          /* max_cand for a final unit, else 0 */
    int8_t n_real;          /* how many of them are not zero candidates */
    int8_t match;           /* the lowest merge index that carries the unit's committed motion; -1: none */
    uint8_t reserved;       /* 0 */
} havoc_mi355x_merge_list;          /* sizeof: 64 */
typedef struct {
    int32_t pic_width, pic_height, ctb_log2, min_cb_log2;
    int32_t max_cand;               /* 1..5 */
    int32_t ref_poc[2];             /* picture order counts of RefPicList0[0] / RefPicList1[0] */
    int32_t reserved[5];            /* 0 */
} havoc_mi355x_merge_params;        /* sizeof: 48 */
int havoc_mi355x_cqt_merge_lists(havoc_mi355x_ctx *ctx, const havoc_mi355x_merge_params *params, const havoc_mi355x_cqt_cell *d_cqt_cells, const void *d_pus, int n,
                                 const havoc_mi355x_temporal_cand *d_temporal, havoc_mi355x_merge_list *d_out);

/* ---- an intra picture's partitions with their real dependencies (round 4; csrc/kernels_decide.hip) ----
 * A partition predicts from the reconstruction of what precedes it (turing/Reconstruct.cpp:609-615) and takes candModeList from its neighbours' decided modes
 * (turing/CandModeList.h:33-95).  A client that runs the batch chain over the partitions level by level (every partition of a level has all its neighbours final)
 * gets what a level needs from the picture's running state here:
 *   intra_gather: per partition the 4n + 1 reference samples from the reconstruction picture -- a sample is there when it lies inside the picture and the partition
 *     owning its 4x4 cell (d_owner, one int32 per cell) precedes this one in coding order (`index`); HEVC 8.4.4.2.2 fills in the others -- written unfiltered and
 *     [1 2 1]-filtered (turing/IntraReferenceSamples.h:373-421) at the job's nb_off / nbf_off, and cand_mode_list / neighbour_modes of its havoc_mi355x_intra_mpm record
 *     from d_modes (one byte per cell) left of and above it (above only inside the same CTU row);
 *   intra_commit: the champions' blocks (block i = n x n samples at i * n * n, as havoc_search_intra_device leaves them) into the picture, their modes into d_modes. */
typedef struct { int32_t x0, y0, log2, index; } havoc_mi355x_intra_chain_part;        /* 16 bytes */
typedef struct { int32_t pic_width, pic_height, stride, pad, cells_per_row, bit_depth, ctb_log2, strong_intra_smoothing; } havoc_mi355x_intra_chain_layout;      /* 32 bytes;
 * strong_intra_smoothing = the sequence's strong_intra_smoothing_enabled_flag (turing/Encoder.cpp:688 sets it): flat 32x32 blocks then take the bi-linear filter of
 * IntraReferenceSamples.h:382-402 */
int havoc_mi355x_intra_gather(havoc_mi355x_ctx *ctx, int S, const havoc_mi355x_intra_chain_layout *layout, const void *d_rec, const int32_t *d_owner, const uint8_t *d_modes,
                              const havoc_mi355x_intra_chain_part *d_parts, int n, const havoc_mi355x_intra_search_job *d_jobs, void *d_neighbours, havoc_mi355x_intra_mpm *d_mpm);
int havoc_mi355x_intra_commit(havoc_mi355x_ctx *ctx, int S, const havoc_mi355x_intra_chain_layout *layout, void *d_rec, uint8_t *d_modes, const havoc_mi355x_intra_chain_part *d_parts,
                              int n, const void *d_blocks, const int32_t *d_mode, int mode_stride);      /* mode of partition i = d_mode[i * mode_stride]: a plain array (1) or
                                                                                                            havoc_mi355x_intra_choice records (10) */
/* after intra_expand: the candidate slots [d_total[0], capacity) that no partition was given become copies of slot 0's records writing into their own slots, so the chain
 * (intra -> tu_forward -> rdoq -> tu_reconstruct -> level_stats) can run over `capacity` = n * HAVOC_MI355X_INTRA_MAX_ORDER jobs WITHOUT the host waiting for the count */
int havoc_mi355x_intra_fill_spare(havoc_mi355x_ctx *ctx, const int32_t *d_total, int capacity, int log2TrafoSize, havoc_mi355x_intra_job *d_intra_jobs,
                                  havoc_mi355x_tu_fused_job *d_tu_jobs, havoc_mi355x_rdoq_job *d_rdoq_jobs, int32_t *d_stat_jobs, int32_t *d_owner);

/* ---- job tables made on the device from the decided motion field (round 4; csrc/kernels_decide.hip) ----
 * Not reference primitives: the reference builds its prediction calls inline from the vectors it has just decided (predictInter, turing/Search.hpp:1659-1706;
 * searchMergeModes :1754-1768).  A batch client whose searches leave the motion field in device memory (havoc_mi355x_search_picture_uni: d_field) gets the
 * job tables of the next launches here, so nothing of the field crosses the link.  Pictures: the planes of one component lie at multiples of *_plane_elems in
 * ONE allocation -- luma: source, list 0, list 1; chroma: Cb source, list 0, list 1, Cr source, list 0, list 1 -- with *_pad samples of border (>= range + 4). */
typedef struct {
    int32_t pic_width, pic_height;
    int32_t range;                 /* vectors are limited so that a block stays within `range` samples of the picture (LimitFullPelMv: CtbSizeY = 64) */
    int32_t field_cw;              /* cells per row of d_field = (pic_width + 3) / 4 */
    int32_t luma_stride, luma_pad, luma_plane_elems;
    int32_t chroma_stride, chroma_pad, chroma_plane_elems;
    int32_t reserved[2];
} havoc_mi355x_field_layout;       /* 48 bytes */
/* the five spatial merge candidates (HEVC 8.5.3.2.3 positions A1, B1, B0, A0, B2; the vectors of both lists decided there, zero outside the picture; Mvp.h's
 * pruning / temporal candidate are the caller's) of n square units of one size as HavocPredBi jobs in three planes: job 5 * i + k, dst_off = job * size^2
 * (chroma: (size / 2)^2), d_vectors[job][list] = (x, y). */
int havoc_mi355x_merge_jobs(havoc_mi355x_ctx *ctx, const havoc_mi355x_field_layout *layout, const int16_t *d_field, const int32_t *d_x0, const int32_t *d_y0, int n, int log2_size,
                            havoc_mi355x_pred_bi_job *d_luma_jobs, havoc_mi355x_pred_bi_job *d_cb_jobs, havoc_mi355x_pred_bi_job *d_cr_jobs, int16_t *d_vectors);
/* the merge decision of n units from the SATDs of their 5 candidates in three planes (job 5 * i + k): d_cost[5 * i + k] = (min(k + 1, 4) << 16) + (satdY + satdCb + satdCr)
 * * reciprocal_sqrt_lambda_q16 (measurePuCost, turing/Search.hpp:1659-1706, with a stand-in for the CABAC rate of the merge index), d_best[i] = the first of the cheapest. */
int havoc_mi355x_merge_decide(havoc_mi355x_ctx *ctx, const int32_t *d_satd_y, const int32_t *d_satd_cb, const int32_t *d_satd_cr, int n, int64_t reciprocal_sqrt_lambda_q16,
                              int64_t *d_cost, int32_t *d_best);
/* HavocPredUni jobs of n square units at the vector decided for `list` at their origin: plane 0 = luma, 1 / 2 = Cb / Cr (half size, eighth-sample phases) */
int havoc_mi355x_pred_jobs(havoc_mi355x_ctx *ctx, const havoc_mi355x_field_layout *layout, const int16_t *d_field, int list, const int32_t *d_x0, const int32_t *d_y0, int n,
                           int log2_size, int plane, const int32_t *d_dst_off, havoc_mi355x_pred_uni_job *d_jobs);

/* ---- a picture's uni-directional motion searches with the decision loops ON THE DEVICE (csrc/kernels_search.hip) ----
 * The reference runs searchMotionUni (turing/Search.hpp:1317-1355: integer search :2060-2336, sub-sample refinement :2010-2061, 2340-2358) per
 * prediction unit and list through the havoc_sad / havoc_sad_multiref / HavocPredUni / hadamard_satd tables.  Here the same loops (restated in
 * turingcodec_amd/search/decision.hpp, compiled for gfx950) run inside the kernel with those primitives computed by the workgroup's lanes; the
 * picture's PUs are walked in the encoder's order with the dependencies of turingcodec_amd/search/picture_order.hpp (derived predictors,
 * mvPreviousInteger2Nx2N along the CTU row, CTU (x, y) after (x + 1, y - 1): TaskEncodeSubstream.cpp:71-95), one launch per wavefront step.
 * The records are those of turingcodec_amd/search/search_abi.h: d_pus = havoc_picture_pu[] (CTU by CTU), d_ctu_first[ctus + 1],
 * d_out = havoc_search_result[2 * n] (index 2 * pu + list), d_field = int16 [2][height / 4][width / 4][x, y] (the decided vectors),
 * d_work = havoc_mi355x_search_workspace(width, height) bytes.  step_launches = 0: ONE launch, a workgroup per (CTU row, list) that waits in
 * the kernel for the row above to be two CTUs ahead; a wait that does not end gives up (nothing hangs) and leaves a non-zero int32 in the last
 * 4 bytes of d_work: the results are then invalid.  step_launches = 1: one launch per wavefront step (no waiting inside a kernel).
 * d_out_bi (optional, havoc_search_result[2 * n_pus]): the bi-directional refinement of searchBi (Search.hpp:1796-1827) after a PU's two
 * uni-directional searches, unless nPbW + nPbH == 12: list 0 against the prediction from list 1's vector, then list 1 against the prediction
 * from list 0's refined vector (searchMotionBi, Search.hpp:1498-1657: the ideal second predictor clip(2 * source - other prediction) built in LDS,
 * an 11 x 11 integer grid, two sub-sample steps); mv, mvd, mvp_flag, calls and cost_subpel (= the cost) are filled.  Nothing of the refinement
 * feeds the walk (the motion field keeps the uni-directional vectors), so it is two more launches after it -- a workgroup per PU, list 0 then list 1.  d_phase: the 16 fractional-sample planes of each reference picture
 * (havoc_mi355x_interp_planes; plane 0 = the picture), which must reach ctb_size + 20 samples beyond the picture on every side; origins are the
 * sample offsets of sample (0, 0).  Everything stays on the device: nothing is uploaded or downloaded by this call.
 * The SOURCE plane d_src is read in whole CTUs (the kernel stages a CTU's ctb_size x ctb_size source block with 16-byte loads): when the picture's width / height are
 * not multiples of ctb_size it must be READABLE up to the next multiple -- i.e. own a border of at least ctb_size - 8 samples to the right and below (the picture store's
 * planes have 96; the values there reach no result: only samples inside a prediction unit are measured). */
typedef struct
{
    int32_t pic_width, pic_height, ctb_size, concurrent_frames;
    int32_t met, small_search_window, bi_small_search_window, half_pel, quarter_pel;
    int32_t bit_depth;
    double reciprocal_sqrt_lambda;
} havoc_mi355x_search_params;      /* 48 bytes; = havoc_search_params */
/* n INDEPENDENT searches (searchMotionUni per record) in ONE launch, a workgroup per search: d_pus = havoc_search_pu[n] (search_abi.h: geometry, the two
 * predictors and their rates, the previous 2Nx2N vector -- inputs here, not derived), one reference picture (d_ref / d_phase), d_out =
 * havoc_search_result[n].  The PUs must lie inside the picture with w, h multiples of 4 in 4..64 and the planes must reach ctb_size + 20 samples beyond it. */
int havoc_mi355x_search_motion_uni(havoc_mi355x_ctx *ctx, int S, const havoc_mi355x_search_params *params, const void *d_src, int64_t src_origin, intptr_t src_stride,
                                   const void *d_ref, int64_t ref_origin, intptr_t ref_stride, const void *d_phase, intptr_t plane_elems, int64_t phase_origin,
                                   const void *d_pus, int n, void *d_out);
/* n INDEPENDENT bi-directional refinements (searchMotionBi, turing/Search.hpp:1498-1657) in ONE launch, a workgroup per refinement: list
 * d_pus[i].ref_list's vector is refined around d_start[2 * i .. 2 * i + 1] (quarter samples) against the prediction the OTHER list's vector d_pus[i].mv_other
 * gives (read from d_phase_other, the other reference picture's 16 phase planes); d_ref / d_phase = the refined list's picture.  d_out[i]: mv, mvd, mvp_flag,
 * calls, cost_subpel (= the cost).  The list form of the refinement launches of havoc_mi355x_search_picture_uni; mvp_rate[] >= 0. */
int havoc_mi355x_search_motion_bi(havoc_mi355x_ctx *ctx, int S, const havoc_mi355x_search_params *params, const void *d_src, int64_t src_origin, intptr_t src_stride,
                                  const void *d_ref, int64_t ref_origin, intptr_t ref_stride, const void *d_phase, intptr_t plane_elems, int64_t phase_origin,
                                  const void *d_phase_other, int64_t phase_other_origin, const void *d_pus, const int16_t *d_start, int n, void *d_out);
size_t havoc_mi355x_search_workspace(int width, int height);
int havoc_mi355x_search_picture_uni(havoc_mi355x_ctx *ctx, int S, const havoc_mi355x_search_params *params, const int64_t mvp_rate[2], const void *d_src,
                                    int64_t src_origin, intptr_t src_stride, const void *d_ref, const int64_t ref_origin[2], intptr_t ref_stride, const void *d_phase,
                                    intptr_t plane_elems, const int64_t phase_origin[2], const void *d_pus, const int32_t *d_ctu_first, int ctus_x, int ctus_y,
                                    int n_pus, void *d_out, void *d_out_bi, int16_t *d_field, void *d_work, int step_launches);
/* Searching into reference pictures that are STILL ARRIVING (the reference: turing/TaskEncodeSubstream.cpp:71-95 -- a CTU starts when its reference picture is
 * reconstructed three CTU rows below it; TaskDeblock.cpp:151-167 publishes the deblocked, padded rows).  d_rows_ready = two device int32: entry l = how many luma rows
 * of reference list l, counted from picture row 0, are final in d_ref AND in all 16 planes of d_phase -- raised (never lowered) by whatever delivers the picture, on
 * ANOTHER stream, while the search kernel runs; the last band raises it to at least pic_height + ctb_size + 8 (bottom border included).  The havoc_mi355x_search_picture_uni
 * launches of this context that follow make CTU row r of list l wait until d_rows_ready[l] >= min((r + 2) * ctb_size, pic_height + ctb_size + 8): with
 * concurrent_frames > 1 (required) the search limits a CTU row's vectors to blocks that end above row (r + 2) * ctb_size - 15 (the reference's LimitFullPelMv), so
 * nothing below is read for a result.  Results are those of the ungated call.  A wait that outlasts ~4 s gives up (HAVOC_MI355X_EDEVICE from the next sync of the
 * caller).  d_rows_ready = NULL removes the gate.  The delivering stream must make its writes visible before it raises the counter (a kernel boundary does), and it
 * must be able to RUN while the search kernel waits: HIP multiplexes the streams of one priority onto GPU_MAX_HW_QUEUES hardware queues (default 4), and a waiting kernel
 * blocks what is queued behind it -- give the delivering stream another priority (hipStreamCreateWithPriority: fine for a few such streams; the high-priority pool is
 * small) or, for many, raise GPU_MAX_HW_QUEUES to about the device's two dozen and keep one priority (bench.py --vr-bands; profiles/r05/banded_pipeline.txt). */
int havoc_mi355x_search_gate(havoc_mi355x_ctx *ctx, const int32_t *d_rows_ready);
/* The TEMPORAL motion vector candidate in the picture search's predictor derivation (turing/Mvp.h:195-436 consults it where the two spatial predictors A and B do not
 * already give two different ones; turingcodec_amd/search/picture_order.hpp: derivePredictors hands it to deriveAmvp).  d_cands = havoc_mi355x_temporal_cand[2 * n_pus]
 * on the device, index 2 * pu + list: the layout havoc_mi355x_temporal_candidates writes for the same d_pus -- the vector is used as written there (already scaled to the
 * target picture's distance; nothing is scaled or clamped here), `available` == 0 means no candidate, `source` is not read.  The havoc_mi355x_search_picture_uni launches
 * of this context that follow read d_cands[2 * pu + list] once per (unit, list) -- both step_launches forms, with or without d_out_bi (the refinement runs with the
 * predictors the uni-directional search ran with, so it follows) -- and must be called with the same n_pus: another count is HAVOC_MI355X_EINVAL there.  The records must
 * be complete in stream order before the search is launched.  d_cands = NULL removes the table: the searches are then, launch for launch and byte for byte, those without
 * this call (kernels compiled without the table).  HAVOC_MI355X_EINVAL for d_cands != NULL with n_pus <= 0 and for a pointer that is not 8-byte aligned.  The table is read,
 * never written; the call allocates nothing, launches nothing and synchronises nothing, so it can be made while a stream is being captured.  Independent of
 * havoc_mi355x_search_gate: either, both or neither may be set.
 * Any int16 components are safe: a predictor is only read FROM after LimitFullPelMv limited it to the picture's surroundings (decision.hpp: fullPel; the kernel's
 * window staging restates it), so no sample is read outside the ctb_size + 20 the planes own; unlimited it enters only the mvd arithmetic, whose int16 wrap-around is
 * the same text on host and device.  The launch + host-replay client (libhavoc_search.so: havoc_search_picture_uni) does not know the table. */
int havoc_mi355x_search_temporal(havoc_mi355x_ctx *ctx, const havoc_mi355x_temporal_cand *d_cands, int n_pus);
/* The PRODUCER's side of the same rule (turing/TaskDeblock.cpp:151-167 deblocks and publishes a picture's rows while the rows below are still being encoded): a launch on
 * THIS context's stream that ends when CTU rows 0 .. ctu_row of both lists of the havoc_mi355x_search_picture_uni running over d_work (its workspace; one-launch form) on
 * ANOTHER stream are done -- whatever is queued behind it (the band's predictions, transform trees, deblocking, padding, the counter a dependent picture's search_gate
 * polls) runs while the rows below are searched.  The two streams must not share a hardware queue (give them different priorities).  The workspace must have been zeroed
 * since the previous picture before anything waits on it.  A wait that outlasts ~8 s, or a search that gave up, sets *d_gave_up and lets the stream through. */
int havoc_mi355x_search_wait_rows(havoc_mi355x_ctx *ctx, const void *d_work, int pic_width, int pic_height, int ctu_row, int32_t *d_gave_up);

#ifdef __cplusplus
}
#endif
#endif
