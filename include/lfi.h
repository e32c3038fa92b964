/*
 * lfi.h — C-ABI of the MI355X light-field interpolation hot path (liblfi_hip.so).
 *
 * This is the drop-in boundary for the reference's device-facing call sites: everything
 * `Interpolator` (reference src/interpolator.cu) does through the CUDA runtime — surface allocation and upload,
 * cudaMemcpyToSymbol of the parameter block, the four kernel launches, event timing, download — is replaced by
 * the calls below.  Plain pointers and sizes only; no C++/torch types.  Each entry point cites the reference lines
 * it replaces (paths relative to the reference repository root).
 *
 * Conventions
 *  - every function returns 0 on success or a negative LFI_E* code; lfi_last_error() returns the message
 *    (the reference checks no CUDA return code at all: src/interpolator.cu:291-292);
 *  - one context per GPU, used from one thread at a time; work is enqueued on the context's HIP stream and is
 *    asynchronous unless stated otherwise;
 *  - images, views and maps are tightly packed RGBA8 planes (row pitch = width*4 bytes) — the linear-HBM
 *    replacement of the reference's cudaArray surfaces; image id g = col*rows + row (src/interpolator.cu:106-113);
 *  - there is no CPU fallback: a missing GPU or code object is an error.
 */
#ifndef LFI_H
#define LFI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LFI_ABI_VERSION 1

typedef struct lfi_ctx lfi_ctx;

typedef struct lfi_int2 { int32_t x, y; } lfi_int2;
typedef struct lfi_float2 { float x, y; } lfi_float2;

/* error codes */
enum {
    LFI_OK = 0,
    LFI_EINVAL = -1,    /* bad argument / call order */
    LFI_EHIP = -2,      /* a HIP runtime call failed */
    LFI_ENODEVICE = -3, /* no usable gfx950 device */
    LFI_ENOMEM = -4
};

/* interpolation methods: the reference's -m strings (src/interpolator.cu:274,282; src/main.cpp:20-22) */
enum {
    LFI_METHOD_STD = 0,    /* "STD":    exact-fp32 ordered FMA chain, RN-even quantisation (src/kernels.cu:289-343) */
    LFI_METHOD_TEN_WM = 1  /* "TEN_WM": fp16 matrix-core contraction, truncating quantisation (src/kernels.cu:345-462) */
};
#define LFI_KERNEL_FOCUS_ESTIMATE 2 /* not a render method: selects variants of FocusMap::estimate in lfi_set_variant */

/* lfi_params.flags */
enum {
    /* By default all-focus renders read the focus maps the reference's kernels read: Standard::process the filtered map 1
     * (src/kernels.cu:326), Tensors::process the unfiltered map 0 (src/kernels.cu:430) — an inconsistency of the reference
     * (SURVEY.md defect D7) that is reproduced so that outputs match it.  With this flag both methods read map 1. */
    LFI_FLAG_UNIFIED_FOCUS_MAP = 1u,
    /* TEN_WM debug numerics: re-round the accumulator to fp16 after every 16-image batch — the reference's half-accumulator WMMA model
     * (wmma::mma_sync with half fragments, src/kernels.cu:418-447; oracle model M16) instead of one final rounding.  Byte for byte the
     * oracle's M16 since round 5: the sums of a batch are formed exactly (fp64 on the vector pipe, one pixel per lane) and rounded once.
     * A debug mode: two orders of magnitude slower than the matrix-core kernels. */
    LFI_FLAG_TEN_ROUND_PER_BATCH = 2u,
    /* Fixed-focus launches over the planar input copy alternate their sweep direction from launch to launch, so that the input rows
     * one launch read last — still in the 256 MB Infinity Cache — are the first the next launch reads (repeated renders of one light
     * field: the reference's 100-launch loop, trajectory blocks, focus sweeps).  With this flag every launch walks the image in
     * ascending order, as a single cold launch does.  Results are identical either way. */
    LFI_FLAG_SINGLE_SWEEP_DIRECTION = 4u,
    /* STD through the band method (fp16 matrix-core sum, exact fmaf chain only for sums near x.5): size the band with the ANALYTIC
     * bound on the matrix core's accumulation error (one whole fp16-product ulp per addend, true of any accumulator that keeps ≥ 24
     * bits even if every addition truncated) instead of the bound measured on gfx950 (a quarter ulp per addend; asserted by
     * tests/test_gpu_parity.py::test_mfma_f16_accumulation_error_bound over 800 adversarial operand sets).  Same bytes, more sums
     * recomputed.  Light fields of up to 64 images use the analytic band BY DEFAULT since round 4 (it costs nothing there); with more
     * images (15x15 grids) it doubles the launch time (tools/std_band_cost.py), so there it stays opt-in, for callers who do not want
     * bit-exactness to rest on a measured property of the hardware. */
    LFI_FLAG_STD_ANALYTIC_BAND = 8u,
    /* Up to 64 images: the band of the measured bound (rounds 2-3's default) instead of the analytic one.  Same bytes. */
    LFI_FLAG_STD_MEASURED_BAND = 16u,
    /* Test hook of the band's self-check (lfi_std_band_info): behave as if the device had FAILED the measurement the measured bound
     * rests on — STD launches over more than 64 images then take the analytic band.  Same bytes. */
    LFI_FLAG_STD_BAND_PROBE_FAIL = 32u,
    /* DEEP VIEWS: fixed-focus renders keep TEN bits per channel straight from the blend's accumulator, on the device, beside the 8-bit views.
     * A view is a weighted mean of 64-225 input bytes accumulated in fp32; the mean carries more than 8 bits, and carries them where banding
     * shows (the smooth out-of-focus gradients of a fixed-focus refocus).  While the flag is set, lfi_render / lfi_prepare / lfi_benchmark with
     * all_focus = 0 launch ONE kernel (csrc/hip/deep_blend.hpp; lfi_last_kernel_name names it, lfi_set_variant choices do not apply) that
     * writes, from one gather and one accumulation per pixel and view:
     *  - the 8-bit views, exactly as a render without the flag defines them (STD: the reference's bytes; TEN_WM: the TEN_WM contract,
     *    floor(min(fp16_RN(s), 255)));
     *  - the DEEP PLANES: [view][3: R,G,B][rows][pitch16] little-endian u16, the code in bits 9..0, the upper six bits 0, pitch16 = 2*W rounded
     *    up to 128 bytes, view = the view's index.  With s the accumulator of (pixel, view, channel):
     *        STD     s = the reference's ordered fp32 fmaf chain (src/kernels.cu:292-299):  D10 = min(1023, rn_even(4*s)) - 4*s is exact in
     *                fp32 and rn_even is the rounding the byte uses: the code is bit-exact;
     *        TEN_WM  s = the fp32-accumulated matrix-core sum:  D10 = min(1023, floor(4*fp16_RN(s))) - the TEN_WM quantisation with two more
     *                bits kept; monotone, and D10 >> 2 IS the 8-bit byte of the same launch.
     * The planes belong to the context (one allocation for all views, counted in lfi_memory.views_bytes, LFI_POISON_DEEP).  lfi_prepare allocates
     * them; otherwise the FIRST deep render does, and that render may block (an allocation; after a change of size the stream is drained
     * first) - a prepared render is only a launch.  They are released wherever the views are.  They hold views [v0, v1) of the last deep launch
     * and are dropped (LFI_YUV_DEEP downloads refused until the next deep render) by any launch that writes views without the flag and by
     * lfi_set_grid, lfi_set_output_layout, lfi_set_row_window, lfi_attach_views and a lfi_set_params that changes the number of views.  They
     * leave the device through lfi_download_views_yuv with a LFI_YUV_DEEP format (below): 10-bit video, or raw gbrp10le planes.
     * Valid: fixed focus; LFI_LAYOUT_PLANAR_RGB; grids up to LFI_MAX_IMAGES images, any number of views, any view range; the kernel reads the
     * derived planar copy of the inputs, so it also serves a context after lfi_release_inputs.
     * LFI_EINVAL with a message that names LFI_FLAG_DEEP_VIEWS, the context usable and nothing written, while the flag is set: all_focus = 1;
     * lfi_render_stream and lfi_render_stream_yuv420; per-view rows (lfi_set_view_offsets, lfi_set_view_float_offsets); a row window; the RGBA
     * view layout; LFI_FLAG_TEN_ROUND_PER_BATCH; lfi_download_prequant; weights outside [0, 2); inputs or offsets the planar copy cannot serve
     * (an attached grid without lfi_grid_modified; after lfi_release_inputs, offsets beyond the copy's padding).
     * Out of scope: all-focus and per-view deep renders, deep quilts / native images / lfi_compare_view[s], a row window, 16-bit PNG. */
    LFI_FLAG_DEEP_VIEWS = 64u,
    /* IN-FRAME BLENDING: a fixed-focus render takes image g at pixel + focused_offsets[g] and, by default, clamps that position to the frame
     * (the reference's surf2Dread(..., cudaBoundaryModeClamp), src/kernels.cu:119-126), which smears each image's edge column or row across a
     * band as wide as its shift.  With this flag the samples that fall outside their image are LEFT OUT and the rest are scaled back to the
     * full weight.  While it is set, lfi_render / lfi_prepare / lfi_benchmark with all_focus = 0 launch ONE kernel (csrc/hip/blend_inframe.hpp;
     * lfi_last_kernel_name names it, lfi_set_variant choices do not apply) that defines view v, channel c, pixel (x, y) as follows - images
     * g = 0 ... N-1 in ascending order, w_g the view's fp16 weight widened to fp32, (ox_g, oy_g) = focused_offsets[g]:
     *      in_g  = 0 <= x + ox_g < W  and  0 <= y + oy_g < H
     *      wall  = fp32 chain  wall <- wall + w_g            over all g
     *      den   = fp32 chain  den  <- den  + w_g            over the g with in_g
     *      num_c = the method's sum of w_g * px_g,c          over the g with in_g
     *              STD:    the ordered chain num <- fmaf(px, w_g, num), the reference's (src/kernels.cu:292-299), skipping the others
     *              TEN_WM: the fp32-accumulated matrix-core sum with the left-out samples as zeros
     *      den == 0:  s_c = 0          (no image has the pixel in frame, or only zero weights do)
     *      otherwise: r = wall / den   (IEEE fp32 division, round to nearest even),  s_c = num_c * r  (one fp32 multiplication, RN)
     *      byte_c = STD: rn_even(s_c) & 0xff      TEN_WM: floor(min(fp16_RN(s_c), 255))   - the epilogues of the two methods
     *  - Where every image has the pixel in frame, den is wall bit for bit, r = 1.0 and the byte is the flag-free render's: STD the reference's
     *    byte, TEN_WM a byte under the TEN_WM contract.
     *  - den, wall and r are the same bits under both methods: the vector pipe forms them in ascending g under both.  Only num carries the
     *    matrix core's accumulation error (a denominator summed on the matrix cores would carry it too, and at den = 0.2 ... 1 the byte would
     *    then be open to three and more values; with the deterministic den it is open to two at the most).
     * The output is ordinary 8-bit views: downloads, YUV frames, quilts, native images, lfi_compare_view[s] and RGB-D work on them unchanged.
     * Without the flag no byte and no launch changes.  A launch with the flag drops the deep views of an earlier deep render.
     * Valid: fixed focus; LFI_LAYOUT_PLANAR_RGB; grids up to LFI_MAX_IMAGES images, any number of views, any view range; the kernel reads the
     * derived planar copy of the inputs (lfi_prepare builds it: a prepared render is only a launch), so it also serves a context after
     * lfi_release_inputs.
     * LFI_EINVAL with a message that starts "LFI_FLAG_IN_FRAME is set: ", the context usable and nothing written or allocated, while the flag is
     * set: all_focus = 1; lfi_render_stream and lfi_render_stream_yuv420; per-view rows (lfi_set_view_offsets, lfi_set_view_float_offsets); a
     * row window; the RGBA view layout; LFI_FLAG_TEN_ROUND_PER_BATCH; LFI_FLAG_DEEP_VIEWS set together with it; lfi_download_prequant; weights
     * outside [0, 2); inputs or offsets the planar copy cannot serve (an attached grid without lfi_grid_modified; after lfi_release_inputs,
     * offsets beyond the copy's padding).
     * Out of scope: all-focus and per-view in-frame renders, the RGBA layout, row windows (and the program's -g above 1), the streaming calls,
     * deep in-frame views, a validity mask taken from the inputs' alpha. */
    LFI_FLAG_IN_FRAME = 128u,
    /* LINEAR-LIGHT BLENDING: a view is a weighted mean of 64-225 samples, and by default that mean is taken over the input BYTES, which are
     * gamma-encoded (sRGB images, or video expanded by the YUV paths).  A synthetic-aperture refocus sums light, and a mean of encoded values is
     * not the encoding of the mean of the light: out-of-focus regions come out too dark and bright points shrink.  With this flag every sample is
     * DECODED to linear light before the sum and the sum is ENCODED afterwards.  While it is set, lfi_render / lfi_prepare / lfi_benchmark with
     * all_focus = 0 launch ONE kernel (csrc/hip/blend_linear.hpp; lfi_last_kernel_name names it, lfi_set_variant choices do not apply) that
     * defines view v, channel c, pixel (x, y) from two tables (csrc/linear_light.h holds them as literal bit patterns, generated once; these
     * formulas are their specification):
     *      eotf(u) = u / 12.92 for u <= 0.04045, else ((u + 0.055) / 1.055)^2.4                      (IEC 61966-2-1)
     *      D[b] = fp16_RN(255 * eotf(b / 255)),          b = 0 ... 255     (D[0] = 0, D[255] = 255)
     *      T[b] = fp32_RN(255 * eotf((b - 0.5) / 255)),  b = 1 ... 255     (the linear value whose encoding is exactly b - 0.5)
     *    No D[b] is nearer than 1.1e-6 (relative) to an fp16 rounding tie and no T[b] nearer than 2.1e-10 to an fp32 tie, so any correctly
     *    working pow gives the same bits.  Both tables increase strictly; T[b] <= D[b] < T[b+1] for every b, so decoding and encoding one
     *    byte is the identity; every D[b] lies at least 0.46 of its bin's width from either edge.
     *      s_c    = the method's sum of w_g * D[px_g,c] over the images g = 0 ... N-1, w_g the view's fp16 weight, px_g,c the samples of a
     *               flag-free fixed-focus render: image g at pixel + focused_offsets[g], clamped to the frame
     *               STD:    the ordered fp32 chain s <- fmaf(float(D[px]), w_g, s), g ascending.  An fp16 times an fp16 is exact in fp32
     *                       (22 bits), so each link is one fp32 addition of an exact product
     *               TEN_WM: the fp32-accumulated matrix-core sum; the operands are D[px] and the fp16 weights as given
     *      byte_c = E(s_c) = #{ b in 1 ... 255 : T[b] <= s_c },   alpha 255
     *    E is monotone, saturates at 255 and is the same under both methods: they differ only in how s is accumulated.
     *  - STD bytes are fully determined.
     *  - TEN_WM bytes lie in [E(max(0, S - eps)), E(S + eps)], S the exact sum (it fits a double) and eps the analytic accumulation bound of
     *    the STD band (LFI_FLAG_STD_ANALYTIC_BAND): 2^-15 per addend times k_pad addends.  That bound rests only on the partial sums staying
     *    below 512 and on exact products; both hold here.
     *  - A weight row with a single 1.0, or with two weights of 0.5, is exact in fp32 in any order: such rows give the same bytes under both
     *    methods, and a one-hot row returns the input image's own bytes.
     * The output is ordinary 8-bit views: downloads, YUV frames, quilts, native images, lfi_compare_view[s] and RGB-D work on them unchanged.
     * Without the flag no byte, launch or message changes.  A launch with the flag drops the deep views of an earlier deep render.
     * Valid: fixed focus; LFI_LAYOUT_PLANAR_RGB; grids up to LFI_MAX_IMAGES images, any number of views, any view range; the kernel reads the
     * derived planar copy of the inputs (lfi_prepare builds it: a prepared render is only a launch; lfi_benchmark builds it before its first
     * timed launch), so it also serves a context after lfi_release_inputs.
     * LFI_EINVAL with a message that starts "LFI_FLAG_LINEAR_LIGHT is set: ", the context usable and nothing written or allocated, while the flag
     * is set: all_focus = 1; lfi_render_stream and lfi_render_stream_yuv420; per-view rows (lfi_set_view_offsets, lfi_set_view_float_offsets); a
     * row window; the RGBA view layout; LFI_FLAG_TEN_ROUND_PER_BATCH; LFI_FLAG_DEEP_VIEWS or LFI_FLAG_IN_FRAME set together with it;
     * lfi_download_prequant; weights outside [0, 2); inputs or offsets the planar copy cannot serve (an attached grid without
     * lfi_grid_modified; after lfi_release_inputs, offsets beyond the copy's padding).
     * Out of scope: all-focus and per-view linear renders; linear light together with in-frame blending or deep views (10 bits of a linear
     * sum); the RGBA layout, row windows (and the program's -g above 1), the streaming calls; other transfer functions (BT.1886, PQ, HLG); a
     * linear-light focus estimate; linear-light resizing in the quilt and native-image kernels. */
    LFI_FLAG_LINEAR_LIGHT = 256u
};

#define LFI_MAX_IMAGES 256     /* MAX_IMAGES, src/kernels.cu:60 */
#define LFI_MAX_FOCUS_IDS 32   /* FOCUS_MAP_IDS_COUNT, src/kernels.cu:68 */
#define LFI_REFERENCE_VIEWS 64 /* VIEW_TOTAL_COUNT, src/kernels.cu:11-13 (a runtime parameter here) */

/*
 * The reference's __constant__ parameter block (src/kernels.cu:15-17, 63-69) as one struct.  All pointers are HOST
 * pointers; lfi_set_params copies what they point to.  The host code above this ABI computes these values
 * (lfinterpolator_amd/csrc/host: same arithmetic as src/interpolator.cu:139-246) so every backend sees identical bytes.
 */
typedef struct lfi_params {
    int32_t views;                    /* V: number of output views / rows of the weight matrix */
    const lfi_int2 *focused_offsets;  /* [N] round(offset*focus): focusedOffsets, src/interpolator.cu:241-244 */
    const lfi_float2 *offsets;        /* [N] offsets, src/interpolator.cu:240,245 */
    const uint16_t *weights_fp16;     /* [V][N] IEEE binary16 bit patterns, row-major: src/interpolator.cu:211-223 */
    const int32_t *focus_map_ids;     /* [n_focus_ids] focusMapIDs, src/interpolator.cu:203-206 (may be NULL if 0) */
    int32_t n_focus_ids;              /* ≤ LFI_MAX_FOCUS_IDS */
    float focus;                      /* inFocus, src/interpolator.cu:152 */
    float range;                      /* inRange, src/interpolator.cu:153 */
    int32_t block_radius[2];          /* constants[9..10], src/interpolator.cu:142-150 */
    uint32_t flags;                   /* LFI_FLAG_* (bit 31 is reserved for the library and ignored) */
} lfi_params;

typedef struct lfi_bench_stats {
    int32_t runs;
    float mean_ms;   /* mean of per-launch event times — what the reference prints (src/interpolator.cu:270-295) */
    float median_ms;
    float min_ms;
    float max_ms;
    float back_to_back_ms; /* (one event pair around `runs` consecutive launches) / runs */
} lfi_bench_stats;

/* ---- lifetime --------------------------------------------------------------------------------------------- */

/* Interpolator::Interpolator / init (src/interpolator.cu:36-50): bind to HIP device `device`, create the stream. */
int lfi_create(int device, lfi_ctx **out_ctx);
/* Interpolator::~Interpolator (src/interpolator.cu:41-44) — frees what the context owns; no device reset. */
int lfi_destroy(lfi_ctx *ctx);
/* message of the last failure on this context (ctx == NULL: last failure of lfi_create on this thread) */
const char *lfi_last_error(const lfi_ctx *ctx);
int lfi_abi_version(void);
/* number of visible HIP devices (≥0) or a negative error */
int lfi_device_count(void);

/* ---- light-field grid: replaces loadGPUData / createSurfaceObject / loadImageToArray (src/interpolator.cu:73-137) --- */

/* Declare a cols×rows grid of width×height RGBA8 images and allocate N = cols*rows input planes + 2 focus maps. */
int lfi_set_grid(lfi_ctx *ctx, int cols, int rows, int width, int height);
/* Row window for spatial (row-band) multi-GPU sharding — SURVEY.md §8(f).2; no counterpart in the reference.  After
 * lfi_set_grid: this context renders output rows [out_y0, out_y1) only and holds input rows [in_y0, in_y1) of every image only
 * (band + the halo the warp reaches into); planes shrink accordingly, so G GPUs each read and write ≈1/G of the bytes.  Host
 * pointers passed to upload / download / quilt calls keep addressing row 0 of the WHOLE image; attached device buffers hold
 * the window's rows only.  lfi_set_params verifies that the input rows cover every row a fixed-focus render samples; lfi_focus_map
 * (which then computes the band's rows of the maps: map 0 for the band plus the filter's reach, map 1 for the band) and all-focus
 * renders verify their own, larger reach — the warp at both ends of [focus, focus + range], plus the block radius for the map —
 * and fail with LFI_EINVAL if the held rows fall short (lfinterpolator_amd/sharding.py input_rows_all_focus computes them). */
int lfi_set_row_window(lfi_ctx *ctx, int out_y0, int out_y1, int in_y0, int in_y1);
/* cudaMemcpy2DToArray of one image (src/interpolator.cu:91): copies; the caller keeps ownership.  Synchronous. */
int lfi_upload_image(lfi_ctx *ctx, int g, const uint8_t *rgba, size_t pitch_bytes);
/* The same copy, asynchronous: enqueued on the context's copy stream — no synchronisation with the compute
 * stream per image, the GPU keeps rendering while images cross PCIe.  A page-locked source (lfi_alloc_pinned) is DMA'd in place:
 * the call returns at once and the buffer must stay valid until lfi_upload_wait / lfi_sync.  A pageable source is staged by the
 * HIP runtime before the call returns (the buffer is free on return; the host thread is busy for the copy's duration).
 * Everything that uses the planes afterwards (renders, focus map, fills) is ordered after the pending copies by an event,
 * without a host wait. */
int lfi_upload_image_async(lfi_ctx *ctx, int g, const uint8_t *rgba, size_t pitch_bytes);
/* host wait for the asynchronous uploads issued so far */
int lfi_upload_wait(lfi_ctx *ctx);
/* Images from 8-bit YUV 4:2:0 video frames (I420), expanded to RGBA on the device: decoded video goes in as it is, 1.5 bytes per pixel
 * cross PCIe instead of the 4 of lfi_upload_image.  A frame has the layout lfi_download_views_yuv420 writes: the Y plane [H][W], then Cb
 * [ch][cw], then Cr [ch][cw], cw = (W + 1) >> 1, ch = (H + 1) >> 1, tightly packed, frame_bytes = W*H + 2*cw*ch; chroma is centre-sited
 * (Y4M's C420jpeg).  matrix and range (LFI_YUV_*) select one of four coefficient sets in 16-bit fixed point:
 *                    cY       rV       gU       gV       bU     y_off
 *   BT.709 limited 76309   117489   -13975   -34925   138438     16
 *   BT.709 full    65536   103206   -12276   -30679   121609      0
 *   BT.601 limited 76309   104597   -25675   -53279   132201     16
 *   BT.601 full    65536    91881   -22553   -46802   116130      0
 * Each entry is round(c * scale * 2^16), scale = 255/219 (limited luma), 255/224 (limited chroma), 1 (full range); with Kr, Kb of the
 * matrix and Kg = 1 - Kr - Kb: rV = 2(1 - Kr), bU = 2(1 - Kb), gU = -2Kb(1 - Kb)/Kg, gV = -2Kr(1 - Kr)/Kg.
 * The chroma of pixel (x, y) is taken in sixteenths; with cx = x >> 1, cy = y >> 1:
 *   LFI_CHROMA_NEAREST    SU = 16*U[cy][cx]
 *   LFI_CHROMA_BILINEAR   SU = 9*U[cy][cx] + 3*U[cy][nx] + 3*U[ny][cx] + U[ny][nx],  nx = clamp(cx + ((x & 1) ? 1 : -1), 0, cw - 1),
 *                         ny = clamp(cy + ((y & 1) ? 1 : -1), 0, ch - 1): the triangle filter of centre siting (libjpeg's "fancy" h2v2
 *                         upsampling)
 * and SV the same from Cr.  With l = 16*cY*(Y - y_off), u = SU - 2048, v = SV - 2048, all in integers:
 *     R = clamp(floor((l + rV*v        + 2^19) / 2^20), 0, 255)
 *     G = clamp(floor((l + gU*u + gV*v + 2^19) / 2^20), 0, 255)
 *     B = clamp(floor((l + bU*u        + 2^19) / 2^20), 0, 255)         A = 255
 * One rounding; over all byte triples the bracket stays within +-573,111,632 before the rounding term (int32, arithmetic shift).  Chroma
 * 128 gives R = G = B for every Y; limited 16 -> 0 and 235 -> 255; codes outside the nominal range are legal input and are clamped. */
enum { LFI_CHROMA_BILINEAR = 0, LFI_CHROMA_NEAREST = 1 };
/* Fills images [g0, g0 + n) of the grid from the frames at frames + k*frame_stride_bytes, k in [0, n): every byte of the n images, alpha
 * included.  Ordered like lfi_upload_image_async: the work goes on the context's copy stream behind the renders already enqueued, a
 * page-locked source must stay valid until lfi_upload_wait / lfi_sync, and everything that uses the planes afterwards is ordered after
 * it by an event, without a host wait.  The frames are copied into a device staging buffer the context owns (lfi_memory.workspace_bytes,
 * LFI_POISON_SCRATCH; the result depends on no byte of it the call did not copy) in chunks of at most 16 frames or 256 MiB, at least one
 * frame, each followed by one kernel launch; where W is a multiple of 8 and H is even a chunk is one copy (frame_stride_bytes ==
 * frame_bytes; else one 2D copy whose rows are whole frames), other sizes take three 2D copies per frame.  An attached grid is written in place; the derived planar
 * copy of the images is rebuilt by its next user, as after lfi_upload_image_async.
 * LFI_EINVAL, the context usable and the grid untouched: no grid; released inputs (lfi_release_inputs); a row window (a 2x2 block may
 * straddle the band); n < 1 or a range outside [0, N); an unknown matrix, range or chroma value; frames NULL; frame_stride_bytes <
 * frame_bytes. */
int lfi_upload_images_yuv420(lfi_ctx *ctx, int g0, int n, int matrix, int range, int chroma, const uint8_t *frames, size_t frame_stride_bytes);
/* Use caller-owned device memory ([N][H][W][4] u8, ≥ N*H*W*4 bytes) for the input planes instead of the context's
 * own allocation — lets the caller fill it (e.g. an RCCL broadcast into a tensor it owns).  Call after lfi_set_grid. */
int lfi_attach_grid(lfi_ctx *ctx, void *device_ptr, size_t bytes);
/* Single-process multi-GPU: copy the input planes of ctxs[root] into every other context's planes with ONE RCCL broadcast over
 * xGMI (ncclCommInitAll + ncclBroadcast; RCCL is loaded on first use) — the light field then lives on every GPU and rendering
 * needs no further collective.  All contexts must sit on distinct devices and describe the same grid and row
 * window.  n == 1 is a no-op.  Synchronous.  (One process per GPU instead: broadcast the attached buffers with your own
 * communicator, as bench.py does through torch.distributed.) */
int lfi_broadcast_grid(lfi_ctx *const *ctxs, int n, int root);
/* Fixed-focus use only: make the derived planar copy of the inputs (3 bytes per pixel and image, built and tuned for the CURRENT
 * parameters' offsets now if it is not yet) the ONLY copy and free the RGBA planes — the inputs' footprint drops from 1.9x to 0.9x of
 * the RGBA bytes (BASELINE config 5: 14.2 -> 6.8 GB).  Afterwards: fixed-focus TEN_WM / STD renders through the default kernels are
 * served as before, for any parameters whose offsets the copy's padding covers (it is padded a quarter beyond the current ones);
 * lfi_upload_image[_async] replaces an image through a one-image staging plane (synchronously); everything that needs the RGBA planes
 * — lfi_focus_map, all-focus renders, debug modes, weights outside [0, 2), larger offsets, lfi_fill_synthetic*, lfi_grid_device_ptr,
 * lfi_broadcast_grid — is refused with LFI_EINVAL until lfi_set_grid / lfi_attach_grid start over.  An attached grid is only forgotten.
 * The reference keeps its inputs as cudaArrays for the lifetime of the object (src/interpolator.cu:73-93, loadGPUData :95-137). */
int lfi_release_inputs(lfi_ctx *ctx);

/* device pointer / size of the input planes currently in use */
int lfi_grid_device_ptr(lfi_ctx *ctx, void **out_ptr, size_t *out_bytes);
/* Tell the library that the contents of the input planes changed behind its back (a write through lfi_grid_device_ptr, or into
 * a buffer given to lfi_attach_grid — e.g. the RCCL broadcast bench.py does after attaching).  The renders keep a derived copy
 * of the inputs (planar, alpha dropped: 25 % fewer bytes to read per launch — DESIGN.md §4.1) which uploads through this API
 * invalidate by themselves.  A context whose planes are attached or whose pointer has been handed out reads the RGBA planes
 * directly on every launch, as the reference reads its surfaces, until this call has been made once: from then on the caller is
 * trusted to repeat it after every such write.  No counterpart in the reference (its inputs are immutable after loadGPUData). */
int lfi_grid_modified(lfi_ctx *ctx);
/* fill the input planes on the device with the synthetic light field of SURVEY.md §8(d):
 * byte = hash32(seed, g, y, x, c) >> 24, alpha 255 (identical to oracle lfo_fill_synthetic) */
int lfi_fill_synthetic(lfi_ctx *ctx, uint32_t seed);
/* the same for images [g0, g1) only — a rank of an all-gather distribution generates (or uploads) just its own slice */
int lfi_fill_synthetic_images(lfi_ctx *ctx, uint32_t seed, int g0, int g1);
/* a STRUCTURED synthetic light field for focus-map measurements: a texture of 8×8-pixel cells seen at a
 * piecewise-constant focus (1024×1024-pixel blocks, each at one of four of the estimate's candidates inside [focus, focus + range]
 * of the current parameters) — image g shows T(p − f*·offsets[g]), so the estimate finds a piecewise-constant map as in real
 * scenes (hash noise gives a noise map, and all-focus renders from a noise map gather one cache line per pixel).  Needs
 * lfi_set_params (offsets, focus, range).  Measurement only. */
int lfi_fill_synthetic_scene(lfi_ctx *ctx, uint32_t seed);

/* ---- parameters: replaces loadGPUOffsets / loadGPUWeights / selectFocusMapViews / loadGPUConstants
 *      (src/interpolator.cu:139-154, 194-246) ------------------------------------------------------------------
 * The arrays are copied before the call returns (the caller's memory is free again).  A call that keeps the number of views (a focus
 * sweep, another trajectory of the same length) replaces the device arrays IN STREAM ORDER through page-locked staging: renders already
 * enqueued keep the parameters they were enqueued with, later ones see the new ones, and the context's stream is not drained.  The staging
 * has two buffers: a call may wait on the host until the copy of the call before the previous one has run, i.e. until the renders enqueued
 * before THAT call have finished — two replacements are always in flight without a wait, a third in a row is not (lfi_set_view_offsets,
 * lfi_set_view_float_offsets and lfi_view_focus_maps stage their rows the same way).  A call that changes the number of views synchronises
 * and reallocates. */
int lfi_set_params(lfi_ctx *ctx, const lfi_params *params);
/* Per-view focus: focal stacks (one camera position at V focus values) and focus pulls (the focus changing along the trajectory) in
 * one launch.  No counterpart in the reference, whose kernels apply one focus to all views (focusedOffsets, src/interpolator.cu:226-246).
 * focused_offsets_vn is [views][N] (host memory, copied before the call returns): view v of a fixed-focus render samples image g at
 * pixel + focused_offsets_vn[v][g] instead of pixel + lfi_params.focused_offsets[g] — row v of round(offset_g * f_v) for a focus f_v per
 * view (lfi_host_build_view_offsets).  Weights, clamping and the numerics of both methods are those of the ordinary render.
 *  - call after lfi_set_params; views must equal lfi_params.views (else LFI_EINVAL).  NULL clears the per-view offsets; so does any
 *    later lfi_set_params, lfi_set_grid or lfi_set_row_window;
 *  - stream-ordered, like lfi_set_params: the offsets go to the device through page-locked staging behind the work already enqueued, so
 *    renders enqueued before the call keep the offsets they were enqueued with and the stream is not drained;
 *  - with a row window, the held input rows must cover every row any view samples (else LFI_EINVAL);
 *  - while they are set, lfi_render (all_focus = 0), lfi_prepare and lfi_benchmark launch one kernel for all views of the range
 *    (csrc/hip/blend_vfocus.hpp; lfi_last_kernel_name names it, lfi_set_variant choices do not apply) — a vector-pipe gather-blend:
 *    STD is bit-exact, TEN_WM is the fp32-accumulated sum rounded once to fp16 and truncated (the TEN_WM contract) and does NOT use the
 *    matrix cores.  Downloads, quilts, lfi_compare_view, both view layouts and attached views work unchanged.  All-focus renders,
 *    lfi_render_stream, lfi_download_prequant and LFI_FLAG_TEN_ROUND_PER_BATCH return LFI_EINVAL;
 *  - after lfi_release_inputs, renders are served while the planar copy's padding covers every per-view horizontal shift (else LFI_EINVAL).
 * Shifts beyond the image are clamped to ±width / ±height (the same samples: every pixel then reads the edge). */
int lfi_set_view_offsets(lfi_ctx *ctx, const lfi_int2 *focused_offsets_vn, int views);
/* Per-view float offsets for all-focus renders: every view shifted about its own camera.  The reference computes one row of offsets for
 * the trajectory's centre (loadGPUOffsets → trajectoryCenter, src/interpolator.cu:226-246) and applies it to every view; its author left a
 * per-view centre commented out there and, in scripts/focusMapCompare.sh, a note to edit the offsets per view id — one run per view.
 * offsets_vn is [views][N] (host memory, copied before the call returns): view v of an all-focus render samples image g at
 * (int)fma(f(x,y), offsets_vn[v][g], pixel) instead of (int)fma(f(x,y), lfi_params.offsets[g], pixel) — row v of lfi_host_build_view_centred_offsets
 * is lfi_params.offsets for the trajectory collapsed onto camera v.  It is the per-view counterpart of lfi_params.offsets:
 *  - call after lfi_set_params; views must equal lfi_params.views and every offset be finite (else LFI_EINVAL).  NULL clears them; so
 *    does any later lfi_set_params, lfi_set_grid or lfi_set_row_window;
 *  - stream-ordered like lfi_set_view_offsets: renders enqueued before the call keep the offsets they were enqueued with;
 *  - all-focus renders only: fixed-focus renders keep lfi_params.focused_offsets, or the integer rows of lfi_set_view_offsets (both may be
 *    set at once; all-focus renders with only the integer rows set stay refused);
 *  - with a row window, the held input rows must cover every row any view of the range samples for f in [focus, focus + range] (else
 *    LFI_EINVAL at the render);
 *  - while they are set, all-focus lfi_render, lfi_prepare and lfi_benchmark launch one kernel for all views of the range
 *    (csrc/hip/blend_vfocus_af.hpp; lfi_last_kernel_name names it, lfi_set_variant choices do not apply) — a vector-pipe gather-blend over
 *    the RGBA planes: STD is bit-exact, TEN_WM is the fp32-accumulated sum rounded once to fp16 and truncated (the TEN_WM contract) and does
 *    NOT use the matrix cores.  Each view reads the same focus map as the ordinary render (map 1 for STD, map 0 for TEN_WM unless
 *    LFI_FLAG_UNIFIED_FOCUS_MAP), at its own pixel.  Downloads, quilts, lfi_compare_view, both view layouts and attached views work
 *    unchanged.  All-focus lfi_render_stream, all-focus lfi_download_prequant and LFI_FLAG_TEN_ROUND_PER_BATCH return LFI_EINVAL.
 * lfi_focus_map is unchanged: it estimates the map at the trajectory's centre from lfi_params.offsets and focus_map_ids.  Each view can have
 * a focus map of its own, estimated at its own camera: lfi_view_focus_maps.  New rows (or NULL) clear those maps. */
int lfi_set_view_float_offsets(lfi_ctx *ctx, const lfi_float2 *offsets_vn, int views);
/* Per-view focus maps: every view of a view-centred all-focus render (lfi_set_view_float_offsets) reads a map estimated at its own camera —
 * what the reference's scripts/focusMapCompare.sh gets from a second run per camera (-t POS,POS,POS,POS -f … -r …).  focus_ids_vk is
 * [views][n_ids] (host memory, copied before the call returns): row v = the images view v's map samples, FocusMap's selection for the
 * trajectory collapsed onto camera v (lfi_host_build_view_focus_ids).  View v's map 0 = FocusMap::estimate with offsets_vn[v], ids row v and
 * lfi_params' focus, range and block radius; its map 1 = FocusMap::filter of it.  The estimate is a min / max over the SET of ids: the order
 * of a row changes no byte.
 *  - call after lfi_set_view_float_offsets; views must equal lfi_params.views, 1 <= n_ids <= LFI_MAX_FOCUS_IDS, every id in [0, N) and
 *    range > 0 (else LFI_EINVAL); LFI_EINVAL too with a row window and after lfi_release_inputs;
 *  - enqueues maps 0 and 1 of every view on the context's stream, no host synchronisation: the factored estimate of lfi_focus_map view by
 *    view ("factored_direct" if lfi_set_variant chose it; the other estimate variants do not apply), then one filter launch for all views.  The padded copies
 *    of the sampled images are shared by the batch: an image that stays among the sampled ones keeps its copy, only the others are padded;
 *  - the maps live in device memory of their own, [views][2][H][W] RGBA (allocated on first use, counted in lfi_memory.maps_bytes, freed with
 *    the context); lfi_focus_map and maps 0 / 1 are unaffected;
 *  - from a successful call until the float rows are cleared (lfi_set_params, lfi_set_grid, lfi_set_row_window, lfi_set_view_float_offsets
 *    with NULL or new rows), all-focus lfi_render, lfi_prepare and lfi_benchmark read view v's own map (map 1 for STD, map 0 for TEN_WM, map 1
 *    for both with LFI_FLAG_UNIFIED_FOCUS_MAP) at view v's pixel (blend_vfocus_af's view_maps variant: lfi_last_kernel_name names it).
 *    Uploads do not clear them.  The refusals of the float rows stay (all-focus lfi_render_stream and lfi_download_prequant,
 *    LFI_FLAG_TEN_ROUND_PER_BATCH). */
int lfi_view_focus_maps(lfi_ctx *ctx, const int32_t *focus_ids_vk, int views, int n_ids);
/* Device layout of the rendered views.  LFI_LAYOUT_RGBA (default): [V][rows][W] RGBA8 dwords — the linear image of the
 * reference's 64 output surfaces.  LFI_LAYOUT_PLANAR_RGB (opt-in): alpha-free byte planes [V][3: R,G,B][rows][pitch] — the alpha
 * the reference's kernels write is the constant 255 (uchar4{…, 255}, src/kernels.cu:393, :309), a quarter of the bytes a render
 * writes; in this layout it is not stored and lfi_download_view / _quilt re-create it, so host-side results are byte-identical.
 * TEN_WM fixed-focus renders write the planes directly (csrc/hip/blend_p3.hpp); every other render goes through the RGBA kernels
 * and is converted.  Call after lfi_set_grid; frees the context's views (an attached buffer is dropped: attach again with the new
 * size); rows = the rows this context renders (all, or its row window). */
enum { LFI_LAYOUT_RGBA = 0, LFI_LAYOUT_PLANAR_RGB = 1 };
int lfi_set_output_layout(lfi_ctx *ctx, int layout);
typedef struct lfi_view_layout_info {
    int32_t layout;            /* LFI_LAYOUT_* */
    int32_t rows;              /* rows per plane */
    size_t row_pitch_bytes;    /* RGBA: W*4; planar: W rounded up to 128 (every plane row starts on a cache line) */
    size_t plane_stride_bytes; /* planar: bytes from a view's R plane to its G plane; RGBA: 0 */
    size_t view_stride_bytes;  /* bytes from view v to view v+1 */
} lfi_view_layout_info;
int lfi_view_layout(lfi_ctx *ctx, lfi_view_layout_info *out);
/* caller-owned device memory for the V views in the current layout (V * view_stride_bytes); call after lfi_set_params */
int lfi_attach_views(lfi_ctx *ctx, void *device_ptr, size_t bytes);
int lfi_views_device_ptr(lfi_ctx *ctx, void **out_ptr, size_t *out_bytes);

/* ---- kernels ------------------------------------------------------------------------------------------------ */

/* FocusMap::estimate + FocusMap::filter launches (src/interpolator.cu:261-266): fills maps 0 and 1.
 * The estimate reads edge-padded copies of the <= 32 sampled images; they depend on the inputs only (and on a bound of the shifts),
 * so they are kept between calls and rebuilt when the images change (any upload / fill through this library, lfi_grid_modified for
 * writes through the raw pointer), when other images are sampled, or when the shifts outgrow the padding: a focus sweep over one
 * light field (the reference's focusMapCompare.sh loop) pads once.  The map is estimated at the trajectory's centre from lfi_params.offsets
 * and focus_map_ids, whether or not per-view float offsets (lfi_set_view_float_offsets) are set. */
int lfi_focus_map(lfi_ctx *ctx);
/* Fine focus maps: the number of focus candidates lfi_focus_map chooses every pixel's focus from.  The reference hard-codes 32
 * (src/kernels.cu:245); the map byte has 256 levels and the all-focus kernels turn any byte into a focus, focus + byte / 255 * range.
 * With `steps` candidates:
 *  - f_i = fmaf(range / (float)(steps - 1), (float)i, focus), for i in [0, steps);
 *  - a pixel's winner is the first i with the strictly smallest comparison key;
 *  - the key is 16 * S_i, or, where S_i = 0, the number of FLT_MIN taps: the reference's MinDispersion (src/kernels.cu:219-237) over its float sum;
 *  - map 0 byte = round((f_best - focus) / range * 255), in float32;
 *  - map 1 is the unchanged filter of map 0.
 * With steps = 32 every byte is what it is without the call.
 *  - allowed: the multiples of 32 from 32 to 256; anything else returns LFI_EINVAL with a message and keeps the setting;
 *  - a context setting, default 32, that lives until it is changed: lfi_set_grid, lfi_set_params and lfi_set_row_window do not touch it;
 *  - it governs lfi_focus_map, whole frame and under a row window.  lfi_view_focus_maps keeps 32 candidates; lfi_focus_tiles keeps 32;
 *    lfi_focus_tiles_steps takes its own argument; lfi_focus_curve keeps its own `steps` argument;
 *  - the estimate variants "factored" (default), "factored_direct" and "packed_p2" honour it (as does the row-window path); with "lds" or
 *    "plain" selected, lfi_focus_map returns LFI_EINVAL while the setting is not 32, and leaves the maps untouched;
 *  - cost: the factored estimate runs one pass per 32 candidates over the same padded planes (a change of steps alone pads nothing) and
 *    carries each pixel's minimum between the passes in one more plane of its workspace (4 bytes per pixel, lfi_memory.workspace_bytes,
 *    LFI_POISON_FOCUS_WORKSPACE), which every call initialises itself. */
int lfi_set_focus_steps(lfi_ctx *ctx, int steps);
int lfi_focus_steps(lfi_ctx *ctx, int *out_steps);
/* Autofocus: the focus CURVE of the region [x0, x1) x [y0, y1) and its minimum — "what is the focus of this object?" (click-to-focus, or the
 * whole frame for a fixed-focus render).  No counterpart in the reference, whose estimate keeps only each pixel's argmin of the cost
 * (MinDispersion, src/kernels.cu:219-237) and throws the cost away; here the cost is summed over the region per candidate instead, on the
 * device (csrc/hip/focus_curve.hpp), and steps * 8 + 16 bytes come back.
 *  - candidates: step = range / (float)(steps - 1), f_i = fmaf(step, (float)i, focus) in fp32 (lfi_host_focus_candidates) — for steps == 32
 *    exactly the estimate's candidates (src/kernels.cu:245-250).  2 <= steps <= 256, range > 0: [focus, focus + range] is the search interval;
 *  - cost[i] = the sum over the region's pixels of S_i(x, y), the integer form of focusDispersion(f_i, (x, y)) (src/kernels.cu:196-217): over
 *    the n_focus_ids images of lfi_params.focus_map_ids, sampled at (int)fmaf(f_i, offsets[g], pixel) +- block_radius (3 x 3 taps, clamp to
 *    edge), per tap the largest channel's max - min over the images, summed over the nine taps.  It uses the CURRENT lfi_params (offsets, ids,
 *    focus, range, block radius), i.e. the trajectory's centre, as lfi_focus_map does; per-view offsets of either kind do not affect it.
 *    The sums are integers: exact, whatever the order;
 *  - one departure from the float code: the reference starts its running maximum at FLT_MIN (src/kernels.cu:178), so a tap whose samples are
 *    all zero contributes 1.2e-38 instead of 0.  Those terms cannot be added meaningfully over a region and are dropped.  It only matters where
 *    several candidates have cost 0: the first of them then wins;
 *  - out->best_index: the first candidate with the strictly smallest cost (MinDispersion's rule, src/kernels.cu:225-231), out->best_focus =
 *    f_best_index, out->pixels = (x1 - x0) * (y1 - y0).  out_cost ([steps], may be NULL) receives the curve;
 *  - synchronous; ordered after pending uploads and the work on the context's stream like lfi_focus_map; it leaves the maps, the views, the
 *    estimate's padded planes and workspace as they were (a later lfi_focus_map gives the same bytes as without the call).  Its own device
 *    memory (per-workgroup partial sums, the curve and the result) is counted in lfi_memory.workspace_bytes;
 *  - LFI_EINVAL: no grid or no parameters; an empty region or one that leaves the image; steps outside [2, 256]; range <= 0; n_focus_ids == 0;
 *    out == NULL; a row window set; after lfi_release_inputs (it reads the RGBA planes).  The context stays usable. */
typedef struct lfi_focus_curve_result {
    int32_t best_index;  /* first candidate with the strictly smallest cost */
    float best_focus;    /* f_best_index */
    uint64_t pixels;     /* pixels of the region */
} lfi_focus_curve_result;
int lfi_focus_curve(lfi_ctx *ctx, int x0, int y0, int x1, int y1, int steps, uint64_t *out_cost, lfi_focus_curve_result *out);
/* Focus tiles: the focus curve of EVERY tile of a tiles_x x tiles_y grid over the frame, from one factored estimate — a grid of autofocus
 * points, a coarse depth layout of the scene, or the interval an all-focus render should search (lfi_host_focus_auto_range).
 *  - tile (tx, ty) is the rectangle [tx * W / tiles_x, (tx + 1) * W / tiles_x) x [ty * H / tiles_y, (ty + 1) * H / tiles_y), the divisions
 *    integer divisions of 64-bit products (lfi_host_focus_tile_rect): the tiles cover the frame exactly once and differ by at most one pixel
 *    per axis.  1 <= tiles_x <= min(W, 256), 1 <= tiles_y <= min(H, 256);
 *  - out_cost[tile][i] ([tiles_y][tiles_x][LFI_FOCUS_TILE_STEPS], may be NULL) and out[tile] ([tiles_y][tiles_x]) are, BY DEFINITION, what
 *    lfi_focus_curve(ctx, the tile's rectangle, LFI_FOCUS_TILE_STEPS, ...) returns: the same candidates (the estimate's 32), the same integer
 *    cost, the same first-strict-minimum rule, the same FLT_MIN departure, the same use of the current lfi_params;
 *  - it is computed differently: the factored focus-map estimate (lfi_focus_map's default variant) runs up to its last pass, and a tile-cost
 *    pass in the pick's place adds up the per-pixel cost the pick would throw away (csrc/hip/focus_tiles.hpp) — all tiles for about the price
 *    of one focus map.  The estimate variant set with lfi_set_variant(LFI_KERNEL_FOCUS_ESTIMATE, ...) is followed: "factored_direct" takes its
 *    range pass; a variant that is not a factored one (or a factored estimate that declines) computes the tiles with lfi_focus_curve's
 *    kernels, one region per tile, inside the same call — the same numbers, slower;
 *  - synchronous; ordered after pending uploads and the work on the context's stream like lfi_focus_map, and joined with the side stream the
 *    estimate uses; one device-to-host copy of tiles * (32 * 8 + 16) bytes.  It writes neither the maps nor the views.  It builds or reuses
 *    the estimate's padded planes exactly as lfi_focus_map does and keeps their bookkeeping: a later lfi_focus_map gives the same bytes as
 *    without the call.  Its device memory is counted in lfi_memory.workspace_bytes;
 *  - LFI_EINVAL: a grid outside the limits above, and wherever lfi_focus_curve returns it (no grid or no parameters; range <= 0;
 *    n_focus_ids == 0; out == NULL; a row window set; after lfi_release_inputs).  The context stays usable. */
#define LFI_FOCUS_TILE_STEPS 32   /* the estimate's candidates, src/kernels.cu:245 */
int lfi_focus_tiles(lfi_ctx *ctx, int tiles_x, int tiles_y, uint64_t *out_cost, lfi_focus_curve_result *out);
/* Fine focus tiles: lfi_focus_tiles over `steps` candidates instead of 32.  lfi_focus_tiles(ctx, x, y, ...) is this call with steps = 32.
 *  - out_cost[tile][i] ([tiles_y][tiles_x][steps], may be NULL) and out[tile] ([tiles_y][tiles_x]) are, BY DEFINITION, what
 *    lfi_focus_curve(ctx, lfi_host_focus_tile_rect(...), steps, ...) returns for tile (tx, ty): the candidates
 *    f_i = fmaf(range / (float)(steps - 1), (float)i, focus), the integer cost with the FLT_MIN terms dropped, the first strict minimum
 *    (best_index, best_focus = f_best_index) and pixels = the tile's area;
 *  - steps: a multiple of 32 from 32 to 256; anything else returns LFI_EINVAL with a message.  It is an argument of this call, as
 *    lfi_focus_curve's is: lfi_set_focus_steps keeps governing lfi_focus_map only, and this call neither reads nor changes that setting;
 *  - the factored estimate runs one pass per 32 candidates over the same padded planes, the tile-cost pass in the pick's place in each;
 *    the per-workgroup partial sums stay those of 32 candidates, only the curves grow with steps.  The carry plane of a fine focus map is
 *    neither read nor written.  A variant that is not a factored one (or a factored estimate that declines) takes lfi_focus_curve's kernels
 *    tile by tile with all the steps — the same numbers, slower;
 *  - everything else is lfi_focus_tiles': synchronous, one device-to-host copy of tiles * (steps * 8 + 16) bytes, neither maps nor views
 *    written, the padded planes built or reused with lfi_focus_map's bookkeeping, the same refusals. */
int lfi_focus_tiles_steps(lfi_ctx *ctx, int tiles_x, int tiles_y, int steps, uint64_t *out_cost, lfi_focus_curve_result *out);
/* which way the last successful lfi_focus_tiles / lfi_focus_tiles_steps of this context took: the passes of the factored estimate it ran
 * (steps / 32), or 0 where it computed the tiles with lfi_focus_curve's kernels tile by tile (0 before the first call, too) — lets a
 * test or a measurement know that the numbers are the path's it means */
int lfi_focus_tiles_passes(const lfi_ctx *ctx);
/* The route of the last ESTIMATE CALL of this context — lfi_focus_map, lfi_focus_tiles, lfi_focus_tiles_steps, lfi_view_focus_maps —: which
 * estimate answered, with which kernels, over which geometry, and what the device's own plan counted.  Read-only: it lets a test (or a
 * measurement) know that the bytes it compares are the path's it means, as lfi_last_kernel_name does for the blend.
 *  - the names are static strings, set at the one place where each launch is chosen; "" = not applicable / nothing ran;
 *  - estimate: "factored" | "factored_direct" (the factored estimate, focus_factored.hpp, with its own or the direct range pass) |
 *    "packed_p2" | "lds" | "plain" (the one-kernel estimates, also where the factored one declined) | "row_window" (lfi_focus_map on a row
 *    window) | "focus_curve" (lfi_focus_tiles* tile by tile with lfi_focus_curve's kernels);
 *  - declined: "" or why the factored estimate declined before it reserved or enqueued anything: "shift" (a candidate's shift of a sampled
 *    image is absurd: |focus| * |offset| >= 1e6 pixels) or "planes" (the padded planes would take more than 16 GiB);
 *  - everything from `passes` on describes the factored estimate and is 0 / "" otherwise.  passes: the passes of 32 candidates it ran;
 *    range_cpw[p]: the candidates per group of pass p's range pass — 8 or 4: focus_range_t<8|4>, 0: focus_range<4> —, range_kernel and
 *    range_striped: the LAST pass's kernel and whether its work items were dealt in stripes per XCD; consumer: what read the keys in
 *    the pick's place — "focus_pick_sep", "focus_pick_sep_carry", "focus_pick<2>", "focus_pick_carry<2>", "focus_pick<1>",
 *    "focus_pick_carry<1>", "focus_tile_costs<2>", "focus_tile_costs<1>" — and consumer_striped likewise;
 *  - planes_padded / planes_kept: the padded planes (one per sampled image) the call rebuilt / found current and left alone;
 *    pad_shift, We_p, He_p, Wp, Hp, R_cap, C_cap: the geometry of the planes, of E and of the line buffers (csrc/hip/focus_factored.hpp);
 *  - row_entries[p] / col_entries[p]: the flagged (row, candidate) and (column, candidate) pairs of pass p as the DEVICE's plan counted
 *    them (focus_plan_prefix); more than R_cap / C_cap of them and the pairs beyond take the tap-by-tap path.  focus_plan_prefix stores
 *    the two totals a second time, per pass, for this call to read: the estimate itself gains no launch and no host wait;
 *  - lfi_view_focus_maps is a batch of `jobs` estimates (one per view; 1 for the other calls): planes_padded and planes_kept are the
 *    batch's totals, everything else is the LAST job's;
 *  - the call synchronises the context's streams and copies 64 bytes from the device when the factored estimate ran.  LFI_EINVAL: ctx or out
 *    NULL.  Before the first estimate call: calls = 0 and everything empty. */
#define LFI_FOCUS_ROUTE_PASSES 8
typedef struct lfi_focus_route {
    int32_t calls;              /* estimate calls of this context so far that passed their argument checks (this record is call number `calls`'s) */
    int32_t jobs;
    const char *estimate;
    const char *declined;
    int32_t passes;
    int32_t range_striped;
    const char *range_kernel;
    const char *consumer;
    int32_t consumer_striped;
    int32_t planes_padded;
    int32_t planes_kept;
    int32_t pad_shift[2];
    int32_t We_p, He_p, Wp, Hp, R_cap, C_cap;
    int32_t range_cpw[LFI_FOCUS_ROUTE_PASSES];
    uint32_t row_entries[LFI_FOCUS_ROUTE_PASSES];
    uint32_t col_entries[LFI_FOCUS_ROUTE_PASSES];
} lfi_focus_route;
int lfi_focus_route_info(lfi_ctx *ctx, lfi_focus_route *out);
/* One launch of Tensors::process / Standard::process (src/interpolator.cu:274-288) for views [v0, v1).
 * all_focus != 0 selects the <true> instantiations (per-pixel focus from the focus map). */
int lfi_render(lfi_ctx *ctx, int method, int all_focus, int v0, int v1);
/* Trajectory streaming: renders a camera path of total_views views — weights_fp16 is [total_views][N], built
 * for the WHOLE path by the host code (one trajectory centre, so the offsets set by lfi_set_params stay valid) — in blocks of V
 * views (V = lfi_params.views) against the resident inputs, with no host synchronisation between blocks: block b+1's weight
 * arrays are prepared on the host and copied while block b renders (page-locked double-buffered staging, stream-ordered device
 * copy), and, when host_out != NULL, block b's views are copied to host_out + (b·V + v)·pitch_bytes·H on a second stream from a
 * second set of views while block b+1 renders.  host_out should be page-locked (lfi_alloc_pinned) and needs the RGBA view
 * layout; NULL renders only (the views of the last block remain on the device).  Returns after everything has completed.
 * Afterwards the context's weights are those of the last block.  The reference renders exactly 64 views per run
 * (src/kernels.cu:11-14); this is its loop over successive 64-view segments of a longer path. */
int lfi_render_stream(lfi_ctx *ctx, int method, int all_focus, const uint16_t *weights_fp16, int total_views, uint8_t *host_out, size_t pitch_bytes);
/* Do now what the first such lfi_render would otherwise do before its launch: (re)build the derived, alpha-free planar copy of
 * the inputs if that launch would read it, and time it.  Optional; synchronous.  No counterpart in the
 * reference (its surfaces are read as uploaded). */
int lfi_prepare(lfi_ctx *ctx, int method, int all_focus, int v0, int v1);
/* device memory this context holds, and what the derived copy cost to build (ms, as measured by the last lfi_prepare that
 * built it; 0 otherwise) — the capacity side of the planar-copy trade, reported by bench.py */
typedef struct lfi_memory {
    size_t grid_bytes;      /* input planes (RGBA) */
    size_t derived_bytes;   /* planar copy of the inputs: 3 bytes per pixel and image (+ padding) */
    size_t views_bytes;     /* output planes, and the deep planes of LFI_FLAG_DEEP_VIEWS once allocated */
    size_t maps_bytes;      /* focus maps (maps 0 / 1, and the per-view maps when allocated) */
    size_t workspace_bytes; /* focus-map workspace + lfi_focus_curve's / lfi_focus_tiles' curves and partial sums + (planar view layout) the RGBA scratch copy of the views that renders other than TEN_WM and
                             * STD on more than 64 images go through, and the one-plane staging buffer of downloads + the kept views (lfi_keep_views) and
                             * lfi_compare_views' staging buffers and partial sums + lfi_download_native's device image + the device frames of
                             * lfi_download_views_yuv420 / lfi_render_stream_yuv420 + the staged frames of lfi_upload_images_yuv420 + the device image of the quilt calls
                             * (lfi_download_quilt*, lfi_download_native's scaled tiles; lfi_download_quilt_yuv reserves it for odd tile sizes
                             * only).  A change of this report: the quilt calls' device image was not counted before lfi_download_quilt_yuv */
    float derived_build_ms;
} lfi_memory;
int lfi_memory_info(lfi_ctx *ctx, lfi_memory *out);
/* The band method's self-check (round 5).  STD over more than 64 images (Standard::process, src/kernels.cu:289-343, computed as fp16
 * matrix-core sums + the exact fmaf chain inside a band around x.5) sizes that band with a bound on the matrix core's accumulation error
 * that was MEASURED on gfx950 (a quarter ulp per addend).  The first such launch on a device therefore repeats the measurement there —
 * chains of the MFMA instructions the kernels use over adversarial operand sets, exact sums on the host, once per device and process —
 * and if any sum exceeds the budget every such launch on that device takes the analytic band instead (LFI_FLAG_STD_ANALYTIC_BAND's:
 * same bytes, more sums recomputed).  This call runs the check if it has not run yet and reports it. */
typedef struct lfi_std_band {
    int32_t probed;           /* 1 once the device has been measured */
    int32_t within_budget;    /* 1: every sum within N*2^-17 of the exact one */
    int32_t analytic_forced;  /* 1: this context's STD launches over more than 64 images take the analytic band although the caller
                                 did not ask for it (the device failed the check, or LFI_FLAG_STD_BAND_PROBE_FAIL) */
    int32_t sums;             /* sums checked */
    float worst_fraction;     /* the largest error seen, as a fraction of the budget */
    float probe_ms;           /* what the check cost, once per device (host wall clock) */
    char message[160];
} lfi_std_band;
int lfi_std_band_info(lfi_ctx *ctx, lfi_std_band *out);
/* name of the blend kernel the last lfi_render / lfi_benchmark of this context launched ("" before the first) — lets the
 * measurement harness label its numbers with what actually ran (dispatch depends on shape, weights and mode) */
const char *lfi_last_kernel_name(const lfi_ctx *ctx);
/* The reference's benchmark loop (src/interpolator.cu:270-295) with warm-up launches excluded. Synchronous. */
int lfi_benchmark(lfi_ctx *ctx, int method, int all_focus, int v0, int v1, int warmup, int runs,
                  lfi_bench_stats *out_stats);
/* hipEvent pair on the context's stream (the reference's Timer, src/interpolator.cu:13-34) */
int lfi_timer_start(lfi_ctx *ctx);
int lfi_timer_stop(lfi_ctx *ctx, float *out_ms); /* records, synchronises, returns elapsed ms */
int lfi_sync(lfi_ctx *ctx);

/* ---- results: replaces storeResults' cudaMemcpy2DFromArray (src/interpolator.cu:309).  Synchronous. --------- */
int lfi_download_view(lfi_ctx *ctx, int v, uint8_t *rgba, size_t pitch_bytes);
int lfi_download_map(lfi_ctx *ctx, int k, uint8_t *rgba, size_t pitch_bytes);
/* Views v0 … v0+tiles_x*tiles_y-1 as ONE image of tiles_x × tiles_y tiles, filled left to right, top to bottom — what
 * scripts/viewsToQuilt.sh builds with ImageMagick `montage -tile 5x9` from the NN.png files (Looking-Glass quilt).
 * rgba: (tiles_y*H) rows of pitch_bytes ≥ tiles_x*W*4.  Synchronous. */
int lfi_download_quilt(lfi_ctx *ctx, int tiles_x, int tiles_y, int v0, uint8_t *rgba, size_t pitch_bytes);
/* The same for PART of a quilt: views v0 … v0+n-1 of this context become tiles first_tile … first_tile+n-1 (row-major) of the
 * tiles_x × tiles_y quilt whose top-left pixel is at rgba — a trajectory sharded over several GPUs (src/interpolator.cu has one GPU;
 * the CLI's -g): every context fills its own tiles of one host image.  The tiles are assembled on the device by one kernel (the
 * planar view layout is expanded on the fly) and copied in at most three rectangles; lfi_download_quilt is this with every tile. */
int lfi_download_quilt_tiles(lfi_ctx *ctx, int tiles_x, int tiles_y, int first_tile, int n, int v0, uint8_t *rgba, size_t pitch_bytes);
/* The quilt with every view RESIZED on the device to a tile of tile_w × tile_h pixels, 1 ≤ tile_w ≤ W, 1 ≤ tile_h ≤ H (downscaling or
 * identity; each axis on its own) — scripts/viewsToQuilt.sh's `montage -tile 5x9 -geometry 1920x1080+0+0` resizes on the way into the
 * quilt too, and a Looking-Glass quilt of 4096² or 8192² pixels has 5 × 9 tiles of 819 × 455 or 1638 × 910.  Only the scaled bytes are
 * copied to the host.  rgba: (tiles_y*tile_h) rows of pitch_bytes ≥ tiles_x*tile_w*4; tiles left to right, top to bottom.  Synchronous.
 * The resize is an exact AREA (box) filter in integers: along x both images lie on a grid of W·tile_w units, output column ox covers
 * [ox·W, (ox+1)·W), source column sx covers [sx·tile_w, (sx+1)·tile_w), and wx(ox, sx) is the length of their overlap (over sx it sums to
 * W); wy likewise with H and tile_h; per colour channel
 *     out = (Σ_sy Σ_sx wy·wx·p[sy][sx] + (W·H) / 2) / (W·H)        (integer division: the exact area mean, rounded half up)
 * and alpha is 255.  So tile = W × H gives lfi_download_quilt's bytes, W = k·tile_w and H = l·tile_h the k × l block mean, and every value
 * lies within 0.5 of the exact area mean.  ImageMagick's default resize filter is a different one: the bytes of `montage` are NOT
 * reproduced.  A 1 × 1 quilt of view v (v0 = v) is that view, scaled: a thumbnail or preview.
 * LFI_EINVAL for what lfi_download_quilt refuses, a tile size outside the limits, views of more than 65535 pixels along an axis, and while
 * a row window is set (a tile's rows average source rows the band does not hold). */
int lfi_download_quilt_scaled(lfi_ctx *ctx, int tiles_x, int tiles_y, int v0, int tile_w, int tile_h, uint8_t *rgba, size_t pitch_bytes);
/* … and for PART of such a quilt, as lfi_download_quilt_tiles: views v0 … v0+n-1 become tiles first_tile … first_tile+n-1, one kernel launch
 * for all n tiles (both view layouts are read as they are), at most three rectangles copied. */
int lfi_download_quilt_tiles_scaled(lfi_ctx *ctx, int tiles_x, int tiles_y, int first_tile, int n, int v0, int tile_w, int tile_h, uint8_t *rgba, size_t pitch_bytes);
/* The NATIVE image of a lenticular (Looking-Glass-type) display, interlaced on the device: one picture of out_w × out_h pixels in which
 * every SUBPIXEL takes its value from the one view that its position under the slanted lens sheet selects — what such a panel shows; a
 * quilt is only the intermediate a host-side interlace would start from.  The lens sheet is given in fixed point: a phase is a u32 in
 * units of 2^-32 lens periods, so the wrap of u32 arithmetic IS the fract() of the usual shader. */
typedef struct lfi_lenticular {
    uint32_t x_step;   /* phase advance per SUBPIXEL along x, in units of 2^-32 lens periods */
    uint32_t y_step;   /* phase advance per pixel row (two's complement: a negative slant wraps) */
    uint32_t phase0;   /* phase of subpixel 0 of pixel (0, 0) */
    int32_t  views;    /* n: the views v0 … v0+n-1 spread over one lens period, 1 ≤ n */
    uint32_t flags;    /* LFI_LENT_INVERT: view n-1-k where the phase selects k; LFI_LENT_BGR, LFI_LENT_BILINEAR, LFI_LENT_BLEND: below */
} lfi_lenticular;
#define LFI_LENT_INVERT 1u
#define LFI_LENT_BGR      4u    /* the panel's subpixels run B, G, R from left to right */
#define LFI_LENT_BILINEAR 8u    /* tile sampling: bilinear instead of nearest */
#define LFI_LENT_BLEND    16u   /* every subpixel blends the two views nearest to its phase */
/* For output pixel (x, y) and colour channel c ∈ {0: R, 1: G, 2: B} (RGB subpixel order), all in unsigned integers:
 *     phase = phase0 + (3·x + c)·x_step + y·y_step                       (mod 2^32)
 *     k     = (u64(phase) · n) >> 32;   with LFI_LENT_INVERT  k = n − 1 − k
 *     sx    = ((2·x + 1)·tile_w) / (2·out_w),   sy = ((2·y + 1)·tile_h) / (2·out_h)        (integer division)
 *     out[y][x][c] = T_{v0+k}[sy][sx][c],   alpha = 255
 * (sx, sy) is the tile pixel under the output pixel's centre (nearest; no filter), and T_v is view v resized to tile_w × tile_h by the
 * exact area filter of lfi_download_quilt_scaled — with tile = W × H the view itself, read in place in either view layout.  The output may
 * be smaller than, equal to or larger than the tile: 1 ≤ out_w, out_h ≤ 65535; the tile obeys lfi_download_quilt_scaled's limits.  With
 * all sizes at most 65535 the kernel computes sx as q + (2·r + tile_w) / (2·out_w) with q, r = quotient and remainder of x·tile_w by
 * out_w: every intermediate is below 2^32 (x·tile_w < 65535², 2·r + tile_w < 3·65535), so 32 bits suffice; sy likewise.
 * The scaled tiles and the native image are made on the device (the tiles never leave it); only out_w·out_h·4 bytes are copied, as one
 * rectangle.  rgba: out_h rows of pitch_bytes ≥ out_w·4.  Synchronous.  Attached views work as they do for quilts.
 * LFI_EINVAL, the context usable and the host image untouched: what lfi_download_quilt_scaled refuses for a tile (a row window among it),
 * lens NULL, n < 1 or v0 + n beyond the rendered views, unknown flag bits, an output size outside the limits, a NULL image or a pitch below
 * out_w·4.  (A display calibration becomes an lfi_lenticular on the host: csrc/host/lenticular.h.)
 *
 * The three filter flags refine the definition above; every other argument keeps its meaning, limits and refusals, and a call with none of
 * them computes exactly what is written above.  Still all in unsigned integers:
 *   LFI_LENT_BGR       the subpixel of channel c is s = 2 − c instead of s = c:  phase = phase0 + (3·x + s)·x_step + y·y_step.  The output stays
 *                      RGBA in memory; only which phase a channel has changes.
 *   view selection     P = u64(phase)·n,  k = P >> 32,  f = (P >> 24) & 255 — the top eight bits of the fraction; in 32 bits the high word of
 *                      phase·n and (phase·n mod 2^32) >> 24.
 *   LFI_LENT_BLEND     view k's centre is at fraction ½:  f ≥ 128: ka = k, kb = min(k + 1, n − 1), wb = f − 128;  else ka = max(k, 1) − 1, kb = k,
 *                      wb = f + 128.  The ends clamp and never wrap: views n − 1 and 0 are the two sides of the jump between lens periods.
 *                      out[y][x][c] = ((256 − wb)·S_{v0+ka} + wb·S_{v0+kb} + 128) >> 8;  without the flag out[y][x][c] = S_{v0+k}.
 *   LFI_LENT_INVERT    maps each selected index q (k, ka, kb) to n − 1 − q, after the selection.
 *   LFI_LENT_BILINEAR  the tile sample S_v(x, y, c), pixel centres at +½ on both sides.  Along x, with D = 2·out_w:
 *                        U  = clamp((2·x + 1)·tile_w − out_w, 0, (tile_w − 1)·D)          (the first term signed before the clamp)
 *                        x0 = U / D,  r = U − x0·D,  fx = (256·r) / D ∈ [0, 255],  x1 = min(x0 + 1, tile_w − 1)
 *                      along y likewise (y0, y1, fy), then
 *                        h_j = (256 − fx)·T_v[y_j][x0][c] + fx·T_v[y_j][x1][c]   (j = 0, 1),   S = ((256 − fy)·h_0 + fy·h_1 + 2^15) >> 16.
 *                      Without the flag S_v = T_v[sy][sx][c] as above.  Every intermediate is below 2^24 except (2·x + 1)·tile_w < 2^33, which the
 *                      kernel splits as it does for sx: with q, r = quotient and remainder of x·tile_w by out_w, (2·x + 1)·tile_w − out_w + D =
 *                      D·q + e with e = 2·r + tile_w + out_w < 4·65535, so 32 bits suffice (csrc/native_taps.h).
 * Alpha is 255.  What follows from this: with tile = out_w × out_h, fx = fy = 0 everywhere and LFI_LENT_BILINEAR changes no byte (the call
 * drops the flag there); a phase exactly on a view's centre (f = 128) has wb = 0, view k alone; a phase on a boundary (f = 0) is the rounded
 * even mix of the two neighbours; n = 1 gives view v0 under any flags.  Flag bits other than these four are refused. */
int lfi_download_native(lfi_ctx *ctx, const lfi_lenticular *lens, int v0, int out_w, int out_h, int tile_w, int tile_h, uint8_t *rgba, size_t pitch_bytes);
/* Views as 8-bit YUV 4:2:0 video frames (I420), converted on the device before the copy: what every encoder and player takes, 1.5 bytes per
 * pixel instead of the 4 of lfi_download_view (the alpha dropped is the constant 255, the chroma dropped is what an encoder's first step
 * would drop).  A frame of a W x H view is the Y plane [H][W], then Cb [ch][cw], then Cr [ch][cw], cw = (W + 1) >> 1, ch = (H + 1) >> 1,
 * tightly packed: frame_bytes = W*H + 2*cw*ch.  matrix and range select one of four coefficient sets in 16-bit fixed point:
 *                   Y (R, G, B)           Cb (R, G, B)             Cr (R, G, B)            y_off
 *   709 limited   11966, 40254, 4064    -6596, -22188, 28784     28784, -26145, -2639      16
 *   709 full      13933, 46871, 4732    -7509, -25259, 32768     32768, -29763, -3005       0
 *   601 limited   16829, 33039, 6416    -9714, -19070, 28784     28784, -24103, -4681      16
 *   601 full      19595, 38470, 7471   -11058, -21710, 32768     32768, -27439, -5329       0
 * Each entry is round(c * scale * 2^16) of the matrix's coefficient c, scale = 219/255 (limited luma), 224/255 (limited chroma), 1 (full
 * range); G is then adjusted so that Y sums to 56284 (limited) or 65536 (full) and Cb and Cr to 0: every grey has chroma exactly 128, white
 * is 235 (limited) or 255 (full).  Over all 2^24 colours limited range keeps Y in [16, 235] and chroma in [16, 240]; full-range chroma
 * reaches 256 before the clamp.  All in integers:
 *     Y[y][x]    = y_off + ((yR*R + yG*G + yB*B + 2^15) >> 16)
 *     Cb[cy][cx] = min(255, (2^25 + 2^17 + uR*SR + uG*SG + uB*SB) >> 18)        Cr likewise with the Cr coefficients
 * SR, SG, SB are the sums over the four pixels (min(2cx + i, W - 1), min(2cy + j, H - 1)), i, j in {0, 1}: centre siting (Y4M's C420jpeg),
 * an odd last column or row replicated.  The bracket is positive and below 2^27: unsigned 32-bit arithmetic, one rounding. */
enum { LFI_YUV_BT709 = 0, LFI_YUV_BT601 = 1 };
enum { LFI_YUV_LIMITED = 0, LFI_YUV_FULL = 1 };
/* Views [v0, v0 + n) as frames at out + k*frame_stride_bytes, k in [0, n).  One kernel launch converts all n views (both view layouts are
 * read in place; attached views too) into device frames the context owns (lfi_memory.workspace_bytes, LFI_POISON_SCRATCH; every byte copied
 * out the call has written); where W is a multiple of 8 and H is even the device frames are the host frames and one copy moves the batch
 * (frame_stride_bytes == frame_bytes; else one 2D copy whose rows are whole frames), other sizes take three 2D copies per frame.
 * Synchronous, ordered like
 * lfi_download_quilt; writes no view and no map.
 * LFI_EINVAL, the context usable and the host memory untouched: nothing rendered yet; n < 1 or a range outside [0, views); an unknown matrix
 * or range; out NULL; frame_stride_bytes < frame_bytes; a row window (a 2x2 block may straddle the band). */
int lfi_download_views_yuv420(lfi_ctx *ctx, int v0, int n, int matrix, int range, uint8_t *out, size_t frame_stride_bytes);
/* lfi_render_stream with YUV 4:2:0 frames for its downloads: the same contract for weights, blocks and ordering; view i of the path becomes
 * the frame at host_out + i*frame_stride_bytes.  Each block is rendered, then converted on the compute stream into one of two buffers of
 * frames, which is copied on the copy stream while the next block renders: no second set of views, and the planar view layout is allowed.
 * host_out must not be NULL (page-locked for the overlap).  LFI_EINVAL for what lfi_download_views_yuv420 refuses of matrix, range, pointer,
 * stride and row window, and wherever lfi_render_stream refuses. */
int lfi_render_stream_yuv420(lfi_ctx *ctx, int method, int all_focus, const uint16_t *weights_fp16, int total_views, int matrix, int range,
                             uint8_t *host_out, size_t frame_stride_bytes);

/* Video surfaces: a batch of 8-bit YUV 4:2:0 frames as decoders deliver and encoders take them — I420 or NV12, rows with a pitch, planes at
 * offsets inside a frame, in host memory or in memory of the context's own GPU.  The conversions are those defined above
 * (lfi_upload_images_yuv420, lfi_download_views_yuv420), bit for bit; the descriptor only says where the bytes lie.
 * Geometry of a W x H frame, cw = (W + 1) >> 1, ch = (H + 1) >> 1: the Y plane starts at the frame's base, H rows of y_pitch bytes.  I420:
 * the Cb plane at c_offset and the Cr plane at cr_offset, ch rows of c_pitch bytes each.  NV12: one plane at c_offset, ch rows of c_pitch
 * bytes, byte 2*cx of a row Cb and byte 2*cx + 1 Cr.  A plane occupies rows * pitch bytes, which the caller's memory must cover; only the
 * first W bytes of a Y row (cw of an I420 chroma row, 2*cw of an NV12 one) carry data: the rest is padding, never used as a value and
 * never written.  Frame k lies at base + k * frame_stride. */
enum { LFI_YUV_I420 = 0, LFI_YUV_NV12 = 1 };
enum { LFI_MEM_HOST = 0, LFI_MEM_DEVICE = 1 };   /* DEVICE: memory of the context's own GPU */
typedef struct lfi_yuv_surfaces {
    int32_t format, memory;
    void   *base;          /* frame 0 */
    size_t  frame_stride;  /* bytes from one frame's base to the next one's */
    size_t  y_pitch;       /* >= W (10-bit formats, below: twice the minima here) */
    size_t  c_offset;      /* from a frame's base to its chroma: NV12 the CbCr plane, I420 the Cb plane */
    size_t  c_pitch;       /* NV12 >= 2*cw, I420 >= cw */
    size_t  cr_offset;     /* I420: the Cr plane; NV12: must be 0 */
} lfi_yuv_surfaces;
/* LFI_OK if s describes n frames of width x height, else LFI_EINVAL: an unknown format or memory value, s or base NULL, width, height or n
 * below 1; a pitch below its minimum; planes of one frame that overlap or are not in the order Y, chroma (I420: Y, Cb, Cr); cr_offset != 0
 * with NV12; n > 1 with frame_stride below the frame's extent (the end of its last plane).  Context-free, needs no GPU. */
int lfi_yuv_surfaces_check(const lfi_yuv_surfaces *s, int width, int height, int n);
/* the tight layout at base (which may be NULL here, to be set later): y_pitch = W, the chroma right behind the Y plane with c_pitch = cw
 * (I420; Cr right behind Cb) or 2*cw (NV12), frame_stride = W*H + 2*cw*ch for both.  An I420 result is lfi_upload_images_yuv420's frame.
 * LFI_EINVAL: an unknown format or memory value, a size below 1, out NULL. */
int lfi_yuv_surfaces_packed(int format, int memory, void *base, int width, int height, lfi_yuv_surfaces *out);
/* lfi_upload_images_yuv420 from surfaces: fills every byte of images [g0, g0 + n), alpha included, from frames [0, n) of src.  Ordered like
 * lfi_upload_image_async: the work goes on the copy stream behind the renders already enqueued, later users of the planes are ordered
 * after it by an event, the source must stay valid and unchanged until lfi_upload_wait / lfi_sync; device surfaces must be complete when
 * the call is made (the call does not know the stream that wrote them).  The source is only read.
 *  - LFI_MEM_HOST: the frames' own bytes are copied with 2D copies that honour the pitches (an NV12 chroma plane is one copy; a tight batch
 *    whose W is a multiple of 8 and whose H is even is one copy per chunk) into the staging buffer of lfi_upload_images_yuv420, in its
 *    chunks of at most 16 frames or 256 MiB, each followed by one launch.
 *  - LFI_MEM_DEVICE: where base, frame_stride, both pitches and the offsets are multiples of 16 the surfaces are read in place: no copy, no
 *    staging buffer, ONE launch for all n frames.  Otherwise device-to-device 2D copies bring the frames into the staging buffer, in the
 *    same chunks.  Nothing crosses PCIe either way.  The pointer must be device memory of the context's GPU that covers the n frames.
 * LFI_EINVAL, the context usable, the grid and the staging buffer untouched: whatever lfi_upload_images_yuv420 refuses of grid, released
 * inputs, row window, range of images, matrix, range and chroma; src refused by lfi_yuv_surfaces_check; LFI_MEM_DEVICE with a pointer that
 * is not device memory of the context's device or whose allocation ends before the last frame does. */
int lfi_upload_images_yuv(lfi_ctx *ctx, int g0, int n, int matrix, int range, int chroma, const lfi_yuv_surfaces *src);
/* lfi_upload_images_yuv for a context that holds only the derived planar copy of its inputs (lfi_release_inputs): the n frames of src are
 * expanded STRAIGHT into the three byte planes of images [g0, g0 + n) of that copy, padding included, in one pass and one kernel — 1.5 bytes
 * read and 3 written per pixel, no RGBA image in between, no rebuild afterwards.  Every byte is what the copy would hold had the frames gone
 * through lfi_upload_images_yuv before lfi_release_inputs: byte j of a row of plane (g, c) is channel c of pixel
 * clamp(j - padx - phase[g], 0, W - 1) of the image the definition above gives (lfi_debug_derived_layout).  The copy keeps its layout, its
 * phases and its validity; renders enqueued before the call read the old frames, renders enqueued after it the new ones, without a host wait.
 * Source handling (host: staged in chunks of at most 16 frames or 256 MiB; device: in place in ONE launch where everything is a multiple of
 * 16, else staged device-to-device), ordering (the copy stream, lfi_upload_wait / lfi_sync) and the arguments are lfi_upload_images_yuv's;
 * tight I420 host frames go in through lfi_yuv_surfaces_packed.  The kernel works on spans of LFI_YUV_DERIVED_SPAN bytes of a plane row.
 * LFI_EINVAL, the context usable, the copy and the staging buffer untouched: a context that still holds its RGBA planes (the call writes
 * the planar copy alone: lfi_release_inputs first); no grid; a row window; and whatever lfi_upload_images_yuv refuses of the range of
 * images, matrix, range, chroma and src. */
#define LFI_YUV_DERIVED_SPAN 384
int lfi_upload_images_yuv_derived(lfi_ctx *ctx, int g0, int n, int matrix, int range, int chroma, const lfi_yuv_surfaces *src);
/* lfi_download_views_yuv420 into surfaces: views [v0, v0 + n) become frames [0, n) of dst.  Synchronous, ordered like
 * lfi_download_views_yuv420; both view layouts are read in place; writes no view and no map.  ONLY the planes' own bytes of dst are
 * written: pitch padding and gaps between planes and frames keep their values.
 *  - LFI_MEM_HOST: one launch converts the views into device frames the context owns (those of lfi_download_views_yuv420), 2D copies that
 *    honour the pitches carry them out.
 *  - LFI_MEM_DEVICE: where base, frame_stride, both pitches and the offsets are multiples of 16 the kernel writes the caller's surfaces
 *    directly (whole blocks as words, a ragged last block of a row byte by byte); otherwise through the device frames and device-to-device
 *    2D copies.  The frames are complete when the call returns.
 * LFI_EINVAL, the context usable and dst untouched: whatever lfi_download_views_yuv420 refuses of views, matrix, range and row window; dst
 * refused by lfi_yuv_surfaces_check; LFI_MEM_DEVICE with a pointer that is not device memory of the context's device or whose allocation
 * ends before the last frame does. */
int lfi_download_views_yuv(lfi_ctx *ctx, int v0, int n, int matrix, int range, const lfi_yuv_surfaces *dst);
/* A QUILT VIDEO frame: the scaled quilt as ONE 8-bit YUV 4:2:0 frame, made on the device — light-field video as holographic displays and
 * players take it, one quilt per time step in ordinary 4:2:0 video.  No new arithmetic: let Q be the RGBA image that
 * lfi_download_quilt_scaled(ctx, tiles_x, tiles_y, v0, tile_w, tile_h, ...) delivers — QW = tiles_x*tile_w by QH = tiles_y*tile_h pixels, tiles
 * left to right and top to bottom, the exact area filter, tile = W x H the views themselves.  The frame is what lfi_download_views_yuv420's
 * definition makes of Q taken as one view of QW x QH: Y per pixel; Cb and Cr from the sums over the four pixels of each 2 x 2 block of Q's
 * coordinates (a block straddles two or four tiles where a tile size is odd); an odd last column or row replicated; matrix and range select
 * one of the four coefficient sets.
 * dst describes ONE frame (n = 1) of QW x QH: I420 or NV12, any pitches and offsets that lfi_yuv_surfaces_check(dst, QW, QH, 1) accepts, in
 * host or device memory.  Synchronous, ordered like lfi_download_quilt_scaled; both view layouts, and attached views, are read in place; no
 * view, map or kept view is written.  ONLY the planes' own bytes of dst are written: pitch padding and gaps keep their values.
 *  - The destination is routed as lfi_download_views_yuv routes it: LFI_MEM_DEVICE with base, frame_stride, pitches and offsets multiples of 16 is written
 *    by the kernel itself; everything else goes through one device frame the context owns (that of lfi_download_views_yuv420:
 *    lfi_memory.workspace_bytes, LFI_POISON_SCRATCH) and copies of the frame's own bytes.
 *  - EVEN tile_w and tile_h (what encoders take): every 2 x 2 block lies inside one tile, and ONE kernel resizes and converts — no RGBA quilt
 *    exists anywhere, the quilt buffer of lfi_download_quilt_scaled is neither reserved nor touched.
 *  - An ODD tile_w or tile_h: blocks straddle tiles; the RGBA quilt is made in lfi_download_quilt_scaled's device buffer and converted by the
 *    kernel of lfi_download_views_yuv as one view of QW x QH (two launches).
 * LFI_EINVAL, the context usable, dst and lfi_memory.workspace_bytes untouched: whatever lfi_download_quilt_scaled refuses (nothing rendered,
 * the tiles or views out of range, a tile size outside the limits, views of more than 65535 pixels along an axis, a row window); an unknown
 * matrix or range; dst refused by lfi_yuv_surfaces_check for (QW, QH, 1); LFI_MEM_DEVICE with a pointer that is not device memory of the
 * context's device or whose allocation ends before the frame does. */
int lfi_download_quilt_yuv(lfi_ctx *ctx, int tiles_x, int tiles_y, int v0, int tile_w, int tile_h, int matrix, int range, const lfi_yuv_surfaces *dst);
/* RGB-D VIDEO frames: a view and a focus map side by side in one 8-bit YUV 4:2:0 frame — the colour image with its depth map beside it, as
 * holographic players ("RGB-D photo / video") and 2D-plus-depth displays take it.  Views [v0, v0 + n) become frames [0, n) of dst, each
 * 2*tile_w x tile_h: the colour in the left half, the depth in the right half.  No new arithmetic.  For frame k:
 *  - V is view v0 + k.
 *  - M is the R byte plane of the chosen map, W x H: without LFI_RGBD_VIEW_MAPS the context's map map_k (0 or 1, what lfi_download_map
 *    delivers), the same for every frame; with it, view v0 + k's own map map_k of lfi_view_focus_maps (what lfi_download_view_map delivers).
 *  - d = M, or 255 - M with LFI_RGBD_INVERT.  The inversion happens BEFORE the resize: 255 - mean rounds ties the other way.
 *  - D is the RGBA image (d, d, d, 255).
 *  - Frame k is what lfi_download_quilt_yuv's definition makes of the 2 x 1 quilt whose tiles are V and D: the exact area filter to
 *    tile_w x tile_h, then lfi_download_views_yuv420's arithmetic on the 2*tile_w x tile_h image taken as one view.
 * Consequences of the coefficient tables, which the kernel relies on (csrc/hip/rgbd_yuv.hpp; the grey image D is never made):
 *  - the resized D is grey with value s, the rounded area mean of d;
 *  - the depth half's luma is Y = y_off + ((S*s + 2^15) >> 16) with S = 56284 (limited range) or 65536 (full range, so Y = s);
 *  - every chroma sample of the depth half is exactly 128: the chroma coefficients sum to 0 and (2^25 + 2^17) >> 18 = 128.
 * Limits: tile_w and tile_h EVEN (no 2 x 2 block may straddle the halves, and encoders take even sizes) and within
 * lfi_download_quilt_scaled's limits; map_k 0 or 1; no flag bits other than the two below.
 * dst is routed exactly as lfi_download_views_yuv routes n frames: LFI_MEM_DEVICE with base, frame_stride, pitches and offsets multiples of
 * 16 is written by the kernel itself; everything else goes through device frames the context owns (lfi_memory.workspace_bytes,
 * LFI_POISON_SCRATCH) and copies of the planes' own bytes.  ONLY the planes' own bytes are written: padding and gaps keep their values.
 * ONE kernel launch makes all 2n halves; both view layouts, and attached views, are read in place; no view and no map is written.
 * Synchronous.  The context's maps are read in the order lfi_download_map reads them (behind the filter that makes map 1), per-view maps
 * in the order lfi_download_view_map reads them.
 * LFI_EINVAL, the context usable, dst and lfi_memory.workspace_bytes untouched: nothing rendered; a row window; n < 1 or views outside
 * [0, views); an odd or out-of-range tile size; a bad map_k or unknown flags; LFI_RGBD_VIEW_MAPS while the per-view maps are not in use (no
 * successful lfi_view_focus_maps for the current parameters); an unknown matrix or range; dst refused by
 * lfi_yuv_surfaces_check(dst, 2*tile_w, tile_h, n); LFI_MEM_DEVICE with a pointer that is not device memory of the context's device or
 * whose allocation ends before the last frame does. */
enum { LFI_RGBD_INVERT = 1u, LFI_RGBD_VIEW_MAPS = 2u };
int lfi_download_rgbd_yuv(lfi_ctx *ctx, int v0, int n, int map_k, uint32_t flags, int tile_w, int tile_h, int matrix, int range, const lfi_yuv_surfaces *dst);
/* CHROMA SITING.  Everything above defines chroma as centre-sited (JPEG's and MPEG-1's convention, Y4M's C420jpeg).  MPEG-2, H.264, HEVC and
 * AV1 video site chroma on the LEFT: a chroma sample is co-sited with the even luma column and lies between the two rows (Y4M's C420mpeg2;
 * what decoders leave as NV12 surfaces and what encoders assume of untagged frames).  The siting is a context setting, one for frames that
 * come in and one for frames that go out.  Under LFI_YUV_SITING_LEFT everything not named here stays as defined above: luma, the
 * coefficient tables, the geometry of a frame, cw and ch.
 *  - OUTPUT, left-sited.  For chroma sample (cx, cy): rows y_j = min(2cy + j, H - 1), j in {0, 1}; columns xl = max(2cx - 1, 0), xc = 2cx,
 *    xr = min(2cx + 1, W - 1).  The sums are
 *        SR = sum over j of [ R(xl, y_j) + 2*R(xc, y_j) + R(xr, y_j) ]          (SG, SB likewise; total weight 8)
 *    and
 *        Cb[cy][cx] = min(255, (2^26 + 2^18 + uR*SR + uG*SG + uB*SB) >> 19)     Cr likewise with the Cr coefficients
 *    the [1 2 1]/4 filter of left siting horizontally, the box vertically, one rounding.  The bracket lies in (0, 2^28] (extremes 524,288
 *    and 134,217,728 over the four rows): unsigned 32-bit arithmetic.  Limited range stays in [16, 240], full range reaches 256 before the
 *    min, every grey gives exactly 128, and a uniform image gives exactly the centre-sited frame.
 *  - INPUT, left-sited, LFI_CHROMA_BILINEAR.  With cx = x >> 1, cy = y >> 1 and ny as above:
 *        h(r) = 4*U[r][cx]                                    (even x)
 *        h(r) = 2*U[r][cx] + 2*U[r][min(cx + 1, cw - 1)]      (odd x)
 *        SU   = 3*h(cy) + h(ny)
 *    SU is in sixteenths as above, and R, G, B follow from it as above.  LFI_CHROMA_NEAREST gives the same bytes under either siting: an odd
 *    column is equally far from both samples and keeps cx.
 * in_siting governs lfi_upload_images_yuv420, lfi_upload_images_yuv and lfi_upload_images_yuv_derived; out_siting governs
 * lfi_download_views_yuv420, lfi_download_views_yuv, lfi_render_stream_yuv420 and lfi_download_quilt_yuv.  Sources, destinations, routing,
 * chunking, ordering and refusals of these calls are the same under both sitings, with two exceptions:
 *  - lfi_download_quilt_yuv under LEFT output is by definition the left-sited frame of lfi_download_quilt_scaled's image taken as one view
 *    (chroma filters across tile edges exactly as that says); it takes the two-launch route of odd tile sizes for even tile sizes too.
 *  - lfi_download_rgbd_yuv under LEFT output returns LFI_EINVAL (the context stays usable): the filter would mix the colour half and the
 *    depth half in the column between them.  Left-sited RGB-D frames are out of scope.
 * The default is centre / centre, under which every call does exactly what it did before the setting existed.  The setting lives until it
 * is changed: lfi_set_grid, lfi_set_params and lfi_set_row_window leave it alone.  LFI_EINVAL for an unknown value; the setting is kept.
 * Not covered: top-left siting (co-sited both ways) and Y4M's C420paldv. */
enum { LFI_YUV_SITING_CENTRE = 0, LFI_YUV_SITING_LEFT = 1 };
int lfi_set_yuv_siting(lfi_ctx *ctx, int in_siting, int out_siting);
int lfi_yuv_siting(lfi_ctx *ctx, int *in_siting, int *out_siting);
/* 10-BIT SURFACES.  What HEVC Main10 and 10-bit AV1 decoders leave and Main10 encoders take: the 8-bit layouts with two bytes per sample.  The
 * depth is a flag on the layout:
 *   LFI_YUV_I010   planar; a sample is a little-endian u16 with the code in bits 9..0  (yuv420p10le, Y4M's C420p10)
 *   LFI_YUV_P010   semi-planar (Cb, Cr interleaved); a sample is a little-endian u16 with the code in bits 15..6  (p010le)
 * Any other value with LFI_YUV_10BIT set is an unknown format (and so is plain 2).  Geometry: that of I420 / NV12 with two bytes per sample;
 * pitches, offsets and strides stay in bytes: y_pitch >= 2*W, c_pitch >= 2*cw (I010) or 4*cw (P010); the tight frame of
 * lfi_yuv_surfaces_packed is 2*(W*H + 2*cw*ch) bytes.  lfi_yuv_surfaces_check additionally refuses, for these formats only, an odd base,
 * pitch, offset or frame_stride (a sample must not straddle an odd address).  Reading: I010 code = word & 1023, P010 code = word >> 6 (the
 * other six bits are ignored).  Writing: the other six bits are written as 0.  Device surfaces are used in place under the same rule as the
 * 8-bit ones: base, frame_stride, pitches and offsets multiples of 16.
 * OUTPUT (views -> frames).  Coefficients with 14 fractional bits: round(c * scale * 2^14), scale = 876/255 (limited luma), 896/255 (limited
 * chroma), 1023/255 (full range); G adjusted so that Y sums to 56284 (limited) or 65729 (full) and Cb and Cr to 0.  The limited sets ARE the
 * 8-bit sets (876/255 * 2^14 = 219/255 * 2^16); the full sets are
 *                   Y (R, G, B)           Cb (R, G, B)             Cr (R, G, B)            y_off10
 *   709 limited   11966, 40254, 4064    -6596, -22188, 28784     28784, -26145, -2639      64
 *   709 full      13974, 47009, 4746    -7531, -25333, 32864     32864, -29851, -3013       0
 *   601 limited   16829, 33039, 6416    -9714, -19070, 28784     28784, -24103, -4681      64
 *   601 full      19653, 38583, 7493   -11091, -21773, 32864     32864, -27519, -5345       0
 *     Y10 = y_off10 + ((yR*R + yG*G + yB*B + 2^13) >> 14)
 *     centre siting:  C10 = min(1023, (2^25 + 2^15 + uR*SR + uG*SG + uB*SB) >> 16)      SR, SG, SB: the 8-bit definition's sums over the 2x2 block
 *     left siting:    C10 = min(1023, (2^26 + 2^16 + uR*SR + uG*SG + uB*SB) >> 17)      SR, SG, SB: the left-sited definition's sums of weight 8
 * Unsigned 32-bit arithmetic, one rounding; the brackets are positive and below 2^27 (centre) and at most 2^28 (left) as in the 8-bit
 * definition.  Over all 2^24 colours: limited range keeps Y in [64, 940] and chroma in [64, 960], full range Y in [0, 1023] and chroma in
 * [1, 1023] after the min; every grey has chroma exactly 512.  A uniform colour survives RGB8 -> 10-bit YUV -> RGB8 (below, nearest chroma)
 * EXACTLY, for all 2^24 colours under all four sets.
 * INPUT (frames -> images).  Chroma in sixteenths exactly as in the 8-bit definition (centre bilinear 9/3/3/1, left-sited 3*h(cy) + h(ny),
 * nearest, the same clamps), of 10-bit codes.  Coefficients round(c * scale * 2^16), scale = 255/876 (limited luma), 255/896 (limited
 * chroma), 255/1023 (full range):
 *                    cY       rV      gU       gV      bU    y_off
 *   709 limited    19077    29372   -3494    -8731   34610    64
 *   709 full       16336    25726   -3060    -7647   30313     0
 *   601 limited    19077    26149   -6419   -13320   33050    64
 *   601 full       16336    22903   -5622   -11666   28947     0
 *     l = 16*cY*(Y10 - y_off),  u = SU - 8192,  v = SV - 8192
 *     R = clamp((l + rV*v + 2^19) >> 20, 0, 255)   G = clamp((l + gU*u + gV*v + 2^19) >> 20, 0, 255)   B = clamp((l + bU*u + 2^19) >> 20, 0, 255)
 * A = 255.  Over all 10-bit code triples the bracket, rounding term included, stays within +-576,213,136 (709 limited, B, Y = U = 1023):
 * int32 with an arithmetic shift, one rounding.  Chroma 512 gives R = G = B; limited 64 -> 0 and 940 -> 255, full 1023 -> 255; codes outside
 * the nominal range are legal and clamped.
 * CALLS.  lfi_upload_images_yuv takes the 10-bit formats under both input sitings and both chroma filters, lfi_download_views_yuv under both
 * output sitings and both view layouts; sources, destinations, routing, chunking and refusals are those of the 8-bit formats.  The device
 * frames the context owns grow to what a 10-bit call needs (lfi_memory.workspace_bytes, LFI_POISON_SCRATCH).  lfi_download_quilt_yuv with
 * a 10-bit dst takes the two-launch route for every tile size: by definition the frame is the 10-bit frame of lfi_download_quilt_scaled's
 * image taken as one view.  LFI_EINVAL, the context usable and nothing touched: a 10-bit format in lfi_upload_images_yuv_derived and in
 * lfi_download_rgbd_yuv.  The ..._yuv420 calls and lfi_render_stream_yuv420 stay 8-bit.  Under the 8-bit formats every byte, launch and
 * allocation is what it was before these formats existed. */
#define LFI_YUV_10BIT 0x100
enum { LFI_YUV_I010 = LFI_YUV_I420 | LFI_YUV_10BIT, LFI_YUV_P010 = LFI_YUV_NV12 | LFI_YUV_10BIT };
/* FRAMES FROM THE DEEP VIEWS (LFI_FLAG_DEEP_VIEWS).  LFI_YUV_DEEP is a SOURCE flag on a 10-bit format, for lfi_download_views_yuv only:
 *   LFI_YUV_I010 | LFI_YUV_DEEP, LFI_YUV_P010 | LFI_YUV_DEEP   the frames of the 10-bit formats, converted from the DEEP planes' 10-bit codes
 *       instead of from the 8-bit views scaled by 876/255: a Main10 encoder gets the render without a first quantisation.  Geometry, routing
 *       (host: staged; device: in place where base, frame_stride, pitches and offsets are multiples of 16, else staged) and refusals are those
 *       of LFI_YUV_I010 / LFI_YUV_P010, under both output sitings;
 *   LFI_YUV_GBRP10 (0x304)   no conversion: three full-size planes G, B, R of H rows each (ffmpeg's gbrp10le: `-f rawvideo -pix_fmt gbrp10le`),
 *       a sample a little-endian u16 with the code in bits 9..0 and the upper six bits 0:
 *           G at the frame's base with y_pitch;  B at c_offset with c_pitch;  R at cr_offset with c_pitch
 *       both pitches >= 2*W, the planes in this order and not overlapping, base, pitches, offsets and frame_stride even; the tight frame of
 *       lfi_yuv_surfaces_packed is 6*W*H bytes.  matrix and range must be valid and are ignored.  A frame is three 2D copies out of the deep
 *       planes, to host or device memory alike (no kernel, no staging buffer; a device pointer is checked as for the other formats).
 * LFI_YUV_DEEP on I010 / P010 says where the samples COME FROM, not where they lie: the context-free lfi_yuv_surfaces_check and
 * lfi_yuv_surfaces_packed, which know no source, keep treating 0x300 and 0x301 as unknown formats - describe the surfaces as LFI_YUV_I010 /
 * LFI_YUV_P010 and set the flag in the descriptor's format for the download, which checks the geometry of the format without it.  LFI_YUV_GBRP10 is
 * a layout of its own and is known to both.  Plain 2, 0x102, 0x200, 0x201, 0x204 and 0x104 stay unknown formats everywhere.  Every other call that takes surfaces (lfi_upload_images_yuv, lfi_upload_images_yuv_derived,
 * lfi_upload_mosaic_yuv[_derived], lfi_download_quilt_yuv, lfi_download_rgbd_yuv) refuses a LFI_YUV_DEEP format with LFI_EINVAL and a message that
 * names LFI_YUV_DEEP.  lfi_download_views_yuv refuses one (LFI_EINVAL, nothing written) unless [v0, v0 + n) lies inside the views of the last
 * deep launch.  Without LFI_YUV_DEEP every byte, launch and allocation is what it was.
 * ARITHMETIC (10-bit RGB codes R, G, B of the deep planes -> 10-bit YUV), integers only.  Coefficients round(c * scale * 2^16), scale = 876/1023
 * (limited luma), 896/1023 (limited chroma), 1 (full range); G adjusted so that Y sums to 56120 (limited) or 65536 (full) and Cb and Cr to 0:
 *                   Y (R, G, B)           Cb (R, G, B)             Cr (R, G, B)            y_off10
 *   709 limited   11931, 40137, 4052    -6576, -22124, 28700     28700, -26068, -2632      64
 *   709 full      13933, 46871, 4732    -7509, -25259, 32768     32768, -29763, -3005       0
 *   601 limited   16780, 32942, 6398    -9685, -19015, 28700     28700, -24033, -4667      64
 *   601 full      19595, 38470, 7471   -11058, -21710, 32768     32768, -27439, -5329       0
 *     Y10 = y_off10 + ((yR*R + yG*G + yB*B + 2^15) >> 16)
 *     centre siting:  C10 = min(1023, (2^27 + 2^17 + uR*SR + uG*SG + uB*SB) >> 18)      SR, SG, SB: the sums over the 2x2 block (clamped as above)
 *     left siting:    C10 = min(1023, (2^28 + 2^18 + uR*SR + uG*SG + uB*SB) >> 19)      SR, SG, SB: the left-sited definition's sums of weight 8
 * Unsigned 32-bit arithmetic, one rounding.  The luma bracket is below 2^26; the chroma brackets lie in (0, 2^28] (centre) and (0, 2^29] (left):
 * the upper ends are reached exactly, by full-range Cb of pure blue and Cr of pure red (32768 * 4092 + 2^27 + 2^17 = 2^28), and the min takes them
 * to 1023.  Every grey has chroma exactly 512; limited range maps 0 -> 64 and 1023 -> 940; full range maps a grey code D to Y = D. */
#define LFI_YUV_DEEP 0x200
enum { LFI_YUV_GBRP10 = 4 | LFI_YUV_10BIT | LFI_YUV_DEEP };

/* Mosaic input: ONE frame that holds all images of the grid as tiles — a camera array packed into one video stream (8 x 8 cameras of
 * 1920 x 1080 in a 15360 x 8640 frame), a Looking-Glass quilt, or the frame lfi_download_quilt_yuv wrote — split into the grid's images on
 * the device.  The inverse of lfi_download_quilt*.  The frame is tiles_x*W by tiles_y*H, W x H the grid's image size: no gutters, no crops.
 *
 * THE MAPPING.  k counts the call's tiles: tile t = first_tile + k of the frame in ROWS order (left to right, then the next tile row) sits at
 * column tx = t % tiles_x of tile row r = t / tiles_x, which is the frame's tile row ty = r, or ty = tiles_y - 1 - r with
 * LFI_MOSAIC_BOTTOM_UP (Looking-Glass quilts start at the bottom left).  tx and ty say where the tile's bytes lie: its top left pixel is
 * (tx*W, ty*H) of the frame.
 *  - LFI_MOSAIC_ROWS: the tile becomes image g0 + k.  The order of lfi_download_quilt*: a quilt of T views is a T x 1 grid.
 *  - LFI_MOSAIC_GRID: the tile is the camera in column tx and row r (BOTTOM_UP: the cameras' rows run from the frame's bottom to its top),
 *    the image the loader makes of the file <r>_<tx>: g = tx*rows + r.  Requires tiles_x == cols, tiles_y == rows, first_tile == 0,
 *    n == cols*rows and g0 == 0.
 * lfi_mosaic_map writes tx, ty and g of tile k (each pointer may be NULL) for a cols x rows grid; LFI_EINVAL, nothing written: m NULL; tiles_x,
 * tiles_y, cols or rows below 1; an unknown order or flag; n < 1, first_tile < 0 or first_tile + n beyond the last tile; g0 < 0 or g0 + n
 * beyond the last image; a GRID mosaic that breaks the rule above; k outside [0, n).  Context-free, needs no GPU.  It is the one definition
 * the entry points, their kernel and the command-line program share. */
enum { LFI_MOSAIC_ROWS = 0, LFI_MOSAIC_GRID = 1 };      /* order */
enum { LFI_MOSAIC_BOTTOM_UP = 1u };                     /* flags */
typedef struct lfi_mosaic {
    int32_t tiles_x, tiles_y;   /* the frame is tiles_x*W by tiles_y*H, W x H the grid's image size */
    int32_t first_tile, n;      /* tiles [first_tile, first_tile + n) in ROWS order */
    int32_t order;
    uint32_t flags;
} lfi_mosaic;
int lfi_mosaic_map(const lfi_mosaic *m, int cols, int rows, int g0, int k, int *tx, int *ty, int *g);
/* A YUV 4:2:0 mosaic.  src describes ONE frame of MW x MH = tiles_x*W x tiles_y*H, LFI_YUV_I420 or LFI_YUV_NV12, host or device memory, any
 * pitches and offsets lfi_yuv_surfaces_check(src, MW, MH, 1) accepts (frame_stride is not used).
 * DEFINITION, no new arithmetic: image g of tile (tx, ty) is what lfi_upload_images_yuv makes of the tile taken as a frame of its own — Y rows
 * [ty*H, ty*H + H) and columns [tx*W, tx*W + W), chroma rows [ty*H/2, ty*H/2 + H/2) and columns [tx*W/2, tx*W/2 + W/2) — under the
 * context's input siting (lfi_set_yuv_siting) and the call's matrix, range and chroma filter.  Chroma neighbours are clamped at the TILE's
 * edges: no value of a neighbouring tile, of pitch padding or of a tile outside [first_tile, first_tile + n) reaches any image.  Images
 * other than the mapped ones are not touched.  W and H must be even (an odd size puts a 2 x 2 chroma block across two tiles).
 * Ordering against uploads, renders, lfi_upload_wait and lfi_sync is lfi_upload_images_yuv's; the source is only read and must stay valid
 * and unchanged until lfi_upload_wait / lfi_sync.
 *  - LFI_MEM_DEVICE where base, both pitches and the offsets are multiples of 16: the frame is read where it lies by ONE launch for all n
 *    tiles, whatever W is (a W that is no multiple of 8 takes a kernel that assembles its pieces from aligned words).  No staging buffer.
 *  - Everything else (host memory, other device descriptors): the frame goes through the staging buffer of lfi_upload_images_yuv in chunks
 *    of whole tile rows, at most 256 MiB and at least one tile row each; a chunk takes one 2D copy per plane of the rows' own bytes — never a
 *    copy per tile — and one launch.
 * LFI_EINVAL, the context usable, the grid and the staging buffer untouched: whatever lfi_upload_images_yuv refuses of grid, released
 * inputs, row window, matrix, range and chroma; a mosaic lfi_mosaic_map refuses for the context's grid; an odd W or H; the 10-bit formats;
 * src refused by lfi_yuv_surfaces_check for (MW, MH, 1); LFI_MEM_DEVICE with a pointer that is not device memory of the context's device
 * or whose allocation ends before the frame does. */
int lfi_upload_mosaic_yuv(lfi_ctx *ctx, const lfi_mosaic *m, int g0, int matrix, int range, int chroma, const lfi_yuv_surfaces *src);
/* lfi_upload_mosaic_yuv for a context that holds only the derived planar copy of its inputs (lfi_release_inputs): the tiles of the frame are
 * expanded STRAIGHT into the three byte planes of their mapped images of that copy, padding included, in one pass — 1.5 bytes read and 3
 * written per pixel, no RGBA image in between, no rebuild afterwards.  DEFINITION, no new arithmetic: after the call the planes of every
 * mapped image g hold what they would hold had the frame gone through lfi_upload_mosaic_yuv before lfi_release_inputs: byte j of a row of
 * plane (g, c) is channel c of pixel clamp(j - padx - phase[g], 0, W - 1) of the image the mosaic definition above gives for g's tile
 * (lfi_debug_derived_layout).  Chroma is clamped at the TILE's edges; no value of a neighbouring tile, of pitch padding or of a tile
 * outside [first_tile, first_tile + n) reaches any plane; images other than the mapped ones keep every byte.  The copy keeps its layout,
 * its phases and its validity, as in lfi_upload_images_yuv_derived, whose ordering this call has too: the work runs on the copy stream
 * behind renders already enqueued, later renders read the new frames without a host wait.  The mosaic, g0, matrix, range, chroma, src and
 * the routing (a device frame with multiples of 16 throughout: in place, ONE launch for all n tiles whatever W is; everything else: the
 * staging buffer in chunks of whole tile rows, one 2D copy per plane and one launch each) are lfi_upload_mosaic_yuv's.
 * LFI_EINVAL, the context usable, the copy, the staging buffer and lfi_memory.workspace_bytes untouched: a context that still holds its
 * RGBA planes (lfi_release_inputs first); no grid; no planar copy; a row window; matrix, range and chroma; and whatever
 * lfi_upload_mosaic_yuv refuses of the mosaic, of an odd W or H, of the frame's size, of the 10-bit formats, of src and of device memory. */
int lfi_upload_mosaic_yuv_derived(lfi_ctx *ctx, const lfi_mosaic *m, int g0, int matrix, int range, int chroma, const lfi_yuv_surfaces *src);
/* An RGBA mosaic in host memory (a quilt PNG): rows of pitch_bytes >= tiles_x*W*4.  By definition lfi_upload_image_async of every tile's
 * rectangle into its mapped image: one 2D copy per tile on the copy stream, no kernel; odd sizes are allowed; ordering, the row window and
 * the lifetime of rgba are lfi_upload_image_async's.  LFI_EINVAL: no grid, a mosaic lfi_mosaic_map refuses, rgba NULL, a pitch too small. */
int lfi_upload_mosaic(lfi_ctx *ctx, const lfi_mosaic *m, int g0, const uint8_t *rgba, size_t pitch_bytes);
/* tests: chunk `chunk` of lfi_upload_mosaic_yuv's staged route for tiles of tile_w x tile_h under a cap of cap_bytes (0: the call's own
 * 256 MiB) — out5 = { first tile row in ROWS order, tile rows, the frame's first tile row copied, first tile k, tiles }.  LFI_EINVAL: a bad
 * mosaic (judged for its natural grid: tiles_x x tiles_y under GRID, n x 1 under ROWS), an odd size, no such chunk.  Needs no GPU. */
int lfi_debug_mosaic_chunk(const lfi_mosaic *m, int tile_w, int tile_h, size_t cap_bytes, int chunk, int32_t *out5);
/* tests: the cap of the staging chunks of lfi_upload_mosaic_yuv and lfi_upload_mosaic_yuv_derived, in place of their own 256 MiB, so that a
 * small frame takes more than one chunk (lfi_debug_mosaic_chunk reports the plan for a cap).  0, the default: the calls' own cap, every
 * byte, copy and launch as without this call.  A context setting; LFI_EINVAL: ctx NULL. */
int lfi_debug_set_mosaic_chunk_cap(lfi_ctx *ctx, size_t cap_bytes);
int lfi_upload_map(lfi_ctx *ctx, int k, const uint8_t *rgba, size_t pitch_bytes); /* tests: inject a focus map */
/* view v's map k (0 or 1) of the per-view maps (lfi_view_focus_maps).  Synchronous.  The upload is a test hook like lfi_upload_map (it
 * allocates the per-view maps if needed and does not put them in use: renders read them after a successful lfi_view_focus_maps). */
int lfi_download_view_map(lfi_ctx *ctx, int v, int k, uint8_t *rgba, size_t pitch_bytes);
int lfi_upload_view_map(lfi_ctx *ctx, int v, int k, const uint8_t *rgba, size_t pitch_bytes);

/* PSNR / SSIM of rendered view v against a reference image on the host, reduced on the device — replaces
 * scripts/imageQualityMetrics.sh:1-12 (ffmpeg psnr / ssim on two PNGs; scripts/compareDirs.sh loops it over directories).  ffmpeg is not
 * part of this product, so the definitions are fixed HERE (the tests restate them in numpy: tests/quality_ref.py):
 *   PSNR  per colour channel c: 10·log10(255² / MSE_c), MSE_c over all pixels; "all" from the mean of the three MSEs;
 *   SSIM  per colour channel: the mean over all 8×8 windows at a stride of 4 pixels (the window set of ffmpeg's ssim filter) of
 *         ((2·μa·μb + C1)(2·σab + C2)) / ((μa² + μb² + C1)(σa² + σb² + C2)), C1 = (0.01·255)², C2 = (0.03·255)², with the window's
 *         biased moments (sums over its 64 pixels); "all" = the mean of the three channels; 1.0 when no window fits.  Alpha is ignored.
 * Squared errors are summed exactly in integers; window SSIMs are summed in fp64.
 * lfi_compare_view IS lfi_compare_views (below) for n = 1 and one host reference with image_stride_bytes = pitch_bytes · H: the same
 * kernels, so out equals that call's out[0].q byte for byte, and the SSIM sums are added in a fixed order — two calls on the same data
 * return the same bits (earlier versions added them with floating-point atomics and could differ in the last bits from run to run;
 * MSE and PSNR, integer sums, are what they were).  Both view layouts are read as they are.  Synchronous.  LFI_EINVAL: nothing rendered
 * yet; a bad view index, pointer or pitch; a row window. */
typedef struct lfi_quality {
    double mse[3], psnr[3], psnr_all; /* identical images: mse 0, psnr +inf */
    double ssim[3], ssim_all;
} lfi_quality;
int lfi_compare_view(lfi_ctx *ctx, int v, const uint8_t *reference_rgba, size_t pitch_bytes, lfi_quality *out);

/* Batch comparison: PSNR / SSIM of n views against n references in one device pass — replaces scripts/compareDirs.sh (a loop of
 * imageQualityMetrics.sh over every file of two result directories: all views against ground truth, or a TEN_WM run against an STD run).
 * The references are host images, or views kept on the device from an earlier render (lfi_keep_views): comparing two methods' renders
 * then moves nothing but the results over PCIe.
 *
 * lfi_keep_views copies views [v0, v0 + n) as they are now, in the current layout, into a reference set the context owns: device to
 * device, in stream order, no host synchronisation (unless the set's size changes: the old allocation is freed).  Later renders do not
 * touch the kept set.  n == 0 frees it.  It is dropped by lfi_set_grid, lfi_set_row_window, lfi_set_output_layout (to another layout) and
 * by a lfi_set_params that changes the number of views; its bytes are counted in lfi_memory.workspace_bytes.
 *
 * lfi_compare_views: out[k] compares view v0 + k with reference k, k in [0, n); out_all (may be NULL) is the aggregate.
 *  - references_rgba != NULL: n host RGBA images, image k at references_rgba + k * image_stride_bytes, rows of pitch_bytes >= W * 4,
 *    image_stride_bytes >= pitch_bytes * H.  They cross PCIe on the context's copy stream in chunks of several images (at most 64 MiB, at
 *    least one image) through two device staging buffers: chunk k + 1 is copied while chunk k is reduced.  Page-locked sources
 *    (lfi_alloc_pinned) are DMA'd in place;
 *  - references_rgba == NULL: the references are the kept views, [v0, v0 + n) must lie inside the kept range (reference k = kept view
 *    v0 + k); one launch covers all n views;
 *  - out[k].q: mse, psnr, psnr_all, ssim, ssim_all exactly as lfi_compare_view defines them (+inf for identical images, ssim = 1.0 when no
 *    window fits); sq_err, differing_bytes, max_abs_diff and windows are exact integers;
 *  - out_all: mse[c] = (sum over the views of sq_err[c]) / (n * W * H), computed from the integers; psnr, psnr_all from it as above;
 *    ssim[c] = the mean of the per-view ssim[c], added in view order; ssim_all = the mean of the three;
 *  - deterministic: window SSIMs are added in a fixed order (per lane, wave, workgroup, then per view: csrc/hip/quality_batch.hpp), no
 *    floating-point atomics: two calls on the same data return the same bits;
 *  - both view layouts are read as they are (no staging plane), kept references in the layout they were kept in;
 *  - synchronous; ordered after the work on the stream in use (a caller's too: lfi_set_stream) and after pending uploads; one
 *    device-to-host copy carries all results.  It writes no view, map or kept view.  It only reads views: it works after
 *    lfi_release_inputs and with per-view offsets or maps set.  The staging buffers and the partial sums belong to the context
 *    (lfi_memory.workspace_bytes, LFI_POISON_SCRATCH); every byte a call reads of them it has written itself;
 *  - LFI_EINVAL, the context stays usable: nothing rendered yet; a range outside [0, views) or n < 1; a pitch or stride too small;
 *    out == NULL; a row window; NULL references without a kept set or with one that does not cover the range (a set kept in another
 *    layout has been dropped). */
typedef struct lfi_view_quality {
    lfi_quality q;             /* the definitions at lfi_compare_view above, unchanged */
    uint64_t sq_err[3];        /* sum of (a-b)^2 per colour channel: exact */
    uint64_t differing_bytes;  /* colour bytes (R, G, B; alpha ignored) with a != b: exact */
    uint64_t windows;          /* 8x8 windows at stride 4 that fit */
    int32_t max_abs_diff;      /* largest |a-b| over the colour bytes: exact */
} lfi_view_quality;
int lfi_keep_views(lfi_ctx *ctx, int v0, int n);
int lfi_compare_views(lfi_ctx *ctx, int v0, int n, const uint8_t *references_rgba, size_t pitch_bytes, size_t image_stride_bytes, lfi_view_quality *out,
                      lfi_quality *out_all);

/* Page-locked host memory for uploads / downloads at full PCIe rate (hipHostMalloc); optional — any host pointer works. */
int lfi_alloc_pinned(size_t bytes, void **out_ptr);
int lfi_free_pinned(void *ptr);

/* ---- plumbing ------------------------------------------------------------------------------------------------- */

/* enqueue on a caller-owned hipStream_t (NULL restores the context's own stream).  Work already enqueued on the stream in use so
 * far (fills, uploads, the derived input copy, focus maps, renders) is ordered before everything enqueued on the new one by an
 * event — no host synchronisation; the stream switched away from must still exist at the time of the call. */
int lfi_set_stream(lfi_ctx *ctx, void *hip_stream);
/* choose a kernel variant by name for a method — or for the focus-map estimate with LFI_KERNEL_FOCUS_ESTIMATE —
 * ("auto" = default); used by the benchmark harness and the parity tests */
int lfi_set_variant(lfi_ctx *ctx, int method, const char *name);
/* comma separated variant names available for a method */
const char *lfi_list_variants(int method);

/* ---- debug / parity hooks --------------------------------------------------------------------------------------- */

/* unclamped warped sample coordinates of image g for every pixel ([H][W] int2), computed on the device:
 * focusCoords (src/kernels.cu:72-82).  Synchronous. */
int lfi_download_coords(lfi_ctx *ctx, int g, int all_focus, int map_index, lfi_int2 *out_hw);
/* accumulator values before quantisation ([H][W][3] float) of view v: fp32 sums for STD, the fp16-rounded value for
 * TEN_WM.  Renders view v again into a scratch buffer.  Synchronous. */
int lfi_download_prequant(lfi_ctx *ctx, int method, int all_focus, int v, float *out_hw3);
/* hardware probe: C[32x32] = A[32x16] (fp16 bits) · B[16x32] (fp16 bits) with one v_mfma_f32_32x32x16_f16,
 * row-major in/out — checks the fragment lane maps and fp16-subnormal handling with exact data */
int lfi_debug_mfma_f16(lfi_ctx *ctx, const uint16_t *a_32x16, const uint16_t *b_16x32, float *c_32x32);
/* hardware probe: gfx950's three-operand packed fp16 minimum / maximum (v_pk_minimum3_f16 / v_pk_maximum3_f16) on u16 lanes that
 * hold bytes, i.e. fp16 subnormal bit patterns, over all 256³ byte triples (twice: once per half) against integer min / max;
 * *out_mismatches = the number of halves that differ (0 on hardware that leaves subnormals alone).  The focus-map range passes
 * reduce two views per instruction with them (csrc/hip/focus_factored.hpp; FocusMap::ElementRange, src/kernels.cu:173-194). */
int lfi_debug_pk_minmax3_f16(lfi_ctx *ctx, uint32_t *out_mismatches);
/* hardware probe: C[32x32] = A[32xk] · B[kx32] accumulated as the kernels accumulate — shape 0: k/16 chained
 * v_mfma_f32_32x32x16_f16, shape 1: k/32 chained v_mfma_f32_16x16x32_f16 per quadrant; k a multiple of 32, ≤ 256.  Measures the
 * matrix pipe's fp32 accumulation error, which the default STD kernel's rounding band assumes a bound for. */
int lfi_debug_mfma_f16_chain(lfi_ctx *ctx, int shape, int k, const uint16_t *a_32xk, const uint16_t *b_kx32, float *c_32x32);
/* Test hook: fill the selected device buffers of the context with `byte` (hipMemsetAsync on the context's stream, ordered like every
 * other call), so that a test which renders or builds a focus map afterwards sees every byte the call leaves unwritten.  Buffers not
 * allocated yet are skipped.  Poisoning never changes the result of a later call: caches in the poisoned memory are marked stale and
 * rebuilt in full by their next user (the estimate's padded planes; the planar copy, as after lfi_grid_modified).
 *   VIEWS            the views in the current layout (attached ones too)
 *   SCRATCH          the planar layout's RGBA scratch copy of the views, the download staging plane, the pre-quantisation buffer, the
 *                    quilt buffer (lfi_download_native's scaled tiles too) and its native image, the YUV 4:2:0 device frames and lfi_upload_images_yuv420's staged frames, lfi_render_stream's second set of views and lfi_compare_views' staging buffers, partial sums and per-view records
 *                    (not the kept views: they are data)
 *   MAPS             both focus maps
 *   FOCUS_WORKSPACE  all of the focus-map estimate's workspace, and lfi_focus_curve's / lfi_focus_tiles' (the curves, the results and the partial sums)
 *   DERIVED          the planar copy of the inputs — refused (LFI_EINVAL) after lfi_release_inputs: it is then the only copy
 *   VIEW_MAPS        the per-view focus maps of lfi_view_focus_maps, every view's pair
 *   DEEP             the deep planes of LFI_FLAG_DEEP_VIEWS, all views' (they stay valid: data, like the views) */
enum { LFI_POISON_VIEWS = 1, LFI_POISON_SCRATCH = 2, LFI_POISON_MAPS = 4, LFI_POISON_FOCUS_WORKSPACE = 8, LFI_POISON_DERIVED = 16,
       LFI_POISON_VIEW_MAPS = 32, LFI_POISON_DEEP = 64 };
int lfi_debug_poison(lfi_ctx *ctx, uint32_t what, uint8_t byte);
/* Test hooks: the derived planar copy of the inputs, byte for byte.  The copy is [N][3][rows][pitch_bytes] bytes: per image three byte planes
 * (R, G, B) of the rows the context holds; byte j of a plane row of image g holds pixel clamp(j - padx - phase[g], 0, W - 1), so every row is
 * padded on both sides with its edge pixels; reach is the largest horizontal offset the padding serves.  Valid whenever the copy is current
 * — after lfi_release_inputs, or once a render that reads the copy (or lfi_prepare) has brought it up to date with the RGBA planes — else
 * LFI_EINVAL.  lfi_debug_derived_layout writes the layout and, where phases_n is not NULL, the N per-image phases; no device work.
 * lfi_debug_download_derived copies the planes of images [g0, g0 + n) to out ([n][3][rows][pitch_bytes]); synchronous, in stream order
 * behind renders and uploads. */
typedef struct lfi_derived_layout {
    size_t pitch_bytes;
    int rows, padx, reach, n;
} lfi_derived_layout;
int lfi_debug_derived_layout(lfi_ctx *ctx, lfi_derived_layout *out, int32_t *phases_n);
int lfi_debug_download_derived(lfi_ctx *ctx, int g0, int n, uint8_t *out);
/* Test hook of the ordering tests (tests/stream_order.py): out3 receives the hipStream_t of the context's own compute stream, of its copy
 * stream and of its side stream, in that order.  The copy and the side stream are created if they do not exist yet, exactly as their first
 * user would create them (the side stream with the highest priority); no other effect, no device work.  The handles belong to the context
 * and die with it.  A test may enqueue work of its own on them (a delay, an event) to hold the library to its stream order. */
int lfi_debug_streams(lfi_ctx *ctx, void **out3);

#ifdef __cplusplus
}
#endif
#endif /* LFI_H */
