// lfi_hip.hip — the C-ABI of include/lfi.h on HIP for gfx950: every extern "C" entry point.  This translation unit is the whole
// device-facing half of the reference's Interpolator (reference src/interpolator.cu:13-154, 194-316); the arithmetic that produces
// the parameters stays in the host code above the ABI (lfinterpolator_amd/csrc/host).  Its parts:
//   lfi_context.hpp      the context (device memory, streams, parameter block) and its helpers
//   lfi_dispatch.hpp     variant tables, kernel launchers, the derived planar copy, launch_blend
//   lfi_focus_sched.hpp  the focus-map estimate's workspace and pass graph; the focus curve's launches
//   lfi_rccl.hpp         RCCL loader for lfi_broadcast_grid
#include "lfi_context.hpp"
#include "lfi_dispatch.hpp"
#include "lfi_focus_sched.hpp"
#include "quilt_scaled.hpp"
#include "quilt_yuv.hpp"
#include "rgbd_yuv.hpp"
#include "native_filter.hpp"
#include "native_image.hpp"
#include "yuv420.hpp"
#include "yuv420_upload.hpp"
#include "yuv_surfaces.hpp"
#include "yuv10.hpp"
#include "deep_yuv.hpp"
#include "yuv_mosaic.hpp"
#include "yuv_mosaic_derived.hpp"
#include "yuv_derived.hpp"
#include "lfi_rccl.hpp"

extern "C" {

int lfi_abi_version(void)
{
    return LFI_ABI_VERSION;
}

int lfi_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if(e != hipSuccess)
    {
        g_create_error = std::string("hipGetDeviceCount: ") + hipGetErrorString(e);
        return LFI_ENODEVICE;
    }
    return n;
}

const char *lfi_last_error(const lfi_ctx *ctx)
{
    return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

int lfi_create(int device, lfi_ctx **out_ctx)
{
    if(!out_ctx)
        return fail(nullptr, LFI_EINVAL, "out_ctx is NULL");
    *out_ctx = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if(e != hipSuccess || n <= 0)
        return fail(nullptr, LFI_ENODEVICE,
                    std::string("no HIP device available (") + (e != hipSuccess ? hipGetErrorString(e) : "device count 0") +
                        "); this library has no CPU fallback");
    if(device < 0 || device >= n)
        return fail(nullptr, LFI_EINVAL, "device index out of range");
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if(e != hipSuccess)
        return fail(nullptr, LFI_EHIP, std::string("hipGetDeviceProperties: ") + hipGetErrorString(e));
    if(std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, LFI_ENODEVICE,
                    std::string("device is ") + prop.gcnArchName + "; the kernels in this library are built for gfx950 only");
    lfi_ctx *c = new lfi_ctx();
    c->device = device;
    c->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if(hipSetDevice(device) != hipSuccess || c->own_stream.ensure() != hipSuccess || c->ev0.ensure(hipEventDefault) != hipSuccess ||
       c->ev1.ensure(hipEventDefault) != hipSuccess || c->ev_order.ensure() != hipSuccess)
    {
        delete c; // releases what was created
        return fail(nullptr, LFI_EHIP, "could not create stream/events on the device");
    }
    c->stream = c->own_stream;
    *out_ctx = c;
    return LFI_OK;
}

int lfi_destroy(lfi_ctx *ctx)
{
    if(!ctx)
        return LFI_EINVAL;
    (void)hipSetDevice(ctx->device); // stays current while the members go
    (void)hipStreamSynchronize(ctx->stream);
    if(ctx->aux_stream)
        (void)hipStreamSynchronize(ctx->aux_stream); // a focus-map filter may still run there
    if(ctx->copy_stream)
        (void)hipStreamSynchronize(ctx->copy_stream);
    // every buffer, event and stream is a member that releases itself, the streams last (lfi_context.hpp)
    delete ctx;
    return LFI_OK;
}

int lfi_set_stream(lfi_ctx *ctx, void *hip_stream)
{
    if(!ctx)
        return LFI_EINVAL;
    hipStream_t next = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->own_stream;
    if(next == ctx->stream)
        return LFI_OK;
    // The context keeps device state that launches on the new stream depend on and that may still be in flight on the old one: the
    // input planes (lfi_fill_synthetic, uploads), the derived planar copy (planar_build), the focus maps and workspace, the views.
    // Everything enqueued so far is ordered before everything enqueued from now on, without blocking the host.
    if(int rc = bind(ctx))
        return rc;
    if(int rc = join_filter(ctx))
        return rc;
    LFI_HIP(ctx, hipEventRecord(ctx->ev_order, ctx->stream));
    LFI_HIP(ctx, hipStreamWaitEvent(next, ctx->ev_order, 0));
    ctx->stream = next;
    return LFI_OK;
}

int lfi_set_grid(lfi_ctx *ctx, int cols, int rows, int width, int height)
{
    if(!ctx)
        return LFI_EINVAL;
    if(cols < 1 || rows < 1 || width < 1 || height < 1)
        return fail(ctx, LFI_EINVAL, "grid dimensions must be positive");
    if((long)cols * rows > LFI_MAX_IMAGES)
        return fail(ctx, LFI_EINVAL, "more than LFI_MAX_IMAGES (256) grid images");
    // device addressing: pixel indices are 32-bit (W·H ≤ 2^26 leaves room for the ×4 bytes and the per-image strides the kernels fold
    // into scalar bases), and rows / columns are multiplied with 24-bit multiplies (__umul24: blend_persist all-focus, blend_p3)
    if((size_t)width * height > (size_t)1 << 26 || width >= (1 << 24) || height >= (1 << 24))
        return fail(ctx, LFI_EINVAL, "image too large (width·height ≤ 2^26 and width, height < 2^24)");
    if(int rc = bind(ctx))
        return rc;
    if(int rc = lfi_upload_wait(ctx))
        return rc;
    if(int rc = join_filter(ctx))
        return rc;
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    free_params(ctx);
    free_view_rows(ctx);
    free_views(ctx);
    drop_kept(ctx);
    free_grid(ctx);
    ctx->cols = cols;
    ctx->rows = rows;
    ctx->n = cols * rows;
    ctx->width = width;
    ctx->height = height;
    ctx->in_y0 = ctx->out_y0 = 0;
    ctx->in_rows = ctx->out_rows = height;
    ctx->windowed = false;
    LFI_HIP(ctx, ctx->grid.fit(plane_bytes(ctx) * ctx->n));
    touch_all(ctx);
    ctx->grid_tracked = true;
    LFI_HIP(ctx, ctx->maps.fit(plane_bytes(ctx) * 2));
    LFI_HIP(ctx, hipMemsetAsync(ctx->maps.get(), 0, plane_bytes(ctx) * 2, ctx->stream));
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LFI_OK;
}

int lfi_set_row_window(lfi_ctx *ctx, int out_y0, int out_y1, int in_y0, int in_y1)
{
    if(!ctx)
        return LFI_EINVAL;
    if(!ctx->n)
        return fail(ctx, LFI_EINVAL, "lfi_set_grid has not been called");
    if(!(0 <= out_y0 && out_y0 < out_y1 && out_y1 <= ctx->height && 0 <= in_y0 && in_y0 < in_y1 && in_y1 <= ctx->height))
        return fail(ctx, LFI_EINVAL, "row window outside the image");
    if(int rc = bind(ctx))
        return rc;
    if(int rc = lfi_upload_wait(ctx))
        return rc;
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    free_params(ctx);
    free_views(ctx);
    drop_kept(ctx);
    drop_inputs(ctx); // the staging plane too: sized for the window in force when it was allocated (a larger window overflowed it)
    ctx->in_y0 = in_y0;
    ctx->in_rows = in_y1 - in_y0;
    ctx->out_y0 = out_y0;
    ctx->out_rows = out_y1 - out_y0;
    ctx->windowed = !(in_y0 == 0 && in_y1 == ctx->height && out_y0 == 0 && out_y1 == ctx->height);
    LFI_HIP(ctx, ctx->grid.fit(in_plane_bytes(ctx) * ctx->n));
    touch_all(ctx);
    ctx->grid_tracked = true;
    return LFI_OK;
}

int lfi_upload_image(lfi_ctx *ctx, int g, const uint8_t *rgba, size_t pitch_bytes)
{
    if(!ctx)
        return LFI_EINVAL;
    if(!ctx->grid && !ctx->inputs_released)
        return fail(ctx, LFI_EINVAL, "lfi_set_grid has not been called");
    if(g < 0 || g >= ctx->n || !rgba || pitch_bytes < (size_t)ctx->width * 4)
        return fail(ctx, LFI_EINVAL, "bad image index, pointer or pitch");
    if(int rc = bind(ctx))
        return rc;
    if(int rc = join_uploads(ctx))
        return rc;
    if(ctx->inputs_released)
    {
        // the RGBA planes are gone: the image goes through a one-image staging plane straight into its planes of the planar copy
        LFI_HIP(ctx, ctx->stage_plane.reserve(in_plane_bytes(ctx))); // (dropped with the row window it was sized for: drop_stage_plane)
        LFI_HIP(ctx, hipMemcpy2DAsync(ctx->stage_plane.get(), (size_t)ctx->width * 4, rgba + (size_t)ctx->in_y0 * pitch_bytes, pitch_bytes, (size_t)ctx->width * 4,
                                      ctx->in_rows, hipMemcpyHostToDevice, ctx->stream));
        // planar_build reads image g at grid + g·plane: hand it a base that puts the staging plane there
        hipLaunchKernelGGL(lfi::planar_build, dim3((ctx->planar_pitch / 4 + 255) / 256, ctx->in_rows, 1), dim3(256), 0, ctx->stream,
                           ctx->stage_plane.get() - in_plane_bytes(ctx) * (size_t)g, ctx->planar.get(), ctx->width, ctx->in_rows, ctx->planar_pitch,
                           ctx->planar_padx, ctx->d_planar_phase.as<int32_t>(), g);
        LFI_HIP(ctx, hipGetLastError());
        LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return LFI_OK;
    }
    // rgba addresses row 0 of the whole image; only the rows this context holds are copied
    LFI_HIP(ctx, hipMemcpy2DAsync(ctx->grid.get() + in_plane_bytes(ctx) * g, (size_t)ctx->width * 4, rgba + (size_t)ctx->in_y0 * pitch_bytes,
                                  pitch_bytes, (size_t)ctx->width * 4, ctx->in_rows, hipMemcpyHostToDevice, ctx->stream));
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    touch_images(ctx, g, g + 1);
    if(ctx->eager_planar && ctx->have_params)
        (void)ensure_planar(ctx); // this image's planes of the derived copy, now (stream-ordered; a failure leaves it to the next render)
    return LFI_OK;
}

int lfi_upload_image_async(lfi_ctx *ctx, int g, const uint8_t *rgba, size_t pitch_bytes)
{
    if(!ctx)
        return LFI_EINVAL;
    if(ctx->inputs_released)
        return lfi_upload_image(ctx, g, rgba, pitch_bytes); // released inputs: through the staging plane, synchronously
    if(!ctx->grid)
        return fail(ctx, LFI_EINVAL, "lfi_set_grid has not been called");
    if(g < 0 || g >= ctx->n || !rgba || pitch_bytes < (size_t)ctx->width * 4)
        return fail(ctx, LFI_EINVAL, "bad image index, pointer or pitch");
    if(int rc = bind(ctx))
        return rc;
    if(int rc = ensure_copy_stream(ctx))
        return rc;
    if(!ctx->uploads_pending)
    {
        // first copy of a batch: renders already enqueued on the compute stream may still read the planes
        LFI_HIP(ctx, hipEventRecord(ctx->ev_order, ctx->stream));
        LFI_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_order, 0));
    }
    // rgba addresses row 0 of the whole image; the rows this context holds are copied.  A page-locked source is DMA'd in place
    // (the call returns at once); a pageable one is staged by the HIP runtime through its own page-locked buffers before the call
    // returns (≈45–50 GB/s of host time on this platform — a staging ring of our own with a host memcpy in front measured
    // 20 GB/s, profiles/r02_upload_time.txt), so the caller's buffer is free on return either way.
    const size_t row_bytes = (size_t)ctx->width * 4;
    LFI_HIP(ctx, hipMemcpy2DAsync(ctx->grid.get() + in_plane_bytes(ctx) * g, row_bytes, rgba + (size_t)ctx->in_y0 * pitch_bytes, pitch_bytes, row_bytes,
                                  ctx->in_rows, hipMemcpyHostToDevice, ctx->copy_stream));
    ctx->uploads_pending = true;
    touch_images(ctx, g, g + 1);
    return LFI_OK;
}

int lfi_upload_wait(lfi_ctx *ctx)
{
    if(!ctx)
        return LFI_EINVAL;
    if(int rc = bind(ctx))
        return rc;
    if(int rc = join_uploads(ctx))
        return rc;
    if(ctx->copy_stream)
        LFI_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));
    return LFI_OK;
}

// ---- YUV 4:2:0 surfaces and input (yuv_surfaces.hpp, yuv420_upload.hpp) ----------------------------------------------------------------

namespace {

// rows · pitch, SIZE_MAX where that overflows
size_t plane_bytes(size_t rows, size_t pitch)
{
    return pitch > SIZE_MAX / rows ? SIZE_MAX : rows * pitch;
}

// a + b, SIZE_MAX where that overflows
size_t add_sat(size_t a, size_t b)
{
    return a > SIZE_MAX - b ? SIZE_MAX : a + b;
}

// the layout of a surface format (LFI_YUV_I420 or LFI_YUV_NV12: the format without its depth flag) and its bytes per sample
int yuv_layout(int format)
{
    return format & ~(LFI_YUV_10BIT | LFI_YUV_DEEP);
}

uint32_t yuv_bps(int format)
{
    return format & LFI_YUV_10BIT ? 2u : 1u;
}

bool yuv_format_known(int format)
{
    return format == LFI_YUV_I420 || format == LFI_YUV_NV12 || format == LFI_YUV_I010 || format == LFI_YUV_P010 || format == (LFI_YUV_I010 | LFI_YUV_DEEP) ||
           format == (LFI_YUV_P010 | LFI_YUV_DEEP) || format == LFI_YUV_GBRP10;
}

// the formats made from the deep planes (deep_yuv.hpp): frames that only lfi_download_views_yuv writes
bool yuv_format_deep(int format)
{
    return yuv_format_known(format) && (format & LFI_YUV_DEEP);
}

const char *const kDeepFormatRefused = "LFI_YUV_DEEP formats (LFI_YUV_I010 | LFI_YUV_DEEP, LFI_YUV_P010 | LFI_YUV_DEEP, LFI_YUV_GBRP10) are frames made from the deep "
                                       "views: only lfi_download_views_yuv writes them";

// why s does not describe n frames of width × height (NULL: it does); *extent: the end of a frame's last plane
// deep: what the caller makes of the LFI_YUV_DEEP formats.  DEEP_REFUSED: it refuses them by name (every call but the next two).  DEEP_LAYOUT
// (lfi_yuv_surfaces_check): LFI_YUV_GBRP10, a layout of its own, is known; LFI_YUV_DEEP on I010 / P010 says where the samples COME FROM, not
// where they lie, and stays an unknown format for a call that knows no source.  DEEP_SOURCE (lfi_download_views_yuv): all three.
// LFI_YUV_GBRP10: three full-size planes G, B, R where I010 has Y, Cb, Cr
enum DeepFormats { DEEP_REFUSED, DEEP_LAYOUT, DEEP_SOURCE };
const char *yuv_surfaces_fault(const lfi_yuv_surfaces *s, int width, int height, int n, size_t *extent, DeepFormats deep = DEEP_REFUSED)
{
    if(!s || !s->base)
        return "the descriptor or its base is NULL";
    if(deep == DEEP_REFUSED && yuv_format_deep(s->format))
        return kDeepFormatRefused;
    if(deep == DEEP_LAYOUT && yuv_format_deep(s->format) && s->format != LFI_YUV_GBRP10)
        return "unknown format: LFI_YUV_DEEP on LFI_YUV_I010 / LFI_YUV_P010 is a source flag for lfi_download_views_yuv, the layout is the format without it";
    if(!yuv_format_known(s->format) || (s->memory != LFI_MEM_HOST && s->memory != LFI_MEM_DEVICE))
        return "unknown format (LFI_YUV_I420, LFI_YUV_NV12, LFI_YUV_I010, LFI_YUV_P010, the latter two | LFI_YUV_DEEP, LFI_YUV_GBRP10) or memory (LFI_MEM_HOST, LFI_MEM_DEVICE)";
    if(width < 1 || height < 1 || n < 1)
        return "width, height and n must be at least 1";
    const bool full = s->format == LFI_YUV_GBRP10; // no subsampling: the second and third plane are as large as the first
    const size_t W = (size_t)width, H = (size_t)height, cw = full ? W : (W + 1) >> 1, ch = full ? H : (H + 1) >> 1;
    const bool nv12 = yuv_layout(s->format) == LFI_YUV_NV12;
    const size_t bps = yuv_bps(s->format);
    if(s->y_pitch < bps * W || s->c_pitch < bps * (nv12 ? 2 * cw : cw))
        return bps == 1 ? "a pitch is below its minimum (y_pitch >= W; c_pitch >= cw for I420, 2*cw for NV12)"
                        : "a pitch is below its minimum (y_pitch >= 2*W; c_pitch >= 2*cw for I010, 4*cw for P010)";
    if(bps == 2 && (reinterpret_cast<uintptr_t>(s->base) | s->y_pitch | s->c_pitch | s->c_offset | s->cr_offset | s->frame_stride) % 2)
        return "alignment: 16-bit samples need an even base, even pitches and offsets and an even frame_stride";
    const size_t y_end = plane_bytes(H, s->y_pitch), c_bytes = plane_bytes(ch, s->c_pitch);
    if(s->c_offset < y_end)
        return "the planes overlap or are out of order: c_offset is below H * y_pitch";
    size_t end = add_sat(s->c_offset, c_bytes);
    if(nv12)
    {
        if(s->cr_offset != 0)
            return "cr_offset must be 0 with NV12";
    }
    else
    {
        if(s->cr_offset < end)
            return "the planes overlap or are out of order: cr_offset is below c_offset + ch * c_pitch";
        end = add_sat(s->cr_offset, c_bytes);
    }
    if(end == SIZE_MAX)
        return "the frame's extent does not fit size_t";
    if(n > 1 && (s->frame_stride < end || s->frame_stride > (SIZE_MAX - end) / (size_t)(n - 1)))
        return "frame_stride is below the frame's extent (the end of its last plane)";
    if(extent)
        *extent = end;
    return nullptr;
}

// the staged frames of a chunk as surfaces: the padded planes of yuv_geometry; NV12's chroma rows are y_pitch bytes (2·c_pitch)
lfi::YuvSurfaces staged_surfaces(const lfi::YuvGeometry &g, int format, uint8_t *dev)
{
    lfi::YuvSurfaces s{};
    const size_t y_plane = (size_t)g.y_pitch * g.y_rows;
    s.base = dev;
    s.frame_stride = g.dev_frame_bytes;
    s.y_pitch = g.y_pitch;
    s.c_offset = y_plane;
    s.c_pitch = yuv_layout(format) == LFI_YUV_NV12 ? g.y_pitch : g.c_pitch;
    s.cr_offset = yuv_layout(format) == LFI_YUV_NV12 ? 0 : y_plane + (size_t)g.c_pitch * g.ch;
    return s;
}

// device surfaces a kernel may address directly: every load and word store of yuv_surfaces.hpp is then aligned and inside its row
bool yuv_surfaces_in_place(const lfi_yuv_surfaces &s)
{
    return s.memory == LFI_MEM_DEVICE && (reinterpret_cast<uintptr_t>(s.base) | s.frame_stride | s.y_pitch | s.c_offset | s.c_pitch | s.cr_offset) % 16 == 0 &&
           s.y_pitch <= UINT32_MAX && s.c_pitch <= UINT32_MAX;
}

lfi::YuvSurfaces caller_surfaces(const lfi_yuv_surfaces &s)
{
    lfi::YuvSurfaces k{};
    k.base = static_cast<uint8_t *>(s.base);
    k.frame_stride = s.frame_stride, k.c_offset = s.c_offset, k.cr_offset = s.cr_offset;
    k.y_pitch = (uint32_t)s.y_pitch, k.c_pitch = (uint32_t)s.c_pitch;
    return k;
}

// the staged frame IS the caller's frame: one copy moves it (W a multiple of 8, H even, the tight layout)
bool yuv_surfaces_like_staged(const lfi_yuv_surfaces &s, const lfi::YuvGeometry &g)
{
    const lfi::YuvSurfaces t = staged_surfaces(g, s.format, nullptr);
    return g.tight && s.y_pitch == t.y_pitch && s.c_pitch == t.c_pitch && s.c_offset == t.c_offset && s.cr_offset == t.cr_offset;
}

// LFI_MEM_DEVICE: base must be device memory of the context's own device, in an allocation that covers the n frames
int check_device_surfaces(lfi_ctx *ctx, const char *who, const lfi_yuv_surfaces &s, size_t extent, int n)
{
    hipPointerAttribute_t attr{};
    if(hipPointerGetAttributes(&attr, s.base) != hipSuccess)
    {
        (void)hipGetLastError(); // a pointer the runtime does not know: not an error of the context's
        return fail(ctx, LFI_EINVAL, std::string(who) + ": LFI_MEM_DEVICE needs a pointer to device memory, the runtime does not know this one");
    }
    if(attr.type != hipMemoryTypeDevice || attr.device != ctx->device)
        return fail(ctx, LFI_EINVAL, std::string(who) + ": LFI_MEM_DEVICE needs a pointer to device memory of the context's own device");
    hipDeviceptr_t a_base = nullptr;
    size_t a_bytes = 0;
    if(hipMemGetAddressRange(&a_base, &a_bytes, s.base) != hipSuccess)
    {
        (void)hipGetLastError();
        return fail(ctx, LFI_EINVAL, std::string(who) + ": LFI_MEM_DEVICE needs a pointer into a device allocation");
    }
    const size_t before = (size_t)(static_cast<const uint8_t *>(s.base) - static_cast<const uint8_t *>(a_base));
    if(before > a_bytes || s.frame_stride * (size_t)(n - 1) + extent > a_bytes - before)
        return fail(ctx, LFI_EINVAL, std::string(who) + ": the device allocation ends before the last frame does");
    return LFI_OK;
}

// host frames whose rows are tight but which are not the staged frame (W no multiple of 8 or H odd): a 2D copy between the two moves row by
// row; such a frame can go through a packed device copy of its planes instead (enqueue_surface_copies' pack)
bool yuv_surfaces_packable(const lfi_yuv_surfaces &s, const lfi::YuvGeometry &g)
{
    return s.memory == LFI_MEM_HOST && !yuv_surfaces_like_staged(s, g) && s.y_pitch == (size_t)g.W * g.bps &&
           s.c_pitch == (yuv_layout(s.format) == LFI_YUV_NV12 ? 2 * (size_t)g.cw : g.cw) * g.bps;
}

// the frames' own bytes between n caller frames (from frame k0 on) and n staged ones at dev, on st; to_staged: caller → staged.
// pack (staged → caller only; NULL: none): device memory for one tight frame (g.frame_bytes), given only where the caller has found
// yuv_surfaces_packable(s, g): each plane is first packed on the device (one device-to-device 2D copy) and then leaves as ONE contiguous
// copy instead of a copy per row
hipError_t enqueue_surface_copies(hipStream_t st, const lfi_yuv_surfaces &s, int k0, int n, const lfi::YuvGeometry &g, uint8_t *dev, bool to_staged,
                                  uint8_t *pack = nullptr)
{
    const hipMemcpyKind kind = s.memory == LFI_MEM_DEVICE ? hipMemcpyDeviceToDevice : to_staged ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    const lfi::YuvSurfaces t = staged_surfaces(g, s.format, dev);
    uint8_t *base = static_cast<uint8_t *>(s.base) + s.frame_stride * (size_t)k0;
    const bool nv12 = yuv_layout(s.format) == LFI_YUV_NV12;
    if(yuv_surfaces_like_staged(s, g))
    {
        if(s.frame_stride == g.frame_bytes || n == 1)
            return to_staged ? hipMemcpyAsync(dev, base, g.frame_bytes * n, kind, st) : hipMemcpyAsync(base, dev, g.frame_bytes * n, kind, st);
        return to_staged ? hipMemcpy2DAsync(dev, g.frame_bytes, base, s.frame_stride, g.frame_bytes, n, kind, st)
                         : hipMemcpy2DAsync(base, s.frame_stride, dev, g.frame_bytes, g.frame_bytes, n, kind, st);
    }
    for(int k = 0; k < n; k++)
    {
        uint8_t *f = base + s.frame_stride * (size_t)k, *d = dev + t.frame_stride * (size_t)k;
        // plane, caller's pitch, staged pitch, bytes per row, rows
        const struct
        {
            size_t f_off, d_off, f_pitch, d_pitch, width, rows;
        } planes[3] = {{0, 0, s.y_pitch, t.y_pitch, (size_t)g.W * g.bps, g.H},
                       {s.c_offset, t.c_offset, s.c_pitch, t.c_pitch, (nv12 ? 2 * (size_t)g.cw : g.cw) * g.bps, g.ch},
                       {s.cr_offset, t.cr_offset, s.c_pitch, t.c_pitch, (size_t)g.cw * g.bps, g.ch}};
        size_t packed = 0; // the plane's offset in the packed frame
        for(int p = 0; p < (nv12 ? 2 : 3); p++)
        {
            const auto &pl = planes[p];
            if(pack && !to_staged)
            {
                hipError_t e = hipMemcpy2DAsync(pack + packed, pl.width, d + pl.d_off, pl.d_pitch, pl.width, pl.rows, hipMemcpyDeviceToDevice, st);
                if(e == hipSuccess)
                    e = hipMemcpyAsync(f + pl.f_off, pack + packed, pl.width * pl.rows, hipMemcpyDeviceToHost, st);
                if(e != hipSuccess)
                    return e;
                packed += pl.width * pl.rows;
                continue;
            }
            const hipError_t e = to_staged ? hipMemcpy2DAsync(d + pl.d_off, pl.d_pitch, f + pl.f_off, pl.f_pitch, pl.width, pl.rows, kind, st)
                                           : hipMemcpy2DAsync(f + pl.f_off, pl.f_pitch, d + pl.d_off, pl.d_pitch, pl.width, pl.rows, kind, st);
            if(e != hipSuccess)
                return e;
        }
    }
    return hipSuccess;
}

// the tight I420 host frames of the *_yuv420 calls, frame_stride_bytes apart, as surfaces; refuses what those calls refuse of them
int host_i420_surfaces(lfi_ctx *ctx, const char *who, const uint8_t *frames, size_t frame_stride_bytes, lfi_yuv_surfaces *s)
{
    if(!frames || frame_stride_bytes < lfi::yuv_geometry(ctx->width, ctx->height).frame_bytes)
        return fail(ctx, LFI_EINVAL, std::string(who) + ": the frames' pointer is NULL or frame_stride_bytes is below W*H + 2*((W+1)/2)*((H+1)/2)");
    lfi_yuv_surfaces_packed(LFI_YUV_I420, LFI_MEM_HOST, const_cast<uint8_t *>(frames), ctx->width, ctx->height, s);
    s->frame_stride = frame_stride_bytes;
    return LFI_OK;
}

// what lfi_upload_images_yuv420, lfi_upload_images_yuv and lfi_upload_images_yuv_derived refuse alike, before they look at the frames.
// derived: the call writes the planar copy of a context whose RGBA inputs were released, and is refused where the others are served
int check_yuv_upload(lfi_ctx *ctx, const char *who, int g0, int n, int matrix, int range, int chroma, bool derived = false)
{
    const char *fault = nullptr;
    if(derived && !ctx->inputs_released)
    {
        if(!ctx->grid)
            return fail(ctx, LFI_EINVAL, "lfi_set_grid has not been called");
        fault = ": the context still holds its RGBA inputs: the call writes the planar copy alone, which is valid only after lfi_release_inputs";
    }
    else if(derived && (!ctx->planar || (int)ctx->planar_phase.size() != ctx->n))
        fault = ": the context holds no planar copy of the inputs";
    else if(!derived && ctx->inputs_released)
        fault = ": the RGBA inputs were released (lfi_release_inputs): lfi_set_grid and upload the images again";
    else if(!derived && !ctx->grid)
        return fail(ctx, LFI_EINVAL, "lfi_set_grid has not been called");
    else if(ctx->windowed)
        fault = ": YUV 4:2:0 frames need whole images: a 2x2 chroma block may straddle the row window's band";
    else if(n < 1 || g0 < 0 || (long)g0 + n > ctx->n)
        fault = ": needs n >= 1 images starting at g0 inside [0, N)";
    else if((matrix != LFI_YUV_BT709 && matrix != LFI_YUV_BT601) || (range != LFI_YUV_LIMITED && range != LFI_YUV_FULL) ||
            (chroma != LFI_CHROMA_BILINEAR && chroma != LFI_CHROMA_NEAREST))
        fault = ": unknown YUV matrix (LFI_YUV_BT709, LFI_YUV_BT601), range (LFI_YUV_LIMITED, LFI_YUV_FULL) or chroma "
                "filter (LFI_CHROMA_BILINEAR, LFI_CHROMA_NEAREST)";
    return fault ? fail(ctx, LFI_EINVAL, std::string(who) + fault) : LFI_OK;
}

// Behind the three upload calls.  The arguments have passed check_yuv_upload; src is what host_i420_surfaces made, or has passed
// yuv_surfaces_fault, which gave extent.  derived: the frames go into the planar copy (yuvs_derived_expand), which stays the valid copy it
// was — no version moves; else into the RGBA planes (yuvs_expand), and the copy is rebuilt from them by the next render that reads it
int upload_yuv_surfaces(lfi_ctx *ctx, const char *who, int g0, int n, int matrix, int range, int chroma, const lfi_yuv_surfaces &src, size_t extent,
                        bool derived = false)
{
    if(int rc = bind(ctx))
        return rc;
    if(src.memory == LFI_MEM_DEVICE)
        if(int rc = check_device_surfaces(ctx, who, src, extent, n))
            return rc;
    if(int rc = ensure_copy_stream(ctx))
        return rc;
    const bool deep = yuv_bps(src.format) == 2; // I010 / P010: yuv10.hpp (never with derived: lfi_upload_images_yuv_derived refuses them)
    const lfi::YuvGeometry g = lfi::yuv_geometry(ctx->width, ctx->height, yuv_bps(src.format));
    const bool in_place = yuv_surfaces_in_place(src);
    const bool left = ctx->yuv_in_siting == LFI_YUV_SITING_LEFT; // lfi_set_yuv_siting
    // staged: chunks of at most 16 frames or 256 MiB, at least one frame: a chunk's copies and its launch follow each other on the copy
    // stream, so stream order is all the staging buffer needs.  In place: one chunk of all n frames, no buffer
    const int chunk = in_place ? n : (int)std::max<size_t>(1, std::min<size_t>(16, ((size_t)256 << 20) / g.dev_frame_bytes));
    const size_t need = in_place ? 0 : g.dev_frame_bytes * std::min(chunk, n);
    if(ctx->yuv_in.bytes() < need)
    {
        LFI_HIP(ctx, hipStreamSynchronize(ctx->copy_stream)); // an earlier call's chunks may still be in the buffer that goes
        LFI_HIP(ctx, ctx->yuv_in.reserve(need));
    }
    if(!ctx->uploads_pending)
    {
        // first copy of a batch: renders already enqueued on the compute stream may still read the planes
        LFI_HIP(ctx, hipEventRecord(ctx->ev_order, ctx->stream));
        LFI_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_order, 0));
    }
    ctx->uploads_pending = true; // from here on something may be enqueued on the copy stream
    hipStream_t st = ctx->copy_stream;
    for(int k0 = 0; k0 < n; k0 += chunk)
    {
        const int nk = std::min(chunk, n - k0);
        // the frames' own bytes only: the staged planes' padding stays whatever it was, the kernel uses none of it
        if(!in_place)
            LFI_HIP(ctx, enqueue_surface_copies(st, src, k0, nk, g, ctx->yuv_in.get(), true));
        lfi::YuvsInArgs a{};
        a.s = in_place ? caller_surfaces(src) : staged_surfaces(g, src.format, ctx->yuv_in.get());
        a.W = g.W, a.H = g.H, a.cw = g.cw, a.ch = g.ch;
        a.blocks_x = (g.W + lfi::YUV_BLOCK_W - 1) / lfi::YUV_BLOCK_W;
        a.k = deep ? lfi::YUV10_IN_COEFFS[matrix * 2 + range] : lfi::YUV_IN_COEFFS[matrix * 2 + range];
        if(derived)
        {
            // whole images (check_yuv_upload refuses a row window): the copy's planes hold in_rows = H rows of planar_pitch bytes
            lfi::YuvsDerivedArgs d{};
            d.in = a;
            d.planar = ctx->planar.get();
            d.phase = ctx->d_planar_phase.as<int32_t>();
            d.pitch = (uint32_t)ctx->planar_pitch, d.padx = (uint32_t)ctx->planar_padx;
            d.g0 = (uint32_t)(g0 + k0);
            LFI_HIP(ctx, lfi::launch_yuvs_derived_expand(st, src.format, chroma == LFI_CHROMA_NEAREST, left, d, nk));
            continue;
        }
        a.dst = ctx->grid.get() + in_plane_bytes(ctx) * (size_t)(g0 + k0);
        a.image_stride = in_plane_bytes(ctx);
        a.rows16 = g.W % 4 == 0; // the grid starts on a 16-byte boundary (hipMalloc; lfi_attach_grid checks), an image is W·H·4 bytes
        if(deep)
            LFI_HIP(ctx, lfi::launch_yuvs_expand10(st, yuv_layout(src.format), chroma == LFI_CHROMA_NEAREST, left, a, nk));
        else
            LFI_HIP(ctx, lfi::launch_yuvs_expand(st, src.format, chroma == LFI_CHROMA_NEAREST, left, a, nk));
    }
    if(!derived)
        touch_images(ctx, g0, g0 + n);
    return LFI_OK;
}

} // namespace

int lfi_yuv_surfaces_check(const lfi_yuv_surfaces *s, int width, int height, int n)
{
    return yuv_surfaces_fault(s, width, height, n, nullptr, DEEP_LAYOUT) ? LFI_EINVAL : LFI_OK;
}

int lfi_yuv_surfaces_packed(int format, int memory, void *base, int width, int height, lfi_yuv_surfaces *out)
{
    // (LFI_YUV_DEEP on I010 / P010 is a source flag, not a layout: pack the format without it)
    if(!yuv_format_known(format) || (yuv_format_deep(format) && format != LFI_YUV_GBRP10) || (memory != LFI_MEM_HOST && memory != LFI_MEM_DEVICE) || width < 1 ||
       height < 1 || !out)
        return LFI_EINVAL;
    const lfi::YuvGeometry g = lfi::yuv_geometry(width, height, yuv_bps(format));
    const bool nv12 = yuv_layout(format) == LFI_YUV_NV12;
    out->format = format, out->memory = memory;
    out->base = base;
    if(format == LFI_YUV_GBRP10) // G, B, R: three planes of H rows of 2·W bytes
    {
        const size_t plane = (size_t)g.W * g.H * 2;
        out->frame_stride = 3 * plane;
        out->y_pitch = out->c_pitch = (size_t)g.W * 2;
        out->c_offset = plane, out->cr_offset = 2 * plane;
        return LFI_OK;
    }
    out->frame_stride = g.frame_bytes;
    out->y_pitch = (size_t)g.W * g.bps;
    out->c_offset = (size_t)g.W * g.H * g.bps;
    out->c_pitch = (nv12 ? 2 * (size_t)g.cw : g.cw) * g.bps;
    out->cr_offset = nv12 ? 0 : out->c_offset + (size_t)g.cw * g.ch * g.bps;
    return LFI_OK;
}

int lfi_upload_images_yuv420(lfi_ctx *ctx, int g0, int n, int matrix, int range, int chroma, const uint8_t *frames, size_t frame_stride_bytes)
{
    if(!ctx)
        return LFI_EINVAL;
    if(int rc = check_yuv_upload(ctx, "lfi_upload_images_yuv420", g0, n, matrix, range, chroma))
        return rc;
    lfi_yuv_surfaces src{};
    if(int rc = host_i420_surfaces(ctx, "lfi_upload_images_yuv420", frames, frame_stride_bytes, &src))
        return rc;
    return upload_yuv_surfaces(ctx, "lfi_upload_images_yuv420", g0, n, matrix, range, chroma, src, 0);
}

int lfi_upload_images_yuv(lfi_ctx *ctx, int g0, int n, int matrix, int range, int chroma, const lfi_yuv_surfaces *src)
{
    if(!ctx)
        return LFI_EINVAL;
    if(int rc = check_yuv_upload(ctx, "lfi_upload_images_yuv", g0, n, matrix, range, chroma))
        return rc;
    size_t extent = 0;
    if(const char *fault = yuv_surfaces_fault(src, ctx->width, ctx->height, n, &extent))
        return fail(ctx, LFI_EINVAL, std::string("lfi_upload_images_yuv: ") + fault);
    return upload_yuv_surfaces(ctx, "lfi_upload_images_yuv", g0, n, matrix, range, chroma, *src, extent);
}

int lfi_upload_images_yuv_derived(lfi_ctx *ctx, int g0, int n, int matrix, int range, int chroma, const lfi_yuv_surfaces *src)
{
    if(!ctx)
        return LFI_EINVAL;
    if(int rc = check_yuv_upload(ctx, "lfi_upload_images_yuv_derived", g0, n, matrix, range, chroma, true))
        return rc;
    size_t extent = 0;
    if(const char *fault = yuv_surfaces_fault(src, ctx->width, ctx->height, n, &extent))
        return fail(ctx, LFI_EINVAL, std::string("lfi_upload_images_yuv_derived: ") + fault);
    if(src->format & LFI_YUV_10BIT)
        return fail(ctx, LFI_EINVAL, "lfi_upload_images_yuv_derived: 10-bit frames (LFI_YUV_I010, LFI_YUV_P010) into the planar copy are not supported: "
                                     "upload them with lfi_upload_images_yuv before lfi_release_inputs");
    return upload_yuv_surfaces(ctx, "lfi_upload_images_yuv_derived", g0, n, matrix, range, chroma, *src, extent, true);
}

// ---- mosaic input: one frame that holds the grid (yuv_mosaic.hpp) -------------------------------------------------------------------------

namespace {

// why m does not map onto images [g0, g0 + n) of a cols × rows grid (NULL: it does): the rules of lfi_mosaic_map
const char *mosaic_fault(const lfi_mosaic *m, int cols, int rows, int g0)
{
    if(!m)
        return "the mosaic is NULL";
    if(m->tiles_x < 1 || m->tiles_y < 1 || cols < 1 || rows < 1)
        return "tiles_x, tiles_y and the grid's columns and rows must be at least 1";
    if(m->order != LFI_MOSAIC_ROWS && m->order != LFI_MOSAIC_GRID)
        return "unknown order (LFI_MOSAIC_ROWS, LFI_MOSAIC_GRID)";
    if(m->flags & ~(uint32_t)LFI_MOSAIC_BOTTOM_UP)
        return "unknown flags (LFI_MOSAIC_BOTTOM_UP)";
    const long long tiles = (long long)m->tiles_x * m->tiles_y, images = (long long)cols * rows;
    if(m->n < 1 || m->first_tile < 0 || (long long)m->first_tile + m->n > tiles)
        return "needs n >= 1 tiles starting at first_tile inside [0, tiles_x * tiles_y)";
    if(g0 < 0 || (long long)g0 + m->n > images)
        return "needs the n images starting at g0 inside [0, N)";
    if(m->order == LFI_MOSAIC_GRID && (m->tiles_x != cols || m->tiles_y != rows || m->first_tile != 0 || m->n != images || g0 != 0))
        return "LFI_MOSAIC_GRID needs tiles_x == cols, tiles_y == rows, first_tile == 0, n == cols * rows and g0 == 0";
    return nullptr;
}

lfi::MosaicMap mosaic_map_of(const lfi_mosaic &m, int rows, int g0)
{
    lfi::MosaicMap k{};
    k.tiles_x = (uint32_t)m.tiles_x, k.tiles_y = (uint32_t)m.tiles_y, k.first_tile = (uint32_t)m.first_tile;
    k.grid = m.order == LFI_MOSAIC_GRID, k.bottom_up = (m.flags & LFI_MOSAIC_BOTTOM_UP) != 0;
    k.rows = (uint32_t)rows, k.g0 = (uint32_t)g0;
    return k;
}

// The staged route's plan: chunk c of a mosaic that has passed mosaic_fault.  A chunk is whole tile rows, as many as fit the cap (at least
// one): tile rows [r0, r0 + nr) in ROWS order, which are the frame's tile rows [ty0, ty0 + nr) (BOTTOM_UP: counted from the other end), and
// of the call's tiles those that lie in them, [k0, k0 + nk).  false: there is no chunk c
struct MosaicChunk
{
    int r0, nr, ty0, k0, nk;
};

bool mosaic_chunk(const lfi_mosaic &m, size_t tile_row_bytes, size_t cap_bytes, int c, MosaicChunk *out)
{
    const long long r_first = m.first_tile / m.tiles_x, r_last = ((long long)m.first_tile + m.n - 1) / m.tiles_x;
    const long long per = std::max<long long>(1, std::min<long long>(r_last - r_first + 1, (long long)(cap_bytes / tile_row_bytes)));
    const long long r0 = r_first + (long long)c * per;
    if(c < 0 || r0 > r_last)
        return false;
    const long long nr = std::min(per, r_last - r0 + 1);
    const long long t_lo = std::max<long long>(m.first_tile, r0 * m.tiles_x), t_hi = std::min<long long>((long long)m.first_tile + m.n, (r0 + nr) * m.tiles_x);
    out->r0 = (int)r0, out->nr = (int)nr;
    out->ty0 = (int)(m.flags & LFI_MOSAIC_BOTTOM_UP ? m.tiles_y - (r0 + nr) : r0);
    out->k0 = (int)(t_lo - m.first_tile), out->nk = (int)(t_hi - t_lo);
    return true;
}

constexpr size_t MOSAIC_CHUNK_CAP = (size_t)256 << 20; // the cap of the YUV uploads' staging chunks

// the staged bytes of one tile row of a frame MW wide: yuv_geometry's padded planes of MW × H
size_t mosaic_tile_row_bytes(int MW, int H)
{
    return lfi::yuv_geometry(MW, H).dev_frame_bytes;
}

} // namespace

int lfi_mosaic_map(const lfi_mosaic *m, int cols, int rows, int g0, int k, int *tx, int *ty, int *g)
{
    if(mosaic_fault(m, cols, rows, g0) || k < 0 || k >= m->n)
        return LFI_EINVAL;
    uint32_t x, y, image;
    lfi::mosaic_tile(mosaic_map_of(*m, rows, g0), (uint32_t)k, x, y, image);
    if(tx)
        *tx = (int)x;
    if(ty)
        *ty = (int)y;
    if(g)
        *g = (int)image;
    return LFI_OK;
}

int lfi_debug_mosaic_chunk(const lfi_mosaic *m, int tile_w, int tile_h, size_t cap_bytes, int chunk, int32_t *out5)
{
    if(!m || !out5 || tile_w < 2 || tile_h < 2 || tile_w % 2 || tile_h % 2 || m->tiles_x < 1 || (long long)m->tiles_x * tile_w > INT32_MAX)
        return LFI_EINVAL;
    // the natural grid of the order: GRID its own, ROWS one row of all tiles
    const bool grid = m->order == LFI_MOSAIC_GRID;
    if(mosaic_fault(m, grid ? m->tiles_x : m->n, grid ? m->tiles_y : 1, 0))
        return LFI_EINVAL;
    MosaicChunk c{};
    if(!mosaic_chunk(*m, mosaic_tile_row_bytes(m->tiles_x * tile_w, tile_h), cap_bytes ? cap_bytes : MOSAIC_CHUNK_CAP, chunk, &c))
        return LFI_EINVAL;
    out5[0] = c.r0, out5[1] = c.nr, out5[2] = c.ty0, out5[3] = c.k0, out5[4] = c.nk;
    return LFI_OK;
}

namespace {

// Behind the two mosaic YUV calls, as upload_yuv_surfaces is behind the frame calls: every check, the staging buffer, the ordering preamble
// and the routing.  derived: the tiles go into the planar copy (yuvs_mosaic_derived_expand), which stays the valid copy it was — no version
// moves; else into the RGBA planes (yuvs_mosaic_expand), and the copy is rebuilt from them by the next render that reads it
int upload_mosaic_yuv_surfaces(lfi_ctx *ctx, const char *who, const lfi_mosaic *m, int g0, int matrix, int range, int chroma, const lfi_yuv_surfaces *src,
                               bool derived)
{
    if(!ctx)
        return LFI_EINVAL;
    if(!m)
        return fail(ctx, LFI_EINVAL, std::string(who) + ": the mosaic is NULL");
    if(int rc = check_yuv_upload(ctx, who, g0, m->n, matrix, range, chroma, derived))
        return rc;
    if(const char *fault = mosaic_fault(m, ctx->cols, ctx->rows, g0))
        return fail(ctx, LFI_EINVAL, std::string(who) + ": " + fault);
    const int W = ctx->width, H = ctx->height;
    if(W % 2 || H % 2)
        return fail(ctx, LFI_EINVAL, std::string(who) + ": a YUV 4:2:0 mosaic needs an even image width and height: an odd size puts a 2x2 chroma block across two tiles");
    if((long long)m->tiles_x * W > INT32_MAX || (long long)m->tiles_y * H > INT32_MAX)
        return fail(ctx, LFI_EINVAL, std::string(who) + ": the frame's size tiles_x * W by tiles_y * H does not fit 31 bits");
    const int MW = m->tiles_x * W, MH = m->tiles_y * H;
    if(src && yuv_format_deep(src->format))
        return fail(ctx, LFI_EINVAL, std::string(who) + ": " + kDeepFormatRefused);
    if(src && yuv_format_known(src->format) && (src->format & LFI_YUV_10BIT))
        return fail(ctx, LFI_EINVAL, std::string(who) + ": 10-bit mosaics (LFI_YUV_I010, LFI_YUV_P010) are not supported: the frame must be LFI_YUV_I420 or LFI_YUV_NV12");
    size_t extent = 0;
    if(const char *fault = yuv_surfaces_fault(src, MW, MH, 1, &extent))
        return fail(ctx, LFI_EINVAL, std::string(who) + ": " + fault + " (the frame is tiles_x * W by tiles_y * H)");
    if(int rc = bind(ctx))
        return rc;
    if(src->memory == LFI_MEM_DEVICE)
        if(int rc = check_device_surfaces(ctx, who, *src, extent, 1))
            return rc;
    if(int rc = ensure_copy_stream(ctx))
        return rc;
    lfi_yuv_surfaces one = *src;
    one.frame_stride = 0; // one frame: its stride addresses nothing and need not be aligned
    const bool in_place = yuv_surfaces_in_place(one);
    const bool nv12 = src->format == LFI_YUV_NV12;
    const size_t tile_row_bytes = mosaic_tile_row_bytes(MW, H);
    const size_t cap = ctx->mosaic_chunk_cap ? ctx->mosaic_chunk_cap : MOSAIC_CHUNK_CAP; // lfi_debug_set_mosaic_chunk_cap
    MosaicChunk c{};
    (void)mosaic_chunk(*m, tile_row_bytes, cap, 0, &c); // chunk 0 exists and is the largest
    const size_t need = in_place ? 0 : lfi::yuv_geometry(MW, c.nr * H).dev_frame_bytes;
    if(ctx->yuv_in.bytes() < need)
    {
        LFI_HIP(ctx, hipStreamSynchronize(ctx->copy_stream)); // an earlier call's chunks may still be in the buffer that goes
        LFI_HIP(ctx, ctx->yuv_in.reserve(need));
    }
    if(!ctx->uploads_pending)
    {
        // first copy of a batch: renders already enqueued on the compute stream may still read the planes
        LFI_HIP(ctx, hipEventRecord(ctx->ev_order, ctx->stream));
        LFI_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_order, 0));
    }
    ctx->uploads_pending = true;
    hipStream_t st = ctx->copy_stream;
    lfi::YuvsMosaicArgs a{};
    a.in.W = (uint32_t)W, a.in.H = (uint32_t)H, a.in.cw = (uint32_t)W / 2, a.in.ch = (uint32_t)H / 2;
    a.in.blocks_x = ((uint32_t)W + lfi::YUV_BLOCK_W - 1) / lfi::YUV_BLOCK_W;
    a.in.k = lfi::YUV_IN_COEFFS[matrix * 2 + range];
    if(!derived)
    {
        a.in.dst = ctx->grid.get();
        a.in.image_stride = in_plane_bytes(ctx);
        a.in.rows16 = W % 4 == 0;
    }
    a.map = mosaic_map_of(*m, ctx->rows, g0);
    const bool nearest = chroma == LFI_CHROMA_NEAREST, left = ctx->yuv_in_siting == LFI_YUV_SITING_LEFT, unaligned = W % lfi::YUV_BLOCK_W != 0;
    // the ONE launch for the nk tiles from a.k0 on, from the surfaces a.in.s
    auto launch = [&](int nk) -> hipError_t {
        if(!derived)
            return lfi::launch_yuvs_mosaic_expand(st, src->format, nearest, left, unaligned, a, nk);
        // whole images (check_yuv_upload refuses a row window): the copy's planes hold in_rows = H rows of planar_pitch bytes
        lfi::YuvsMosaicDerivedArgs d{};
        d.d.in = a.in;
        d.d.planar = ctx->planar.get();
        d.d.phase = ctx->d_planar_phase.as<int32_t>();
        d.d.pitch = (uint32_t)ctx->planar_pitch, d.d.padx = (uint32_t)ctx->planar_padx;
        d.map = a.map, d.k0 = a.k0, d.ty_bias = a.ty_bias;
        return lfi::launch_yuvs_mosaic_derived_expand(st, src->format, nearest, left, unaligned, d, nk);
    };
    if(in_place)
    {
        // the frame is read where it lies: ONE launch for all n tiles
        a.in.s = caller_surfaces(*src);
        LFI_HIP(ctx, launch(m->n));
    }
    else
    {
        // staged: chunks of whole tile rows, each ONE 2D copy per plane of the rows' own bytes and one launch; copies and launch follow each
        // other on the copy stream, so stream order is all the staging buffer needs
        const hipMemcpyKind kind = src->memory == LFI_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        const uint8_t *base = static_cast<const uint8_t *>(src->base);
        for(int i = 0; mosaic_chunk(*m, tile_row_bytes, cap, i, &c); i++)
        {
            const lfi::YuvGeometry g = lfi::yuv_geometry(MW, c.nr * H);
            const lfi::YuvSurfaces t = staged_surfaces(g, src->format, ctx->yuv_in.get());
            const size_t y0 = (size_t)c.ty0 * H, c0 = y0 / 2;
            LFI_HIP(ctx, hipMemcpy2DAsync(t.base, t.y_pitch, base + y0 * src->y_pitch, src->y_pitch, (size_t)MW, g.H, kind, st));
            LFI_HIP(ctx, hipMemcpy2DAsync(t.base + t.c_offset, t.c_pitch, base + src->c_offset + c0 * src->c_pitch, src->c_pitch,
                                          nv12 ? (size_t)MW : (size_t)MW / 2, g.ch, kind, st));
            if(!nv12)
                LFI_HIP(ctx, hipMemcpy2DAsync(t.base + t.cr_offset, t.c_pitch, base + src->cr_offset + c0 * src->c_pitch, src->c_pitch, (size_t)MW / 2, g.ch, kind, st));
            a.in.s = t;
            a.k0 = (uint32_t)c.k0, a.ty_bias = (uint32_t)c.ty0;
            LFI_HIP(ctx, launch(c.nk));
        }
    }
    // the images the tiles became: a contiguous range under ROWS, the whole grid under GRID
    if(!derived)
        touch_images(ctx, g0, g0 + m->n);
    return LFI_OK;
}

} // namespace

int lfi_upload_mosaic_yuv(lfi_ctx *ctx, const lfi_mosaic *m, int g0, int matrix, int range, int chroma, const lfi_yuv_surfaces *src)
{
    return upload_mosaic_yuv_surfaces(ctx, "lfi_upload_mosaic_yuv", m, g0, matrix, range, chroma, src, false);
}

int lfi_upload_mosaic_yuv_derived(lfi_ctx *ctx, const lfi_mosaic *m, int g0, int matrix, int range, int chroma, const lfi_yuv_surfaces *src)
{
    return upload_mosaic_yuv_surfaces(ctx, "lfi_upload_mosaic_yuv_derived", m, g0, matrix, range, chroma, src, true);
}

int lfi_debug_set_mosaic_chunk_cap(lfi_ctx *ctx, size_t cap_bytes)
{
    if(!ctx)
        return LFI_EINVAL;
    ctx->mosaic_chunk_cap = cap_bytes;
    return LFI_OK;
}

int lfi_upload_mosaic(lfi_ctx *ctx, const lfi_mosaic *m, int g0, const uint8_t *rgba, size_t pitch_bytes)
{
    const char *who = "lfi_upload_mosaic";
    if(!ctx)
        return LFI_EINVAL;
    if(!ctx->grid && !ctx->inputs_released)
        return fail(ctx, LFI_EINVAL, "lfi_set_grid has not been called");
    if(const char *fault = mosaic_fault(m, ctx->cols, ctx->rows, g0))
        return fail(ctx, LFI_EINVAL, std::string(who) + ": " + fault);
    if(!rgba || pitch_bytes / 4 / (size_t)m->tiles_x < (size_t)ctx->width)
        return fail(ctx, LFI_EINVAL, std::string(who) + ": the image's pointer is NULL or pitch_bytes is below tiles_x * W * 4");
    const lfi::MosaicMap map = mosaic_map_of(*m, ctx->rows, g0);
    for(int k = 0; k < m->n; k++)
    {
        // lfi_upload_image_async of the tile's rectangle: one 2D copy on the copy stream
        uint32_t tx, ty, g;
        lfi::mosaic_tile(map, (uint32_t)k, tx, ty, g);
        if(int rc = lfi_upload_image_async(ctx, (int)g, rgba + (size_t)ty * ctx->height * pitch_bytes + (size_t)tx * ctx->width * 4, pitch_bytes))
            return rc;
    }
    return LFI_OK;
}

namespace {

// the planar copy holds the current inputs: the only copy of them (lfi_release_inputs), or one that a render has brought up to date
bool derived_copy_current(const lfi_ctx *ctx)
{
    return ctx->planar && (int)ctx->planar_phase.size() == ctx->n && ctx->n > 0 && (ctx->inputs_released || ctx->planar_version == ctx->grid_version);
}

} // namespace

int lfi_debug_streams(lfi_ctx *ctx, void **out3)
{
    if(!ctx || !out3)
        return LFI_EINVAL;
    if(int rc = bind(ctx))
        return rc;
    if(int rc = ensure_copy_stream(ctx))
        return rc;
    if(int rc = ensure_aux_stream(ctx))
        return rc;
    out3[0] = static_cast<hipStream_t>(ctx->own_stream);
    out3[1] = static_cast<hipStream_t>(ctx->copy_stream);
    out3[2] = static_cast<hipStream_t>(ctx->aux_stream);
    return LFI_OK;
}

int lfi_debug_derived_layout(lfi_ctx *ctx, lfi_derived_layout *out, int32_t *phases_n)
{
    if(!ctx || !out)
        return LFI_EINVAL;
    if(!derived_copy_current(ctx))
        return fail(ctx, LFI_EINVAL, "lfi_debug_derived_layout: the context holds no current planar copy of the inputs");
    out->pitch_bytes = (size_t)ctx->planar_pitch;
    out->rows = ctx->in_rows, out->padx = ctx->planar_padx, out->reach = ctx->planar_reach, out->n = ctx->n;
    if(phases_n)
        std::copy(ctx->planar_phase.begin(), ctx->planar_phase.end(), phases_n);
    return LFI_OK;
}

int lfi_debug_download_derived(lfi_ctx *ctx, int g0, int n, uint8_t *out)
{
    if(!ctx)
        return LFI_EINVAL;
    if(!derived_copy_current(ctx))
        return fail(ctx, LFI_EINVAL, "lfi_debug_download_derived: the context holds no current planar copy of the inputs");
    if(n < 1 || g0 < 0 || (long)g0 + n > ctx->n || !out)
        return fail(ctx, LFI_EINVAL, "lfi_debug_download_derived: needs n >= 1 images starting at g0 inside [0, N) and a destination");
    if(int rc = bind(ctx))
        return rc;
    if(int rc = join_uploads(ctx)) // in stream order behind the uploads, as a render is
        return rc;
    const size_t image = (size_t)3 * ctx->in_rows * ctx->planar_pitch;
    LFI_HIP(ctx, hipMemcpyAsync(out, ctx->planar.get() + image * (size_t)g0, image * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LFI_OK;
}

int lfi_attach_grid(lfi_ctx *ctx, void *device_ptr, size_t bytes)
{
    if(!ctx)
        return LFI_EINVAL;
    if(!ctx->n)
        return fail(ctx, LFI_EINVAL, "lfi_set_grid has not been called");
    if(!device_ptr || bytes < in_plane_bytes(ctx) * ctx->n)
        return fail(ctx, LFI_EINVAL, "attached grid buffer is NULL or smaller than N*rows*W*4 bytes");
    if(reinterpret_cast<uintptr_t>(device_ptr) % 16)
        return fail(ctx, LFI_EINVAL, "attached grid buffer must be 16-byte aligned");
    if(int rc = bind(ctx))
        return rc;
    if(int rc = lfi_upload_wait(ctx))
        return rc;
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    drop_inputs(ctx);
    ctx->grid.attach(device_ptr, bytes);
    touch_all(ctx);
    ctx->grid_tracked = false; // the caller writes this buffer itself: see lfi_grid_modified
    return LFI_OK;
}

int lfi_broadcast_grid(lfi_ctx *const *ctxs, int n, int root)
{
    if(!ctxs || n < 1 || root < 0 || root >= n)
        return LFI_EINVAL;
    for(int i = 0; i < n; i++)
        if(!ctxs[i])
            return LFI_EINVAL;
    lfi_ctx *r0 = ctxs[root];
    if(!r0->grid)
        return fail(r0, LFI_EINVAL, "lfi_set_grid has not been called on the root context");
    if(n == 1)
        return LFI_OK;
    std::vector<int> devs(n);
    for(int i = 0; i < n; i++)
    {
        lfi_ctx *c = ctxs[i];
        if(!c->grid || c->n != r0->n || c->width != r0->width || c->height != r0->height || c->in_y0 != r0->in_y0 || c->in_rows != r0->in_rows)
            return fail(r0, LFI_EINVAL, "all contexts of a broadcast must describe the same grid and row window");
        devs[i] = c->device;
        for(int j = 0; j < i; j++)
            if(devs[j] == devs[i])
                return fail(r0, LFI_EINVAL, "the contexts of a broadcast must sit on distinct devices");
    }
    const Rccl &nc = rccl();
    if(!nc.ok)
        return fail(r0, LFI_EHIP, "librccl.so could not be loaded");
    for(int i = 0; i < n; i++)
        if(ctxs[i]->uploads_pending)
            if(int rc = lfi_upload_wait(ctxs[i]))
                return rc;
    int caller_device = -1; // the loop below walks the contexts' devices; the caller's current device is restored afterwards
    (void)hipGetDevice(&caller_device);
    std::vector<Rccl::comm_t> comms(n, nullptr);
    int rc = nc.CommInitAll(comms.data(), n, devs.data());
    if(rc != 0)
    {
        if(caller_device >= 0)
            (void)hipSetDevice(caller_device);
        return fail(r0, LFI_EHIP, std::string("ncclCommInitAll: ") + nc.GetErrorString(rc));
    }
    const size_t bytes = in_plane_bytes(r0) * r0->n;
    constexpr int NCCL_UINT8 = 1;
    int status = LFI_OK;
    rc = nc.GroupStart();
    for(int i = 0; i < n && rc == 0; i++)
    {
        if(hipSetDevice(ctxs[i]->device) != hipSuccess)
        {
            rc = -1;
            break;
        }
        rc = nc.Broadcast(r0->grid.get(), ctxs[i]->grid.get(), bytes, NCCL_UINT8, root, comms[i], ctxs[i]->stream);
    }
    const int rc_end = nc.GroupEnd();
    if(rc != 0 || rc_end != 0)
        status = fail(r0, LFI_EHIP, std::string("ncclBroadcast: ") + (rc > 0 ? nc.GetErrorString(rc) : rc_end ? nc.GetErrorString(rc_end) : "hipSetDevice failed"));
    for(int i = 0; i < n; i++)
    {
        (void)hipSetDevice(ctxs[i]->device);
        if(hipStreamSynchronize(ctxs[i]->stream) != hipSuccess && status == LFI_OK)
            status = fail(r0, LFI_EHIP, "hipStreamSynchronize after the broadcast failed");
    }
    for(int i = 0; i < n; i++)
    {
        (void)nc.CommDestroy(comms[i]);
        touch_all(ctxs[i]);
    }
    if(caller_device >= 0)
        (void)hipSetDevice(caller_device);
    return status;
}

int lfi_release_inputs(lfi_ctx *ctx)
{
    if(!ctx)
        return LFI_EINVAL;
    if(ctx->inputs_released)
        return LFI_OK;
    if(!ctx->grid || !ctx->have_params)
        return fail(ctx, LFI_EINVAL, "lfi_set_grid / lfi_set_params have not been called");
    if(int rc = bind(ctx))
        return rc;
    if(int rc = lfi_upload_wait(ctx))
        return rc;
    // the planar copy, complete and tuned for the current offsets, becomes the only copy of the inputs
    if(!ensure_planar(ctx, true))
        return fail(ctx, LFI_EINVAL, "the planar copy of the inputs cannot be built (inputs the library does not track, absurd offsets, out of memory)");
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    drop_inputs(ctx);
    ctx->inputs_released = true;
    return LFI_OK;
}

int lfi_grid_device_ptr(lfi_ctx *ctx, void **out_ptr, size_t *out_bytes)
{
    if(!ctx || !out_ptr)
        return LFI_EINVAL;
    if(ctx->inputs_released) // before anything is touched: the query must not cost the context its only copy of the inputs
        return fail(ctx, LFI_EINVAL, "the RGBA inputs were released (lfi_release_inputs): lfi_set_grid and upload the images again");
    if(ctx->uploads_pending && bind(ctx) == LFI_OK)
        (void)lfi_upload_wait(ctx); // the caller is about to read or write the planes itself
    *out_ptr = ctx->grid.get();
    if(out_bytes)
        *out_bytes = ctx->grid ? in_plane_bytes(ctx) * ctx->n : 0;
    ctx->grid_tracked = false; // the caller may write through the pointer: see lfi_grid_modified
    touch_all(ctx);
    return LFI_OK;
}

int lfi_grid_modified(lfi_ctx *ctx)
{
    if(!ctx)
        return LFI_EINVAL;
    if(ctx->inputs_released)
        return fail(ctx, LFI_EINVAL, "the RGBA inputs were released (lfi_release_inputs): lfi_set_grid and upload the images again");
    if(!ctx->grid)
        return fail(ctx, LFI_EINVAL, "lfi_set_grid has not been called");
    touch_all(ctx);
    ctx->grid_tracked = true; // the caller announces its writes from now on
    return LFI_OK;
}

int lfi_fill_synthetic_images(lfi_ctx *ctx, uint32_t seed, int g0, int g1)
{
    if(!ctx)
        return LFI_EINVAL;
    if(ctx->inputs_released)
        return fail(ctx, LFI_EINVAL, "the RGBA inputs were released (lfi_release_inputs): lfi_set_grid and upload the images again");
    if(!ctx->grid)
        return fail(ctx, LFI_EINVAL, "lfi_set_grid has not been called");
    if(g0 < 0 || g1 > ctx->n || g0 > g1)
        return fail(ctx, LFI_EINVAL, "image range [g0, g1) outside the grid");
    if(g0 == g1)
        return LFI_OK;
    if(int rc = bind(ctx))
        return rc;
    if(int rc = join_uploads(ctx))
        return rc;
    touch_images(ctx, g0, g1);
    hipLaunchKernelGGL(lfi::fill_synthetic, dim3(256 * 16), dim3(256), 0, ctx->stream, ctx->grid.get(), g0, g1 - g0, ctx->width,
                       ctx->in_rows, ctx->in_y0, seed);
    LFI_HIP(ctx, hipGetLastError());
    if(ctx->eager_planar && ctx->have_params)
        (void)ensure_planar(ctx); // as lfi_upload_image
    return LFI_OK;
}

int lfi_fill_synthetic_scene(lfi_ctx *ctx, uint32_t seed)
{
    if(!ctx)
        return LFI_EINVAL;
    if(ctx->inputs_released)
        return fail(ctx, LFI_EINVAL, "the RGBA inputs were released (lfi_release_inputs): lfi_set_grid and upload the images again");
    if(!ctx->grid || !ctx->have_params)
        return fail(ctx, LFI_EINVAL, "lfi_set_grid / lfi_set_params have not been called (the scene is built from the images' offsets)");
    if(int rc = bind(ctx))
        return rc;
    touch_all(ctx);
    hipLaunchKernelGGL(lfi::fill_scene, dim3(256 * 16), dim3(256), 0, ctx->stream, ctx->grid.get(), ctx->d_offsets, ctx->n, ctx->width, ctx->in_rows,
                       ctx->in_y0, seed, ctx->focus, ctx->range);
    LFI_HIP(ctx, hipGetLastError());
    return LFI_OK;
}

int lfi_fill_synthetic(lfi_ctx *ctx, uint32_t seed)
{
    return ctx ? lfi_fill_synthetic_images(ctx, seed, 0, ctx->n) : LFI_EINVAL;
}

int lfi_set_params(lfi_ctx *ctx, const lfi_params *p)
{
    if(!ctx)
        return LFI_EINVAL;
    if(!ctx->n)
        return fail(ctx, LFI_EINVAL, "lfi_set_grid has not been called");
    if(!p || p->views < 1 || !p->focused_offsets || !p->offsets || !p->weights_fp16)
        return fail(ctx, LFI_EINVAL, "lfi_params: views < 1 or a required array is NULL");
    if(p->n_focus_ids < 0 || p->n_focus_ids > LFI_MAX_FOCUS_IDS || (p->n_focus_ids > 0 && !p->focus_map_ids))
        return fail(ctx, LFI_EINVAL, "lfi_params: bad focus_map_ids");
    for(int i = 0; i < p->n_focus_ids; i++)
        if(p->focus_map_ids[i] < 0 || p->focus_map_ids[i] >= ctx->n)
            return fail(ctx, LFI_EINVAL, "lfi_params: focus_map_ids entry outside the grid");
    if(p->views > 4096)
        return fail(ctx, LFI_EINVAL, "lfi_params: more than 4096 views");
    if(int rc = bind(ctx))
        return rc;

    if(ctx->windowed)
        for(int g = 0; g < ctx->n; g++)
        {
            const int oy = p->focused_offsets[g].y, H = ctx->height;
            const int lo = std::min(std::max(ctx->out_y0 + oy, 0), H - 1), hi = std::min(std::max(ctx->out_y0 + ctx->out_rows - 1 + oy, 0), H - 1);
            if(lo < ctx->in_y0 || hi >= ctx->in_y0 + ctx->in_rows)
                return fail(ctx, LFI_EINVAL, "the input row window does not cover the rows image " + std::to_string(g) + " is sampled at");
        }
    ctx->view_offsets.set = ctx->view_float_offsets.set = false; // per-view rows belong to the parameters they were set for
    ctx->view_maps_set = false;                                   // … and so do the per-view maps
    const int n = ctx->n, V = p->views;
    const int k_pad = (n + 15) / 16 * 16;
    // 64 spare rows: a view range may start anywhere, and a wave always reads whole 32-row tiles
    const int v_pad = (V + 63) / 64 * 64 + 64;
    const bool views_changed = V != ctx->views_n;

    // host staging of the padded arrays, one blob
    const size_t off_focused = 0;
    const size_t off_offsets = off_focused + sizeof(lfi_int2) * k_pad;
    const size_t off_w16 = off_offsets + sizeof(lfi_float2) * k_pad;
    const size_t off_w16s = (off_w16 + sizeof(uint16_t) * (size_t)v_pad * k_pad + 15) / 16 * 16;
    const size_t off_w32 = (off_w16s + sizeof(uint16_t) * (size_t)v_pad * k_pad + 15) / 16 * 16;
    const size_t off_w32t = off_w32 + sizeof(float) * (size_t)v_pad * k_pad;
    const size_t off_ids = off_w32t + sizeof(float) * (size_t)v_pad * k_pad;
    const size_t total = off_ids + sizeof(int32_t) * LFI_MAX_FOCUS_IDS;
    // Same blob size as the arrays in place (and as many views: nothing else to reallocate): stage in page-locked memory and copy in
    // stream order — launches already enqueued keep reading the old arrays, later ones see the new; the context's stream is not
    // drained.  Otherwise (first call, another view count or grid): synchronise, reallocate, copy synchronously.
    const bool in_place = ctx->param_blob && ctx->param_total == total && !views_changed && ctx->views;
    std::vector<uint8_t> blob_pageable;
    uint8_t *blob_ptr = nullptr;
    if(in_place)
    {
        for(int i = 0; i < 2; i++)
            LFI_HIP(ctx, ctx->ev_half_done[i].ensure());
        LFI_HIP(ctx, ctx->param_ring.acquire(total, &blob_ptr));
        std::memset(blob_ptr, 0, total);
    }
    else
    {
        LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
        blob_pageable.assign(total, 0);
        blob_ptr = blob_pageable.data();
    }
    struct
    {
        uint8_t *p;
        uint8_t *data() const { return p; }
    } blob{blob_ptr};
    std::memcpy(blob.data() + off_focused, p->focused_offsets, sizeof(lfi_int2) * n);
    int fo_min[2] = {p->focused_offsets[0].x, p->focused_offsets[0].y}, fo_max[2] = {fo_min[0], fo_min[1]};
    for(int g = 1; g < n; g++)
    {
        fo_min[0] = std::min(fo_min[0], p->focused_offsets[g].x);
        fo_max[0] = std::max(fo_max[0], p->focused_offsets[g].x);
        fo_min[1] = std::min(fo_min[1], p->focused_offsets[g].y);
        fo_max[1] = std::max(fo_max[1], p->focused_offsets[g].y);
    }
    std::memcpy(blob.data() + off_offsets, p->offsets, sizeof(lfi_float2) * n);
    bool scalable = true, sums_ok = true;
    fill_weight_arrays(p->weights_fp16, V, n, k_pad, v_pad, blob.data() + off_w16, off_w16s - off_w16, off_w32 - off_w16, off_w32t - off_w16, &scalable,
                       &sums_ok);
    if(p->n_focus_ids)
        std::memcpy(blob.data() + off_ids, p->focus_map_ids, sizeof(int32_t) * p->n_focus_ids);

    if(in_place)
    {
        // into the device copy no launch reads any more, on the copy stream: beside the renders still running from the other copy.  Order:
        // the launches that read the idle copy were all enqueued before the context switched away from it (ev_half_done, recorded then);
        // launches enqueued from now on wait for this copy.
        if(int rc = ensure_copy_stream(ctx))
            return rc;
        const int cur = ctx->param_half, next = cur ^ 1;
        LFI_HIP(ctx, hipEventRecord(ctx->ev_half_done[cur], ctx->stream));
        ctx->half_done_recorded[cur] = true;
        if(ctx->half_done_recorded[next])
            LFI_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_half_done[next], 0));
        LFI_HIP(ctx, hipMemcpyAsync(ctx->param_blob.get() + (size_t)next * ctx->param_half_stride, blob.data(), total, hipMemcpyHostToDevice,
                                    ctx->copy_stream));
        LFI_HIP(ctx, ctx->param_ring.commit(ctx->copy_stream));
        LFI_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->param_ring.committed(), 0));
        ctx->param_half = next;
    }
    else
    {
        free_params(ctx);
        ctx->param_half_stride = (total + 255) / 256 * 256;
        LFI_HIP(ctx, ctx->param_blob.fit(2 * ctx->param_half_stride));
        ctx->param_total = total;
        LFI_HIP(ctx, hipMemcpy(ctx->param_blob.get(), blob.data(), total, hipMemcpyHostToDevice));
    }
    uint8_t *base = param_base(ctx);
    ctx->d_focused = reinterpret_cast<lfi_int2 *>(base + off_focused);
    ctx->d_offsets = reinterpret_cast<lfi_float2 *>(base + off_offsets);
    ctx->d_w16 = reinterpret_cast<uint16_t *>(base + off_w16);
    ctx->d_w16s = reinterpret_cast<uint16_t *>(base + off_w16s);
    ctx->weights_scalable = scalable;
    ctx->weights_sum_ok = sums_ok;
    ctx->d_w32 = reinterpret_cast<float *>(base + off_w32);
    ctx->d_w32t = reinterpret_cast<float *>(base + off_w32t);
    ctx->d_ids = reinterpret_cast<int32_t *>(base + off_ids);
    ctx->blob_off_w16 = off_w16;
    ctx->blob_weights_bytes = off_ids - off_w16;
    ctx->k_pad = k_pad;
    ctx->v_pad = v_pad;
    ctx->views_n = V;
    ctx->n_focus_ids = p->n_focus_ids;
    ctx->h_offsets.assign(p->offsets, p->offsets + n);
    if((int)ctx->h_focused.size() != n || std::memcmp(ctx->h_focused.data(), p->focused_offsets, sizeof(lfi_int2) * n) != 0)
        ctx->launches_with_offsets = 0; // new integer offsets: the planar copy's phases may no longer fit them (ensure_planar)
    ctx->h_focused.assign(p->focused_offsets, p->focused_offsets + n);
    ctx->h_focus_offsets.clear();
    for(int k = 0; k < p->n_focus_ids; k++)
        ctx->h_focus_offsets.push_back(p->offsets[p->focus_map_ids[k]]);
    ctx->h_focus_ids.assign(p->focus_map_ids, p->focus_map_ids + p->n_focus_ids);
    ctx->focus = p->focus;
    ctx->range = p->range;
    for(int d = 0; d < 2; d++)
    {
        ctx->fo_min[d] = fo_min[d];
        ctx->fo_max[d] = fo_max[d];
    }
    ctx->radius[0] = std::max(p->block_radius[0], 1);
    ctx->radius[1] = std::max(p->block_radius[1], 1);
    ctx->flags = p->flags & 0x7fffffffu; // (bit 31 is the dispatcher's own: LFI_KFLAG_PLAIN_TILE_ORDER, lfi_device.hpp)

    if(views_changed)
        drop_deep_range(ctx); // (an attached view buffer that is still large enough keeps the views: the deep views of the old parameters go all the same)
    if(views_changed)
        drop_kept(ctx); // the kept views' indices belong to the old number of views (the stream has been drained above)
    if(views_changed || !ctx->views)
    {
        const bool was_attached = ctx->views && !ctx->views.owned();
        if(!(was_attached && ctx->views.bytes() >= out_plane_bytes(ctx) * V))
        {
            free_views(ctx);
            ctx->have_params = false; // until the views exist: a failed allocation must not leave renders a null pointer to store through
            LFI_HIP(ctx, alloc_views(ctx->views, out_plane_bytes(ctx) * V));
        }
    }
    ctx->have_params = true;
    return LFI_OK;
}

int lfi_set_view_offsets(lfi_ctx *ctx, const lfi_int2 *focused_offsets_vn, int views)
{
    if(!ctx)
        return LFI_EINVAL;
    if(!ctx->have_params)
        return fail(ctx, LFI_EINVAL, "lfi_set_params has not been called");
    if(!focused_offsets_vn)
    {
        ctx->view_offsets.set = false;
        return LFI_OK;
    }
    if(views != ctx->views_n)
        return fail(ctx, LFI_EINVAL, "lfi_set_view_offsets: views (" + std::to_string(views) + ") differs from lfi_params.views (" +
                                         std::to_string(ctx->views_n) + ")");
    if(int rc = bind(ctx))
        return rc;
    const int n = ctx->n, W = ctx->width, H = ctx->height;
    // A shift beyond the image samples its edge for every pixel, exactly as a shift of ±W / ±H does (clamp to edge): clamping here keeps
    // every coordinate the kernel forms far from int overflow and changes no result.
    auto at = [&](int v, int g) {
        lfi_int2 d = focused_offsets_vn[(size_t)v * n + g];
        d.x = std::min(std::max(d.x, -W), W);
        d.y = std::min(std::max(d.y, -H), H);
        return d;
    };
    if(ctx->windowed)
        for(int v = 0; v < views; v++)
            for(int g = 0; g < n; g++)
            {
                const int oy = at(v, g).y;
                const int lo = std::min(std::max(ctx->out_y0 + oy, 0), H - 1), hi = std::min(std::max(ctx->out_y0 + ctx->out_rows - 1 + oy, 0), H - 1);
                if(lo < ctx->in_y0 || hi >= ctx->in_y0 + ctx->in_rows)
                    return fail(ctx, LFI_EINVAL, "the input row window does not cover the rows image " + std::to_string(g) + " is sampled at in view " +
                                                     std::to_string(v));
            }
    int reach = 0;
    if(int rc = stage_view_rows(ctx, ctx->view_offsets, [&](int v, int g) {
           const lfi_int2 d = at(v, g);
           reach = std::max(reach, std::abs(d.x));
           return d;
       }))
        return rc;
    ctx->view_offsets_reach = reach;
    return LFI_OK;
}

int lfi_set_view_float_offsets(lfi_ctx *ctx, const lfi_float2 *offsets_vn, int views)
{
    if(!ctx)
        return LFI_EINVAL;
    if(!ctx->have_params)
        return fail(ctx, LFI_EINVAL, "lfi_set_params has not been called");
    if(!offsets_vn)
    {
        ctx->view_float_offsets.set = false;
        ctx->view_maps_set = false;
        return LFI_OK;
    }
    if(views != ctx->views_n)
        return fail(ctx, LFI_EINVAL, "lfi_set_view_float_offsets: views (" + std::to_string(views) + ") differs from lfi_params.views (" +
                                         std::to_string(ctx->views_n) + ")");
    const int n = ctx->n;
    for(size_t i = 0; i < (size_t)views * n; i++)
        if(!std::isfinite(offsets_vn[i].x) || !std::isfinite(offsets_vn[i].y))
            return fail(ctx, LFI_EINVAL, "lfi_set_view_float_offsets: offsets must be finite");
    if(int rc = bind(ctx))
        return rc;
    ctx->view_maps_set = false; // estimated for the rows these replace
    if(int rc = stage_view_rows(ctx, ctx->view_float_offsets, [&](int v, int g) { return offsets_vn[(size_t)v * n + g]; }))
        return rc;
    ctx->h_view_float_offsets.assign(offsets_vn, offsets_vn + (size_t)views * n);
    return LFI_OK;
}

int lfi_attach_views(lfi_ctx *ctx, void *device_ptr, size_t bytes)
{
    if(!ctx)
        return LFI_EINVAL;
    if(!ctx->have_params)
        return fail(ctx, LFI_EINVAL, "lfi_set_params has not been called");
    if(!device_ptr || bytes < out_plane_bytes(ctx) * ctx->views_n)
        return fail(ctx, LFI_EINVAL, "attached view buffer is NULL or smaller than the views in the current layout (lfi_view_layout)");
    if(reinterpret_cast<uintptr_t>(device_ptr) % 16)
        return fail(ctx, LFI_EINVAL, "attached view buffer must be 16-byte aligned");
    if(int rc = bind(ctx))
        return rc;
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    free_views(ctx);
    ctx->views.attach(device_ptr, bytes);
    return LFI_OK;
}

int lfi_set_output_layout(lfi_ctx *ctx, int layout)
{
    if(!ctx)
        return LFI_EINVAL;
    if(layout != LFI_LAYOUT_RGBA && layout != LFI_LAYOUT_PLANAR_RGB)
        return fail(ctx, LFI_EINVAL, "unknown view layout");
    if(!ctx->n)
        return fail(ctx, LFI_EINVAL, "lfi_set_grid has not been called");
    if(layout == ctx->out_layout)
        return LFI_OK;
    if(int rc = bind(ctx))
        return rc;
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    free_views(ctx); // an attached buffer is dropped too: its size belongs to the old layout
    drop_kept(ctx);  // kept in the old layout
    ctx->out_layout = layout;
    if(ctx->have_params)
    {
        ctx->have_params = false; // a failed allocation leaves the context without parameters (lfi_set_params again), not with null views
        LFI_HIP(ctx, alloc_views(ctx->views, out_plane_bytes(ctx) * ctx->views_n));
        ctx->have_params = true;
    }
    return LFI_OK;
}

int lfi_view_layout(lfi_ctx *ctx, lfi_view_layout_info *out)
{
    if(!ctx || !out)
        return LFI_EINVAL;
    if(!ctx->n)
        return fail(ctx, LFI_EINVAL, "lfi_set_grid has not been called");
    out->layout = ctx->out_layout;
    out->rows = ctx->out_rows;
    if(ctx->out_layout == LFI_LAYOUT_PLANAR_RGB)
    {
        out->row_pitch_bytes = (size_t)view_pitch(ctx);
        out->plane_stride_bytes = (size_t)ctx->out_rows * view_pitch(ctx);
    }
    else
    {
        out->row_pitch_bytes = (size_t)ctx->width * 4;
        out->plane_stride_bytes = 0;
    }
    out->view_stride_bytes = out_plane_bytes(ctx);
    return LFI_OK;
}

int lfi_views_device_ptr(lfi_ctx *ctx, void **out_ptr, size_t *out_bytes)
{
    if(!ctx || !out_ptr)
        return LFI_EINVAL;
    *out_ptr = ctx->views.get();
    if(out_bytes)
        *out_bytes = ctx->views ? out_plane_bytes(ctx) * ctx->views_n : 0;
    return LFI_OK;
}

// map 1 = the box mean of map 0 over the rows a.map_y0 … + a.map_rows: from LDS (focus_filter_tiled) when the window allows it.
// views > 0: a.maps holds that many pairs [views][2][H][W] (lfi_view_focus_maps), all filtered by one launch
static void launch_focus_filter(lfi_ctx *ctx, const lfi::KernelArgs &a, hipStream_t st, int views = 0)
{
    const int rx = std::max(ctx->radius[0] / 10, 1), ry = std::max(ctx->radius[1] / 10, 1);
    const size_t lds = lfi::focus_filter_tiled_lds(rx, ry);
    const bool tiled = rx <= 128 && ry <= 128 && lds <= 64u * 1024u;
    if(views > 0)
    {
        if(tiled)
            hipLaunchKernelGGL(lfi::focus_filter_tiled_views, dim3((ctx->width + lfi::FF_TW - 1) / lfi::FF_TW, (a.map_rows + lfi::FF_TH - 1) / lfi::FF_TH, views),
                               dim3(256), lds, st, a);
        else
            hipLaunchKernelGGL(lfi::focus_filter_views, dim3((ctx->width + 63) / 64, (a.map_rows + 3) / 4, views), dim3(256), 0, st, a);
    }
    else if(tiled)
        hipLaunchKernelGGL(lfi::focus_filter_tiled, dim3((ctx->width + lfi::FF_TW - 1) / lfi::FF_TW, (a.map_rows + lfi::FF_TH - 1) / lfi::FF_TH), dim3(256), lds, st, a);
    else
        hipLaunchKernelGGL(lfi::focus_filter, dim3((ctx->width + 63) / 64, (a.map_rows + 3) / 4), dim3(256), 0, st, a);
}

int lfi_set_focus_steps(lfi_ctx *ctx, int steps)
{
    if(!ctx)
        return LFI_EINVAL;
    if(steps < lfi::FOCUS_STEPS || steps > lfi::FOCUS_STEPS * lfi::FOCUS_MAX_PASSES || steps % lfi::FOCUS_STEPS != 0)
        return fail(ctx, LFI_EINVAL, "lfi_set_focus_steps: " + std::to_string(steps) + " candidates - the focus map takes a multiple of 32 from 32 to 256");
    ctx->focus_steps = steps;
    return LFI_OK;
}

int lfi_set_yuv_siting(lfi_ctx *ctx, int in_siting, int out_siting)
{
    if(!ctx)
        return LFI_EINVAL;
    const auto known = [](int s) { return s == LFI_YUV_SITING_CENTRE || s == LFI_YUV_SITING_LEFT; };
    if(!known(in_siting) || !known(out_siting))
        return fail(ctx, LFI_EINVAL, "lfi_set_yuv_siting: unknown chroma siting (LFI_YUV_SITING_CENTRE, LFI_YUV_SITING_LEFT) - in " + std::to_string(in_siting) +
                                         ", out " + std::to_string(out_siting));
    ctx->yuv_in_siting = in_siting, ctx->yuv_out_siting = out_siting;
    return LFI_OK;
}

int lfi_yuv_siting(lfi_ctx *ctx, int *in_siting, int *out_siting)
{
    if(!ctx || !in_siting || !out_siting)
        return LFI_EINVAL;
    *in_siting = ctx->yuv_in_siting, *out_siting = ctx->yuv_out_siting;
    return LFI_OK;
}

int lfi_focus_steps(lfi_ctx *ctx, int *out_steps)
{
    if(!ctx || !out_steps)
        return LFI_EINVAL;
    *out_steps = ctx->focus_steps;
    return LFI_OK;
}

// What every focus entry point asks before it enqueues anything, in this order: the RGBA inputs, the grid and the parameters; no row window
// unless the call computes a band (window_allowed); the call's own arguments (args_error: empty when they are fine); sampled images
// (centre_ids: the parameters' focus_map_ids — lfi_view_focus_maps brings its own) and a search interval; then the device is bound and the
// uploads in flight are joined.  call: the entry point's name; noun: what it computes, as the messages name it.
static int focus_entry(lfi_ctx *ctx, const char *call, const std::string &noun, bool window_allowed, const std::string &args_error, bool centre_ids = true)
{
    if(ctx->inputs_released)
        return fail(ctx, LFI_EINVAL, "the RGBA inputs were released (lfi_release_inputs): the " + noun + (noun.back() == 's' ? " need" : " needs") +
                                         " them - upload the images again (lfi_set_grid)");
    if(!ctx->grid || !ctx->have_params)
        return fail(ctx, LFI_EINVAL, "lfi_set_grid / lfi_set_params have not been called");
    if(ctx->windowed && !window_allowed)
        return fail(ctx, LFI_EINVAL, std::string(call) + " does not work on a row window");
    if(!args_error.empty())
        return fail(ctx, LFI_EINVAL, args_error);
    if(centre_ids && ctx->n_focus_ids < 1)
        return fail(ctx, LFI_EINVAL, "no focus_map_ids in the parameters");
    if(!(ctx->range > 0.0f))
        return fail(ctx, LFI_EINVAL, "focus range must be > 0 for the " + noun + ": [focus, focus + range] is the search interval");
    if(int rc = bind(ctx))
        return rc;
    return join_uploads(ctx);
}

int lfi_focus_map(lfi_ctx *ctx)
{
    if(!ctx)
        return LFI_EINVAL;
    // lfi_set_focus_steps: the sweep's length.  The factored estimate (one pass per 32 candidates) and focus_estimate_packed_sweep honour it;
    // the LDS-staged and the plain kernel are the reference's 32 candidates as written and refuse any other number
    const bool fine = ctx->focus_steps != lfi::FOCUS_STEPS;
    std::string bad;
    if(fine && !ctx->windowed && (ctx->focus_variant == 1 || ctx->focus_variant == 3))
        bad = std::string("lfi_focus_map: the estimate variant \"") + (ctx->focus_variant == 1 ? "lds" : "plain") +
              "\" computes 32 candidates only (lfi_set_focus_steps is " + std::to_string(ctx->focus_steps) + ")";
    if(int rc = focus_entry(ctx, "lfi_focus_map", "focus map", true, bad))
        return rc;
    if(int rc = join_filter(ctx)) // the previous map's filter still reads map 0, which this call rewrites
        return rc;
    route_begin(ctx);
    KernelArgs a = make_args(ctx, 0, ctx->views_n, LFI_METHOD_STD);
    a.focus_steps = ctx->focus_steps;
    a.focus_div = float(ctx->focus_steps - 1);
    if(ctx->windowed)
    {
        // Row window (spatial sharding): the maps are whole-image planes, but only the band's rows are computed — map 0 for the band
        // plus the filter's reach above and below, map 1 for the band — by the one-wave-per-row kernel from the input rows held.
        const int H = ctx->height, fry = std::max(ctx->radius[1] / 10, 1), ry = ctx->radius[1];
        const int e0 = std::max(ctx->out_y0 - fry, 0), e1 = std::min(ctx->out_y0 + ctx->out_rows + fry, H);
        const float f_lo = std::min(ctx->focus, ctx->focus + ctx->range), f_hi = std::max(ctx->focus, ctx->focus + ctx->range);
        for(const lfi_float2 &o : ctx->h_focus_offsets)
        {
            const double d_lo = std::min((double)f_lo * o.y, (double)f_hi * o.y), d_hi = std::max((double)f_lo * o.y, (double)f_hi * o.y);
            const int lo = std::min(std::max((int)std::floor(e0 + d_lo) - 1 - ry, 0), H - 1);
            const int hi = std::min(std::max((int)std::ceil(e1 - 1 + d_hi) + 1 + ry, 0), H - 1);
            if(lo < ctx->in_y0 || hi >= ctx->in_y0 + ctx->in_rows)
                return fail(ctx, LFI_EINVAL, "the input row window does not cover the rows the focus map of this band samples");
        }
        a.map_y0 = e0;
        a.map_rows = e1 - e0;
        ctx->route.estimate = "row_window";
        if(fine)
            hipLaunchKernelGGL((lfi::focus_estimate_packed_sweep<2, 4>), dim3((ctx->width + 127) / 128, a.map_rows), dim3(64), 0, ctx->stream, a);
        else
            hipLaunchKernelGGL((lfi::focus_estimate_packed<2, 4>), dim3((ctx->width + 127) / 128, a.map_rows), dim3(64), 0, ctx->stream, a);
        LFI_HIP(ctx, hipGetLastError());
        a.map_y0 = ctx->out_y0;
        a.map_rows = ctx->out_rows;
        launch_focus_filter(ctx, a, ctx->stream);
        LFI_HIP(ctx, hipGetLastError());
        return LFI_OK;
    }
    // the LDS-staged kernel needs its window (128 + 2·radius_x + slack pixels) to fit a 256-pixel LDS row
    const bool lds_fits = 128 + 2 * ctx->radius[0] + 2 * lfi::FOCUS_LDS_SLACK <= lfi::FOCUS_LDS_ROW;
    // "factored" (default): W and H must fit the 16-bit column / row lists
    bool done = false;
    if((ctx->focus_variant == 0 || ctx->focus_variant == 4) && ctx->width <= 65535 && ctx->height <= 65535)
    {
        FocusJob job;
        job.offsets = ctx->h_focus_offsets.data();
        job.ids = ctx->h_focus_ids.data();
        job.n_ids = ctx->n_focus_ids;
        if(int rc = launch_focus_factored(ctx, a, job, &done, ctx->focus_variant == 4))
            return rc;
    }
    if(done)
        ;
    else if(fine) // "packed_p2", and where the factored estimate declined: the variant that takes any number of candidates
    {
        ctx->route.estimate = "packed_p2";
        hipLaunchKernelGGL((lfi::focus_estimate_packed_sweep<2, 4>), dim3((ctx->width + 127) / 128, ctx->height), dim3(64), 0, ctx->stream, a);
    }
    else if(ctx->focus_variant <= 1 && lds_fits) // "lds"
    {
        ctx->route.estimate = "lds";
        hipLaunchKernelGGL(lfi::focus_estimate_lds, dim3((ctx->width + 127) / 128, ctx->height), dim3(64), 0, ctx->stream, a);
    }
    else if(ctx->focus_variant == 3) // "plain": one pixel per lane, float min/max exactly as the reference writes it
    {
        ctx->route.estimate = "plain";
        hipLaunchKernelGGL(lfi::focus_estimate, pixel_grid(ctx), dim3(256), 0, ctx->stream, a);
    }
    else // "packed_p2" (also the fallback of "lds" for very large radii)
    {
        ctx->route.estimate = "packed_p2";
        hipLaunchKernelGGL((lfi::focus_estimate_packed<2, 4>), dim3((ctx->width + 127) / 128, ctx->height), dim3(64), 0, ctx->stream, a);
    }
    LFI_HIP(ctx, hipGetLastError());
    if(done && ctx->aux_stream)
    {
        // map 1 = the box mean of map 0 (FocusMap::filter, src/kernels.cu:260-280), on the side stream: the reference's Tensors::process<true>
        // reads map 0 (src/kernels.cu:430), so a TEN_WM all-focus render enqueued next runs BESIDE the filter (0.13 ms at 4K) instead of
        // behind it; everything that reads map 1 or writes a map joins the side stream first (join_filter)
        LFI_HIP(ctx, ctx->ev_pick.ensure());
        LFI_HIP(ctx, ctx->ev_filter.ensure());
        LFI_HIP(ctx, hipEventRecord(ctx->ev_pick, ctx->stream));
        LFI_HIP(ctx, hipStreamWaitEvent(ctx->aux_stream, ctx->ev_pick, 0));
        launch_focus_filter(ctx, a, ctx->aux_stream);
        LFI_HIP(ctx, hipGetLastError());
        LFI_HIP(ctx, hipEventRecord(ctx->ev_filter, ctx->aux_stream));
        ctx->filter_pending = true;
        return LFI_OK;
    }
    launch_focus_filter(ctx, a, ctx->stream);
    LFI_HIP(ctx, hipGetLastError());
    return LFI_OK;
}

int lfi_focus_curve(lfi_ctx *ctx, int x0, int y0, int x1, int y1, int steps, uint64_t *out_cost, lfi_focus_curve_result *out)
{
    if(!ctx)
        return LFI_EINVAL;
    const char *bad = !out ? "lfi_focus_curve: out is NULL"
                      : steps < 2 || steps > lfi::FOCUS_CURVE_MAX_STEPS ? "lfi_focus_curve: steps must be in [2, 256]"
                      : x0 < 0 || y0 < 0 || x1 > ctx->width || y1 > ctx->height || x0 >= x1 || y0 >= y1 ? "lfi_focus_curve: the region is empty or leaves the image"
                                                                                                        : "";
    if(int rc = focus_entry(ctx, "lfi_focus_curve", "focus curve", false, bad))
        return rc;
    const KernelArgs a = make_args(ctx, 0, ctx->views_n, LFI_METHOD_STD);
    const uint8_t *d_head = nullptr;
    if(int rc = launch_focus_curve(ctx, a, x0, y0, x1, y1, steps, &d_head))
        return rc;
    // the curve and the result lie back to back: one copy of steps · 8 + 16 bytes
    uint64_t head[focus_curve_head(lfi::FOCUS_CURVE_MAX_STEPS) / sizeof(uint64_t)];
    LFI_HIP(ctx, hipMemcpyAsync(head, d_head, focus_curve_head(steps), hipMemcpyDeviceToHost, ctx->stream));
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if(out_cost)
        std::memcpy(out_cost, head, sizeof(uint64_t) * steps);
    std::memcpy(out, head + steps, sizeof(lfi_focus_curve_result));
    return LFI_OK;
}

int lfi_focus_tiles(lfi_ctx *ctx, int tiles_x, int tiles_y, uint64_t *out_cost, lfi_focus_curve_result *out)
{
    return lfi_focus_tiles_steps(ctx, tiles_x, tiles_y, LFI_FOCUS_TILE_STEPS, out_cost, out);
}

int lfi_focus_tiles_passes(const lfi_ctx *ctx)
{
    return ctx ? ctx->tiles_passes : 0;
}

int lfi_focus_route_info(lfi_ctx *ctx, lfi_focus_route *out)
{
    if(!ctx || !out)
        return LFI_EINVAL;
    *out = ctx->route;
    if(out->passes < 1 || !ctx->focus_ws)
        return LFI_OK;
    if(int rc = bind(ctx))
        return rc;
    // the plan runs on the side stream, which the compute stream joins in front of the keys: behind the compute stream's work the counts stand
    uint32_t totals[2 * LFI_FOCUS_ROUTE_PASSES];
    LFI_HIP(ctx, hipMemcpyAsync(totals, ctx->focus_ws.get() + ctx->route_counts_at, sizeof(totals), hipMemcpyDeviceToHost, ctx->stream));
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for(int p = 0; p < out->passes; p++)
        out->row_entries[p] = totals[2 * p], out->col_entries[p] = totals[2 * p + 1];
    return LFI_OK;
}

// (steps is this call's argument: ctx->focus_steps, lfi_set_focus_steps' setting of lfi_focus_map, is neither read nor written)
int lfi_focus_tiles_steps(lfi_ctx *ctx, int tiles_x, int tiles_y, int steps, uint64_t *out_cost, lfi_focus_curve_result *out)
{
    if(!ctx)
        return LFI_EINVAL;
    std::string bad;
    if(!out)
        bad = "lfi_focus_tiles: out is NULL";
    else if(tiles_x < 1 || tiles_y < 1 || tiles_x > std::min(ctx->width, 256) || tiles_y > std::min(ctx->height, 256))
        bad = "lfi_focus_tiles: the grid must have 1 to min(width, 256) columns and 1 to min(height, 256) rows of tiles";
    else if(steps < lfi::FOCUS_STEPS || steps > lfi::FOCUS_STEPS * lfi::FOCUS_MAX_PASSES || steps % lfi::FOCUS_STEPS != 0)
        bad = "lfi_focus_tiles_steps: " + std::to_string(steps) + " candidates - the focus tiles take a multiple of 32 from 32 to 256";
    if(int rc = focus_entry(ctx, "lfi_focus_tiles", "focus tiles", false, bad))
        return rc;
    route_begin(ctx);
    const KernelArgs a = make_args(ctx, 0, ctx->views_n, LFI_METHOD_STD);
    const uint8_t *d_head = nullptr;
    if(int rc = launch_focus_tiles(ctx, a, tiles_x, tiles_y, steps, &d_head))
        return rc;
    // per tile the curve and the result lie back to back: one copy of tiles · (steps · 8 + 16) bytes
    const size_t tiles = size_t(tiles_x) * size_t(tiles_y);
    const size_t words = focus_curve_head(steps) / sizeof(uint64_t);
    std::vector<uint64_t> head(tiles * words);
    LFI_HIP(ctx, hipMemcpyAsync(head.data(), d_head, sizeof(uint64_t) * words * tiles, hipMemcpyDeviceToHost, ctx->stream));
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for(size_t t = 0; t < tiles; t++)
    {
        if(out_cost)
            std::memcpy(out_cost + t * steps, head.data() + t * words, sizeof(uint64_t) * steps);
        std::memcpy(out + t, head.data() + t * words + steps, sizeof(lfi_focus_curve_result));
    }
    return LFI_OK;
}

// the per-view maps [views_n][2][H][W], allocated (or grown) on first use; renders in flight may read the old buffer
static int ensure_view_maps(lfi_ctx *ctx)
{
    const size_t need = plane_bytes(ctx) * 2 * ctx->views_n;
    if(ctx->view_maps.bytes() >= need)
        return LFI_OK;
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->view_maps_set = false;
    LFI_HIP(ctx, ctx->view_maps.reserve(need));
    return LFI_OK;
}

// ids (n of them) in pad-slot order after `prev`, the slot layout of the padded planes: an image prev already holds keeps its slot, the
// others take the remaining slots in ascending order.  The estimate is a min / max over the set, so the order changes no byte.
static void pad_slot_order(const std::vector<int32_t> &prev, const int32_t *ids, int n, int32_t *out)
{
    std::vector<char> placed(n, 0);
    for(int k = 0; k < n; k++)
        out[k] = -1;
    if((int)prev.size() == n)
        for(int k = 0; k < n; k++)
            for(int j = 0; j < n; j++)
                if(!placed[j] && ids[j] == prev[k])
                {
                    out[k] = ids[j];
                    placed[j] = 1;
                    break;
                }
    int k = 0;
    for(int j = 0; j < n; j++)
        if(!placed[j])
        {
            while(out[k] >= 0)
                k++;
            out[k] = ids[j];
        }
}

int lfi_view_focus_maps(lfi_ctx *ctx, const int32_t *focus_ids_vk, int views, int n_ids)
{
    if(!ctx)
        return LFI_EINVAL;
    std::string bad;
    if(!ctx->view_float_offsets.set)
        bad = "lfi_view_focus_maps: no per-view float offsets (lfi_set_view_float_offsets)";
    else if(views != ctx->views_n)
        bad = "lfi_view_focus_maps: views (" + std::to_string(views) + ") differs from lfi_params.views (" + std::to_string(ctx->views_n) + ")";
    else if(n_ids < 1 || n_ids > LFI_MAX_FOCUS_IDS || !focus_ids_vk)
        bad = "lfi_view_focus_maps: n_ids must be in [1, LFI_MAX_FOCUS_IDS] and focus_ids_vk non-NULL";
    for(size_t i = 0; bad.empty() && i < (size_t)views * n_ids; i++)
        if(focus_ids_vk[i] < 0 || focus_ids_vk[i] >= ctx->n)
            bad = "lfi_view_focus_maps: id outside the grid in view " + std::to_string(i / n_ids);
    if(bad.empty() && (ctx->width > 65535 || ctx->height > 65535))
        bad = "lfi_view_focus_maps: image too large for the factored estimate";
    if(int rc = focus_entry(ctx, "lfi_view_focus_maps", "focus maps", false, bad, false))
        return rc;
    if(int rc = join_filter(ctx)) // the centre map's filter shares the side stream
        return rc;
    if(int rc = ensure_view_maps(ctx))
        return rc;
    route_begin(ctx);
    const int n = ctx->n, V = views;
    // every view's ids in slot order (slots stay with their images from view to view: only the images that change are padded again), the
    // offsets of its sampled images, and one pad geometry for the whole batch
    std::vector<int32_t> slots((size_t)V * n_ids);
    std::vector<lfi_float2> sampled((size_t)V * n_ids);
    std::vector<int32_t> prev = ctx->pad_ids;
    int need[2] = {0, 0};
    for(int v = 0; v < V; v++)
    {
        int32_t *row = slots.data() + (size_t)v * n_ids;
        pad_slot_order(prev, focus_ids_vk + (size_t)v * n_ids, n_ids, row);
        prev.assign(row, row + n_ids);
        for(int k = 0; k < n_ids; k++)
            sampled[(size_t)v * n_ids + k] = ctx->h_view_float_offsets[(size_t)v * n + row[k]];
        int sx = 0, sy = 0;
        if(!focus_pad_shift(ctx, sampled.data() + (size_t)v * n_ids, n_ids, &sx, &sy))
            return fail(ctx, LFI_EINVAL, "lfi_view_focus_maps: the shifts of view " + std::to_string(v) + " are too large");
        need[0] = std::max(need[0], sx);
        need[1] = std::max(need[1], sy);
    }
    // the estimate's arrays on the device: the float rows as [V][N] (the render's copy is [N][v_pad]) and the slot-ordered ids [V][n_ids]
    const size_t off_bytes = sizeof(lfi_float2) * (size_t)V * n, ids_at = (off_bytes + 255) / 256 * 256;
    const size_t total = ids_at + sizeof(int32_t) * (size_t)V * n_ids;
    if(ctx->view_focus_args.bytes() < total)
    {
        LFI_HIP(ctx, hipStreamSynchronize(ctx->stream)); // an estimate in flight may read the old buffer
        LFI_HIP(ctx, ctx->view_focus_args.reserve(total));
    }
    uint8_t *staged = nullptr;
    LFI_HIP(ctx, ctx->view_focus_ring.acquire(total, &staged));
    std::memcpy(staged, ctx->h_view_float_offsets.data(), off_bytes);
    std::memcpy(staged + ids_at, slots.data(), sizeof(int32_t) * slots.size());
    LFI_HIP(ctx, hipMemcpyAsync(ctx->view_focus_args.get(), staged, total, hipMemcpyHostToDevice, ctx->stream));
    LFI_HIP(ctx, ctx->view_focus_ring.commit(ctx->stream));
    const lfi_float2 *d_off = ctx->view_focus_args.as<const lfi_float2>();
    const int32_t *d_ids = reinterpret_cast<const int32_t *>(ctx->view_focus_args.get() + ids_at);
    ctx->view_maps_set = false; // until every view's pair is enqueued
    KernelArgs a = make_args(ctx, 0, V, LFI_METHOD_STD);
    a.n_focus_ids = n_ids;
    int padded = 0;
    for(int v = 0; v < V; v++)
    {
        a.offsets = d_off + (size_t)v * n;
        a.focus_ids = d_ids + (size_t)v * n_ids;
        a.maps = ctx->view_maps.get() + plane_bytes(ctx) * 2 * v;
        FocusJob job;
        job.offsets = sampled.data() + (size_t)v * n_ids;
        job.ids = slots.data() + (size_t)v * n_ids;
        job.n_ids = n_ids;
        job.need_shift[0] = need[0];
        job.need_shift[1] = need[1];
        job.slot_reuse = true;
        bool done = false;
        if(int rc = launch_focus_factored(ctx, a, job, &done, ctx->focus_variant == 4))
            return rc;
        if(!done)
            return fail(ctx, LFI_EINVAL, "lfi_view_focus_maps: the padded planes of these shifts would be too large");
        padded += job.padded;
    }
    // maps 1 of all views by one launch, on the compute stream (renders of either map follow in stream order)
    a.maps = ctx->view_maps.get();
    launch_focus_filter(ctx, a, ctx->stream, V);
    LFI_HIP(ctx, hipGetLastError());
    ctx->view_maps_padded = padded;
    ctx->view_maps_set = true;
    return LFI_OK;
}

// view v's map k on the device: the per-view maps of the current parameters
static int view_map_plane(lfi_ctx *ctx, int v, int k, const void *host, size_t pitch_bytes, uint8_t **out)
{
    if(!ctx->have_params || !ctx->view_maps || ctx->view_maps.bytes() < plane_bytes(ctx) * 2 * ctx->views_n)
        return fail(ctx, LFI_EINVAL, "no per-view focus maps (lfi_view_focus_maps)");
    if(v < 0 || v >= ctx->views_n || k < 0 || k > 1 || !host || pitch_bytes < (size_t)ctx->width * 4)
        return fail(ctx, LFI_EINVAL, "bad view index, map index, pointer or pitch");
    *out = ctx->view_maps.get() + plane_bytes(ctx) * (2 * (size_t)v + k);
    return LFI_OK;
}

int lfi_download_view_map(lfi_ctx *ctx, int v, int k, uint8_t *rgba, size_t pitch_bytes)
{
    if(!ctx)
        return LFI_EINVAL;
    uint8_t *src = nullptr;
    if(int rc = view_map_plane(ctx, v, k, rgba, pitch_bytes, &src))
        return rc;
    if(int rc = bind(ctx))
        return rc;
    LFI_HIP(ctx, hipMemcpy2DAsync(rgba, pitch_bytes, src, (size_t)ctx->width * 4, (size_t)ctx->width * 4, ctx->height, hipMemcpyDeviceToHost,
                                  ctx->stream));
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LFI_OK;
}

int lfi_upload_view_map(lfi_ctx *ctx, int v, int k, const uint8_t *rgba, size_t pitch_bytes)
{
    if(!ctx)
        return LFI_EINVAL;
    if(ctx->have_params)
    {
        if(int rc = bind(ctx))
            return rc;
        if(int rc = ensure_view_maps(ctx))
            return rc;
    }
    uint8_t *dst = nullptr;
    if(int rc = view_map_plane(ctx, v, k, rgba, pitch_bytes, &dst))
        return rc;
    LFI_HIP(ctx, hipMemcpy2DAsync(dst, (size_t)ctx->width * 4, rgba, pitch_bytes, (size_t)ctx->width * 4, ctx->height, hipMemcpyHostToDevice,
                                  ctx->stream));
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LFI_OK;
}

int lfi_render(lfi_ctx *ctx, int method, int all_focus, int v0, int v1)
{
    if(int rc = check_render_args(ctx, method, v0, v1))
        return rc;
    if(int rc = bind(ctx))
        return rc;
    const KernelArgs a = make_args(ctx, v0, v1, method);
    return launch_blend(ctx, method, all_focus, a);
}

int lfi_prepare(lfi_ctx *ctx, int method, int all_focus, int v0, int v1)
{
    if(int rc = check_render_args(ctx, method, v0, v1))
        return rc;
    if(int rc = bind(ctx))
        return rc;
    if(int rc = join_uploads(ctx))
        return rc;
    const KernelArgs a = make_args(ctx, v0, v1, method);
    ctx->derived_build_ms = 0.0f;
    if(ctx->flags & LFI_FLAG_LINEAR_LIGHT) // the copy below: a linear-light render is then only a launch.  (First: it refuses the other two beside it)
        if(int rc = flagged_refused(ctx, LFI_FLAG_LINEAR_LIGHT, all_focus, a))
            return rc;
    const bool in_frame = ctx->flags & LFI_FLAG_IN_FRAME; // the copy below: an in-frame render is then only a launch
    if(in_frame)
        if(int rc = flagged_refused(ctx, LFI_FLAG_IN_FRAME, all_focus, a))
            return rc;
    const bool deep = ctx->flags & LFI_FLAG_DEEP_VIEWS; // the copy below, then the deep planes: the first deep render is then only a launch
    if(deep)
        if(int rc = flagged_refused(ctx, LFI_FLAG_DEEP_VIEWS, all_focus, a))
            return rc;
    const ViewRowsKind rows = view_rows_of(ctx, all_focus);
    bool planar = false;
    if(rows == VIEW_ROWS_FLOAT) // the RGBA planes are read as they are, nothing to build
        return view_rows_ready(ctx, rows, all_focus, a, &planar);
    if(rows == VIEW_ROWS_INT) // the copy padded for the per-view shifts, as launch_view_rows makes it
    {
        const uint64_t before = ctx->planar_version;
        LFI_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        if(int rc = view_rows_ready(ctx, rows, all_focus, a, &planar))
            return rc;
        LFI_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        LFI_HIP(ctx, hipEventSynchronize(ctx->ev1));
        if(planar && ctx->planar_version != before)
            LFI_HIP(ctx, hipEventElapsedTime(&ctx->derived_build_ms, ctx->ev0, ctx->ev1));
        return LFI_OK;
    }
    if(route_blend(ctx, method, all_focus != 0, a, true).reads_copy) // the route launch_blend takes
    {
        ctx->eager_planar = true; // images that arrive from now on refresh their planes of the copy at once
        const uint64_t before = ctx->planar_version;
        LFI_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        const bool ok = ensure_planar(ctx, true);
        LFI_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        LFI_HIP(ctx, hipEventSynchronize(ctx->ev1));
        if(ok && ctx->planar_version != before)
            LFI_HIP(ctx, hipEventElapsedTime(&ctx->derived_build_ms, ctx->ev0, ctx->ev1));
    }
    if(deep)
        return ensure_deep_planes(ctx);
    return LFI_OK;
}

int lfi_memory_info(lfi_ctx *ctx, lfi_memory *out)
{
    if(!ctx || !out)
        return LFI_EINVAL;
    out->grid_bytes = ctx->grid ? in_plane_bytes(ctx) * ctx->n : 0;
    out->derived_bytes = ctx->planar.bytes();
    out->views_bytes = ctx->views.bytes() + ctx->deep.bytes(); // the deep planes (LFI_FLAG_DEEP_VIEWS) belong to the views
    out->maps_bytes = (ctx->maps ? plane_bytes(ctx) * 2 : 0) + ctx->view_maps.bytes();
    out->workspace_bytes = ctx->focus_ws.bytes() + ctx->curve_ws.bytes() + ctx->rgba_scratch.bytes() + ctx->dl_plane.bytes() + ctx->kept.bytes() +
                           ctx->cmp_stage[0].bytes() + ctx->cmp_stage[1].bytes() + ctx->cmp_ws.bytes() + ctx->native.bytes() + ctx->yuv[0].bytes() + ctx->yuv[1].bytes() +
                           ctx->yuv_in.bytes() + ctx->quilt.bytes();
    out->derived_build_ms = ctx->derived_build_ms;
    return LFI_OK;
}

int lfi_std_band_info(lfi_ctx *ctx, lfi_std_band *out)
{
    if(!ctx || !out)
        return LFI_EINVAL;
    if(int rc = bind(ctx))
        return rc;
    const BandProbe *p = nullptr;
    if(int rc = run_band_probe(ctx, &p))
        return rc;
    std::memset(out, 0, sizeof(*out));
    out->probed = p->done;
    out->within_budget = p->ok;
    out->analytic_forced = (!p->ok || (ctx->flags & LFI_FLAG_STD_BAND_PROBE_FAIL)) && !(ctx->flags & LFI_FLAG_STD_ANALYTIC_BAND);
    out->sums = p->sums;
    out->worst_fraction = p->worst;
    out->probe_ms = p->ms;
    std::snprintf(out->message, sizeof(out->message),
                  p->ok ? (ctx->flags & LFI_FLAG_STD_BAND_PROBE_FAIL ? "measured bound holds (worst %.3f of the budget over %d sums); analytic band forced by LFI_FLAG_STD_BAND_PROBE_FAIL"
                                                                      : "measured bound holds on this device: worst %.3f of the budget over %d sums")
                        : "measured bound VIOLATED on this device (worst %.3f of the budget over %d sums): STD over more than 64 images takes the analytic band",
                  p->worst, p->sums);
    return LFI_OK;
}

const char *lfi_last_kernel_name(const lfi_ctx *ctx)
{
    return ctx ? ctx->last_kernel : "";
}

// ---- YUV 4:2:0 frames (yuv_surfaces.hpp, yuv420.hpp) --------------------------------------------------------------------------------------

// what every call that writes YUV frames refuses alike
static int check_yuv_out(lfi_ctx *ctx, const char *who, int matrix, int range)
{
    if(ctx->windowed)
        return fail(ctx, LFI_EINVAL, std::string(who) + ": YUV 4:2:0 frames need whole views: a 2x2 chroma block may straddle the row window's band");
    if((matrix != LFI_YUV_BT709 && matrix != LFI_YUV_BT601) || (range != LFI_YUV_LIMITED && range != LFI_YUV_FULL))
        return fail(ctx, LFI_EINVAL, std::string(who) + ": unknown YUV matrix (LFI_YUV_BT709, LFI_YUV_BT601) or range (LFI_YUV_LIMITED, LFI_YUV_FULL)");
    return LFI_OK;
}

// what lfi_download_views_yuv420 and lfi_download_views_yuv refuse alike, before they look at the frames
static int check_yuv_download(lfi_ctx *ctx, const char *who, int v0, int n, int matrix, int range)
{
    if(int rc = check_rendered(ctx))
        return rc;
    if(n < 1 || v0 < 0 || (long)v0 + n > ctx->views_n)
        return fail(ctx, LFI_EINVAL, std::string(who) + ": needs n >= 1 views starting at v0 inside [0, views)");
    return check_yuv_out(ctx, who, matrix, range);
}

// The ONE yuvs_convert launch, on st: view i of src → frame i of s (of `format`), n of them.  src starts on a 16-byte boundary (the views:
// hipMalloc, lfi_attach_views checks; the quilt buffer: hipMalloc) and a view is W·H·4 bytes, so with W a multiple of 4 every RGBA row
// does.  blocks_x is yuv_geometry's y_pitch / YUV_BLOCK_W: the same number.  siting: the context's out_siting (lfi_set_yuv_siting).
static hipError_t enqueue_yuv_convert(hipStream_t st, const lfi::ViewsSrc &src, bool planar, int n, int matrix, int range, int format, int siting,
                                      const lfi::YuvSurfaces &s)
{
    lfi::YuvsOutArgs a{};
    a.src = src, a.s = s;
    a.cw = (src.W + 1) >> 1, a.ch = (src.H + 1) >> 1;
    a.blocks_x = (src.W + lfi::YUV_BLOCK_W - 1) / lfi::YUV_BLOCK_W;
    a.rows16 = src.W % 4 == 0;
    if(yuv_bps(format) == 2) // I010 / P010: yuv10.hpp
    {
        a.k = lfi::YUV10_COEFFS[matrix * 2 + range];
        return lfi::launch_yuvs_convert10(st, planar, yuv_layout(format), siting == LFI_YUV_SITING_LEFT, a, n);
    }
    a.k = lfi::YUV_COEFFS[matrix * 2 + range];
    return lfi::launch_yuvs_convert(st, planar, format, siting == LFI_YUV_SITING_LEFT, a, n);
}

// How n frames of W × H reach dst, which has passed yuv_surfaces_fault (that gave extent) or is what host_i420_surfaces made: the kernel
// writes the caller's device surfaces in place, or staged frames in yuv[0] whose own bytes are then copied.  may_pack: a single host frame
// with tight rows that is not the staged frame (W no multiple of 8, or H odd) leaves through a packed device copy (yuv[1]): one contiguous
// copy per plane instead of one per row.
struct YuvDelivery
{
    lfi::YuvGeometry g;
    lfi::YuvSurfaces frames; // what the kernel writes
    bool in_place, packs;
};

// binds the device, checks a device surface, picks the route and reserves its buffers
static int open_yuv_delivery(lfi_ctx *ctx, const char *who, const lfi_yuv_surfaces &dst, size_t extent, int W, int H, int n, bool may_pack, YuvDelivery *d)
{
    if(int rc = bind(ctx))
        return rc;
    if(dst.memory == LFI_MEM_DEVICE)
        if(int rc = check_device_surfaces(ctx, who, dst, extent, n))
            return rc;
    d->g = lfi::yuv_geometry(W, H, yuv_bps(dst.format));
    d->in_place = yuv_surfaces_in_place(dst);
    d->packs = may_pack && !d->in_place && yuv_surfaces_packable(dst, d->g);
    if(!d->in_place)
        LFI_HIP(ctx, ctx->yuv[0].reserve(d->g.dev_frame_bytes * n));
    if(d->packs)
        LFI_HIP(ctx, ctx->yuv[1].reserve(d->g.frame_bytes));
    d->frames = d->in_place ? caller_surfaces(dst) : staged_surfaces(d->g, dst.format, ctx->yuv[0].get());
    return LFI_OK;
}

// behind the kernel on the context's stream: the copies of the staged frames (none in place), then the wait for them
static int finish_yuv_delivery(lfi_ctx *ctx, const lfi_yuv_surfaces &dst, int n, const YuvDelivery &d)
{
    if(!d.in_place)
        LFI_HIP(ctx, enqueue_surface_copies(ctx->stream, dst, 0, n, d.g, ctx->yuv[0].get(), false, d.packs ? ctx->yuv[1].get() : nullptr));
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LFI_OK;
}

// Behind both download calls.  The arguments have passed check_yuv_download
static int download_yuv_surfaces(lfi_ctx *ctx, const char *who, int v0, int n, int matrix, int range, const lfi_yuv_surfaces &dst, size_t extent)
{
    YuvDelivery d;
    if(int rc = open_yuv_delivery(ctx, who, dst, extent, ctx->width, ctx->height, n, false, &d))
        return rc;
    bool planar;
    const lfi::ViewsSrc src = rendered_views(ctx, v0, &planar);
    LFI_HIP(ctx, enqueue_yuv_convert(ctx->stream, src, planar, n, matrix, range, dst.format, ctx->yuv_out_siting, d.frames));
    return finish_yuv_delivery(ctx, dst, n, d);
}

// lfi_download_views_yuv with a LFI_YUV_DEEP format: frames from the DEEP planes of views [v0, v0 + n) (deep_yuv.hpp).  I010 / P010: the
// delivery of the 10-bit formats (in place, or staged frames and copies of their own bytes) around one deep_convert10 launch.  GBRP10: no
// arithmetic — the planes' upper six bits are 0 as deep_blend wrote them, so a frame is three 2D copies of 2·W bytes by H rows straight
// out of the deep planes (R, G, B there; G, B, R in the frame), to host or device memory alike: no kernel, no staging buffer
static int download_deep_surfaces(lfi_ctx *ctx, const char *who, int v0, int n, int matrix, int range, const lfi_yuv_surfaces &dst, size_t extent)
{
    if(!ctx->deep || v0 < ctx->deep_v0 || v0 + n > ctx->deep_v1)
        return fail(ctx, LFI_EINVAL, std::string(who) + ": a LFI_YUV_DEEP format needs views [v0, v0 + n) inside the range of the last deep render (LFI_FLAG_DEEP_VIEWS); "
                                         "a render without the flag drops the deep views");
    const size_t pitch = (size_t)deep_pitch(ctx), plane = pitch * ctx->out_rows;
    const uint8_t *src = ctx->deep.get() + (size_t)v0 * 3 * plane;
    if(dst.format == LFI_YUV_GBRP10)
    {
        if(int rc = bind(ctx))
            return rc;
        if(dst.memory == LFI_MEM_DEVICE)
            if(int rc = check_device_surfaces(ctx, who, dst, extent, n))
                return rc;
        const hipMemcpyKind kind = dst.memory == LFI_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        const size_t off[3] = {dst.cr_offset, 0, dst.c_offset}, dpitch[3] = {dst.c_pitch, dst.y_pitch, dst.c_pitch}; // where R, G, B go
        for(int k = 0; k < n; k++)
            for(int ch = 0; ch < 3; ch++)
                LFI_HIP(ctx, hipMemcpy2DAsync(static_cast<uint8_t *>(dst.base) + dst.frame_stride * (size_t)k + off[ch], dpitch[ch], src + ((size_t)k * 3 + ch) * plane,
                                              pitch, (size_t)ctx->width * 2, ctx->height, kind, ctx->stream));
        LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return LFI_OK;
    }
    YuvDelivery d;
    if(int rc = open_yuv_delivery(ctx, who, dst, extent, ctx->width, ctx->height, n, false, &d))
        return rc;
    lfi::DeepOutArgs a{};
    a.deep = src, a.view_stride = 3 * plane, a.pitch = (uint32_t)pitch;
    a.W = ctx->width, a.H = ctx->height;
    a.s = d.frames;
    a.cw = (a.W + 1) >> 1, a.ch = (a.H + 1) >> 1;
    a.blocks_x = (a.W + lfi::YUV_BLOCK_W - 1) / lfi::YUV_BLOCK_W;
    a.k = lfi::DEEP_COEFFS[matrix * 2 + range];
    LFI_HIP(ctx, lfi::launch_deep_convert10(ctx->stream, yuv_layout(dst.format), ctx->yuv_out_siting == LFI_YUV_SITING_LEFT, a, n));
    return finish_yuv_delivery(ctx, dst, n, d);
}

int lfi_download_views_yuv420(lfi_ctx *ctx, int v0, int n, int matrix, int range, uint8_t *out, size_t frame_stride_bytes)
{
    if(!ctx)
        return LFI_EINVAL;
    if(int rc = check_yuv_download(ctx, "lfi_download_views_yuv420", v0, n, matrix, range))
        return rc;
    lfi_yuv_surfaces dst{};
    if(int rc = host_i420_surfaces(ctx, "lfi_download_views_yuv420", out, frame_stride_bytes, &dst))
        return rc;
    return download_yuv_surfaces(ctx, "lfi_download_views_yuv420", v0, n, matrix, range, dst, 0);
}

int lfi_download_views_yuv(lfi_ctx *ctx, int v0, int n, int matrix, int range, const lfi_yuv_surfaces *dst)
{
    if(!ctx)
        return LFI_EINVAL;
    if(int rc = check_yuv_download(ctx, "lfi_download_views_yuv", v0, n, matrix, range))
        return rc;
    size_t extent = 0;
    if(const char *fault = yuv_surfaces_fault(dst, ctx->width, ctx->height, n, &extent, DEEP_SOURCE))
        return fail(ctx, LFI_EINVAL, std::string("lfi_download_views_yuv: ") + fault);
    if(dst->format & LFI_YUV_DEEP)
        return download_deep_surfaces(ctx, "lfi_download_views_yuv", v0, n, matrix, range, *dst, extent);
    return download_yuv_surfaces(ctx, "lfi_download_views_yuv", v0, n, matrix, range, *dst, extent);
}

// where lfi_render_stream_yuv420's frames go; NULL: lfi_render_stream's RGBA downloads
struct YuvSink
{
    lfi_yuv_surfaces frames; // host, I420, tight planes, the caller's stride
    int matrix, range;
};

static int render_stream(lfi_ctx *ctx, int method, int all_focus, const uint16_t *weights_fp16, int total_views, uint8_t *host_out, size_t pitch_bytes, const YuvSink *yuv);

int lfi_render_stream(lfi_ctx *ctx, int method, int all_focus, const uint16_t *weights_fp16, int total_views, uint8_t *host_out, size_t pitch_bytes)
{
    if(int rc = check_render_args(ctx, method, 0, 1))
        return rc;
    if(const ViewRowsKind rows = view_rows_of(ctx, all_focus))
        return fail(ctx, LFI_EINVAL, view_rows_set(rows) + "lfi_render_stream is not supported - clear them with NULL");
    if(ctx->flags & LFI_FLAG_LINEAR_LIGHT)
        return fail(ctx, LFI_EINVAL, "LFI_FLAG_LINEAR_LIGHT is set: lfi_render_stream is not supported");
    if(ctx->flags & LFI_FLAG_DEEP_VIEWS)
        return fail(ctx, LFI_EINVAL, "LFI_FLAG_DEEP_VIEWS is set: lfi_render_stream is not supported");
    if(ctx->flags & LFI_FLAG_IN_FRAME)
        return fail(ctx, LFI_EINVAL, "LFI_FLAG_IN_FRAME is set: lfi_render_stream is not supported");
    if(!weights_fp16 || total_views < 1)
        return fail(ctx, LFI_EINVAL, "lfi_render_stream: weights are NULL or total_views < 1");
    if(host_out && (ctx->out_layout != LFI_LAYOUT_RGBA || pitch_bytes < (size_t)ctx->width * 4))
        return fail(ctx, LFI_EINVAL, "lfi_render_stream: downloads need the RGBA view layout and a pitch of at least width*4 bytes");
    return render_stream(ctx, method, all_focus, weights_fp16, total_views, host_out, pitch_bytes, nullptr);
}

int lfi_render_stream_yuv420(lfi_ctx *ctx, int method, int all_focus, const uint16_t *weights_fp16, int total_views, int matrix, int range, uint8_t *host_out,
                             size_t frame_stride_bytes)
{
    if(int rc = check_render_args(ctx, method, 0, 1))
        return rc;
    if(const ViewRowsKind rows = view_rows_of(ctx, all_focus))
        return fail(ctx, LFI_EINVAL, view_rows_set(rows) + "lfi_render_stream_yuv420 is not supported - clear them with NULL");
    if(ctx->flags & LFI_FLAG_LINEAR_LIGHT)
        return fail(ctx, LFI_EINVAL, "LFI_FLAG_LINEAR_LIGHT is set: lfi_render_stream_yuv420 is not supported");
    if(ctx->flags & LFI_FLAG_DEEP_VIEWS)
        return fail(ctx, LFI_EINVAL, "LFI_FLAG_DEEP_VIEWS is set: lfi_render_stream_yuv420 is not supported");
    if(ctx->flags & LFI_FLAG_IN_FRAME)
        return fail(ctx, LFI_EINVAL, "LFI_FLAG_IN_FRAME is set: lfi_render_stream_yuv420 is not supported");
    if(!weights_fp16 || total_views < 1)
        return fail(ctx, LFI_EINVAL, "lfi_render_stream_yuv420: weights are NULL or total_views < 1");
    YuvSink sink{};
    sink.matrix = matrix, sink.range = range;
    if(int rc = check_yuv_out(ctx, "lfi_render_stream_yuv420", matrix, range))
        return rc;
    if(int rc = host_i420_surfaces(ctx, "lfi_render_stream_yuv420", host_out, frame_stride_bytes, &sink.frames))
        return rc;
    return render_stream(ctx, method, all_focus, weights_fp16, total_views, host_out, 0, &sink);
}

// The loop of both: block b's weights go up behind block b − 1's kernel, block b renders, and its result leaves on the copy stream while
// block b + 1 renders.  RGBA (yuv == NULL): the blocks alternate between two sets of views, each copied out as it is.  YUV: every block
// renders into the one set of views and is converted on the compute stream, in stream order before the next render overwrites it, into
// one of two buffers of frames; that buffer is what the copy stream reads.
static int render_stream(lfi_ctx *ctx, int method, int all_focus, const uint16_t *weights_fp16, int total_views, uint8_t *host_out, size_t pitch_bytes, const YuvSink *yuv)
{
    if(int rc = bind(ctx))
        return rc;
    const int V = ctx->views_n, n = ctx->n, k_pad = ctx->k_pad, v_pad = ctx->v_pad;
    const size_t wbytes = ctx->blob_weights_bytes;
    const lfi::YuvGeometry yuv_g = lfi::yuv_geometry(ctx->width, ctx->height);
    const size_t off_w16s = (sizeof(uint16_t) * (size_t)v_pad * k_pad + 15) / 16 * 16; // the layout lfi_set_params laid out
    const size_t off_w32 = (off_w16s + sizeof(uint16_t) * (size_t)v_pad * k_pad + 15) / 16 * 16;
    const size_t off_w32t = off_w32 + sizeof(float) * (size_t)v_pad * k_pad;
    for(int i = 0; i < 2; i++)
    {
        LFI_HIP(ctx, ctx->stream_staging[i].fit(wbytes));
        LFI_HIP(ctx, ctx->ev_h2d[i].ensure());
        LFI_HIP(ctx, ctx->ev_rendered[i].ensure());
        LFI_HIP(ctx, ctx->ev_d2h[i].ensure());
    }
    if(host_out)
    {
        if(int rc = ensure_copy_stream(ctx))
            return rc;
        if(yuv)
        {
            for(int i = 0; i < 2; i++)
                LFI_HIP(ctx, ctx->yuv[i].reserve(yuv_g.dev_frame_bytes * V));
        }
        else
            LFI_HIP(ctx, ctx->views2.fit(out_plane_bytes(ctx) * V));
    }
    if(int rc = join_uploads(ctx))
        return rc;
    const int n_blocks = (total_views + V - 1) / V;
    uint8_t *dev_weights = param_base(ctx) + ctx->blob_off_w16;
    uint8_t *const vbuf[2] = {ctx->views.get(), host_out && !yuv ? ctx->views2.get() : ctx->views.get()};
    int status = LFI_OK;
    for(int b = 0; b < n_blocks && status == LFI_OK; b++)
    {
        const int slot = b & 1;
        const int nv = std::min(V, total_views - b * V);
        // the staging slot is free once the copy of block b − 2 out of it has been executed
        if(b >= 2)
            LFI_HIP(ctx, hipEventSynchronize(ctx->ev_h2d[slot]));
        std::memset(ctx->stream_staging[slot].get(), 0, wbytes);
        bool scalable = true, sums_ok = true;
        fill_weight_arrays(weights_fp16 + (size_t)b * V * n, nv, n, k_pad, v_pad, ctx->stream_staging[slot].get(), off_w16s, off_w32, off_w32t, &scalable, &sums_ok);
        ctx->weights_scalable = scalable; // the dispatch of THIS block's launch (read at enqueue time)
        ctx->weights_sum_ok = sums_ok;
        // stream order protects the device arrays: the previous block's kernel is ahead of this copy on the same stream
        LFI_HIP(ctx, hipMemcpyAsync(dev_weights, ctx->stream_staging[slot].get(), wbytes, hipMemcpyHostToDevice, ctx->stream));
        LFI_HIP(ctx, hipEventRecord(ctx->ev_h2d[slot], ctx->stream));
        if(host_out && !yuv && b >= 2)
            LFI_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_d2h[slot], 0)); // block b − 2 has left this set of views
        KernelArgs a = make_args(ctx, 0, nv, method);
        a.views = vbuf[slot];
        status = launch_blend(ctx, method, all_focus, a);
        if(status != LFI_OK || !host_out)
            continue;
        if(yuv)
        {
            if(b >= 2)
                LFI_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_d2h[slot], 0)); // block b − 2 has left this buffer of frames
            bool planar;
            const lfi::ViewsSrc src = rendered_views(ctx, 0, &planar); // vbuf[slot]: YUV blocks all render into the one set of views
            LFI_HIP(ctx, enqueue_yuv_convert(ctx->stream, src, planar, nv, yuv->matrix, yuv->range, LFI_YUV_I420, ctx->yuv_out_siting,
                                             staged_surfaces(yuv_g, LFI_YUV_I420, ctx->yuv[slot].get())));
        }
        LFI_HIP(ctx, hipEventRecord(ctx->ev_rendered[slot], ctx->stream));
        LFI_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_rendered[slot], 0));
        if(yuv)
        {
            LFI_HIP(ctx, enqueue_surface_copies(ctx->copy_stream, yuv->frames, b * V, nv, yuv_g, ctx->yuv[slot].get(), false));
            LFI_HIP(ctx, hipEventRecord(ctx->ev_d2h[slot], ctx->copy_stream));
            continue;
        }
        const size_t view_bytes = pitch_bytes * ctx->height;
        for(int v = 0; v < nv; v++)
            LFI_HIP(ctx, hipMemcpy2DAsync(host_out + ((size_t)b * V + v) * view_bytes + (size_t)ctx->out_y0 * pitch_bytes, pitch_bytes,
                                          vbuf[slot] + out_plane_bytes(ctx) * v, (size_t)ctx->width * 4, (size_t)ctx->width * 4, ctx->out_rows,
                                          hipMemcpyDeviceToHost, ctx->copy_stream));
        LFI_HIP(ctx, hipEventRecord(ctx->ev_d2h[slot], ctx->copy_stream));
    }
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if(host_out)
        LFI_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));
    return status;
}

int lfi_keep_views(lfi_ctx *ctx, int v0, int n)
{
    if(!ctx)
        return LFI_EINVAL;
    if(n == 0)
    {
        if(int rc = bind(ctx))
            return rc;
        drop_kept(ctx); // hipFree waits for a copy into the set that is still in flight
        return LFI_OK;
    }
    if(int rc = check_rendered(ctx))
        return rc;
    if(v0 < 0 || n < 0 || (long)v0 + n > ctx->views_n)
        return fail(ctx, LFI_EINVAL, "lfi_keep_views: views [v0, v0 + n) must lie inside [0, views)");
    if(int rc = bind(ctx))
        return rc;
    // Views are written on the stream in use only (renders, the planar conversion, poison), never on the copy or the side stream: the copy
    // below needs no join with pending uploads or the focus map's filter.  With a row window the band's rows are kept, as the views hold them
    // (lfi_compare_views refuses windows; lfi_set_row_window drops the set).
    const size_t stride = out_plane_bytes(ctx), bytes = stride * n;
    ctx->kept_v0 = ctx->kept_n = 0;
    LFI_HIP(ctx, ctx->kept.fit(bytes)); // another size: the old set is freed (compares are synchronous: nothing reads it any more)
    // behind the renders already enqueued, in front of the later ones: the views as they are at this point of the stream
    LFI_HIP(ctx, hipMemcpyAsync(ctx->kept.get(), ctx->views.get() + (size_t)v0 * stride, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    ctx->kept_v0 = v0;
    ctx->kept_n = n;
    return LFI_OK;
}

namespace {

constexpr size_t COMPARE_CHUNK_BYTES = (size_t)64 << 20; // host references cross PCIe in chunks of at most this many bytes (at least one image)

double psnr_of(double mse)
{
    return mse > 0 ? 10.0 * std::log10(255.0 * 255.0 / mse) : INFINITY;
}

// psnr, psnr_all and ssim_all from mse[] and ssim[]
void finish_quality(lfi_quality *q)
{
    double mse_all = 0, ssim_all = 0;
    for(int c = 0; c < 3; c++)
    {
        q->psnr[c] = psnr_of(q->mse[c]);
        mse_all += q->mse[c] / 3.0;
        ssim_all += q->ssim[c] / 3.0;
    }
    q->psnr_all = psnr_of(mse_all);
    q->ssim_all = ssim_all;
}

// Behind lfi_compare_views and lfi_compare_view, whose checks the arguments have passed: views [v0, v0 + n) against host references, or
// (references_rgba NULL) against the kept views
int run_compare_views(lfi_ctx *ctx, int v0, int n, const uint8_t *references_rgba, size_t pitch_bytes, size_t image_stride_bytes, lfi_view_quality *out,
                      lfi_quality *out_all)
{
    const int W = ctx->width, H = ctx->height;
    if(int rc = bind(ctx))
        return rc;
    if(int rc = join_uploads(ctx))
        return rc;
    // n <= views <= 4096 (lfi_set_params): the launch grid's z dimension stays far below its limit of 65535
    const int tiles = lfi::quality_tiles_x(W) * lfi::quality_tiles_y(H);
    const size_t records_bytes = sizeof(lfi::QualityViewSums) * (size_t)n;
    LFI_HIP(ctx, ctx->cmp_ws.reserve(records_bytes + sizeof(lfi::QualityPartial) * (size_t)n * tiles));
    lfi::QualityViewSums *const d_records = ctx->cmp_ws.as<lfi::QualityViewSums>();
    lfi::QualityPartial *const d_partials = reinterpret_cast<lfi::QualityPartial *>(ctx->cmp_ws.get() + records_bytes);
    bool planar;
    const lfi::ViewsSrc views = rendered_views(ctx, v0, &planar);
    const size_t stride = views.view_stride;
    const uint32_t view_row = planar ? views.pitch : (uint32_t)W * 4u;
    const lfi::QualityImages a{views.base, stride, view_row};
    if(!references_rgba)
    {
        // kept views, in the views' layout: one launch for all n
        const lfi::QualityImages b{ctx->kept.get() + (size_t)(v0 - ctx->kept_v0) * stride, stride, view_row};
        LFI_HIP(ctx, lfi::launch_quality_tiles(ctx->stream, planar, planar, a, b, W, H, n, d_partials));
    }
    else
    {
        // chunks of `per` images through two staging buffers: the copy of chunk k + 1 (copy stream) runs beside the reduction of chunk k
        const size_t image = plane_bytes(ctx), row = (size_t)W * 4;
        const int per = (int)std::min<size_t>((size_t)n, std::max<size_t>(COMPARE_CHUNK_BYTES / image, 1));
        if(int rc = ensure_copy_stream(ctx))
            return rc;
        for(int i = 0; i < 2; i++)
        {
            LFI_HIP(ctx, ctx->ev_cmp_copied[i].ensure());
            LFI_HIP(ctx, ctx->ev_cmp_reduced[i].ensure());
            if(i == 0 || per < n)
                LFI_HIP(ctx, ctx->cmp_stage[i].reserve(image * per));
        }
        // the staging buffers are written on the copy stream: behind whatever the stream in use still has queued for them (a reserve's
        // predecessor is gone, but lfi_debug_poison fills them in stream order) — one event, no host wait
        LFI_HIP(ctx, hipEventRecord(ctx->ev_cmp_reduced[0], ctx->stream));
        LFI_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_cmp_reduced[0], 0));
        for(int c0 = 0, k = 0; c0 < n; c0 += per, k++)
        {
            const int slot = k & 1, cnt = std::min(per, n - c0);
            if(k >= 2) // the buffer is free again once the chunk before last has been reduced
                LFI_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_cmp_reduced[slot], 0));
            const uint8_t *src = references_rgba + (size_t)c0 * image_stride_bytes;
            if(image_stride_bytes == pitch_bytes * H) // the images' rows follow each other: one copy for the chunk
                LFI_HIP(ctx, hipMemcpy2DAsync(ctx->cmp_stage[slot].get(), row, src, pitch_bytes, row, (size_t)cnt * H, hipMemcpyHostToDevice, ctx->copy_stream));
            else
                for(int i = 0; i < cnt; i++)
                    LFI_HIP(ctx, hipMemcpy2DAsync(ctx->cmp_stage[slot].get() + (size_t)i * image, row, src + (size_t)i * image_stride_bytes, pitch_bytes, row, H,
                                                  hipMemcpyHostToDevice, ctx->copy_stream));
            LFI_HIP(ctx, hipEventRecord(ctx->ev_cmp_copied[slot], ctx->copy_stream));
            LFI_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_cmp_copied[slot], 0));
            const lfi::QualityImages ac{a.base + (size_t)c0 * stride, stride, view_row};
            const lfi::QualityImages b{ctx->cmp_stage[slot].get(), image, (uint32_t)row};
            LFI_HIP(ctx, lfi::launch_quality_tiles(ctx->stream, planar, false, ac, b, W, H, cnt, d_partials + (size_t)c0 * tiles));
            LFI_HIP(ctx, hipEventRecord(ctx->ev_cmp_reduced[slot], ctx->stream));
        }
    }
    hipLaunchKernelGGL(lfi::quality_views, dim3(n), dim3(256), 0, ctx->stream, d_partials, tiles, d_records);
    LFI_HIP(ctx, hipGetLastError());
    std::vector<lfi::QualityViewSums> sums(n);
    LFI_HIP(ctx, hipMemcpyAsync(sums.data(), d_records, records_bytes, hipMemcpyDeviceToHost, ctx->stream));
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));

    const double px = (double)W * H;
    unsigned long long total[3] = {0ull, 0ull, 0ull};
    double ssim_views[3] = {0.0, 0.0, 0.0};
    for(int k = 0; k < n; k++)
    {
        const lfi::QualityViewSums &s = sums[k];
        lfi_view_quality &o = out[k];
        std::memset(&o, 0, sizeof(o)); // padding included: equal results are equal bytes
        for(int c = 0; c < 3; c++)
        {
            o.sq_err[c] = s.sq_err[c];
            o.q.mse[c] = (double)s.sq_err[c] / px;
            o.q.ssim[c] = s.windows ? s.ssim[c] / (double)s.windows : 1.0;
            total[c] += s.sq_err[c];
            ssim_views[c] += o.q.ssim[c];
        }
        finish_quality(&o.q);
        o.differing_bytes = s.differing;
        o.windows = s.windows;
        o.max_abs_diff = s.max_abs_diff;
    }
    if(out_all)
    {
        std::memset(out_all, 0, sizeof(*out_all));
        for(int c = 0; c < 3; c++)
        {
            out_all->mse[c] = (double)total[c] / (double)((unsigned long long)n * (unsigned long long)W * (unsigned long long)H);
            out_all->ssim[c] = ssim_views[c] / (double)n;
        }
        finish_quality(out_all);
    }
    return LFI_OK;
}

} // namespace

int lfi_compare_views(lfi_ctx *ctx, int v0, int n, const uint8_t *references_rgba, size_t pitch_bytes, size_t image_stride_bytes, lfi_view_quality *out,
                      lfi_quality *out_all)
{
    if(!ctx)
        return LFI_EINVAL;
    if(!out)
        return fail(ctx, LFI_EINVAL, "lfi_compare_views: out is NULL");
    if(int rc = check_rendered(ctx))
        return rc;
    if(ctx->windowed)
        return fail(ctx, LFI_EINVAL, "lfi_compare_views needs whole views (no row window)");
    if(v0 < 0 || n < 1 || (long)v0 + n > ctx->views_n)
        return fail(ctx, LFI_EINVAL, "lfi_compare_views: views [v0, v0 + n), n >= 1, must lie inside [0, views)");
    if(references_rgba)
    {
        if(pitch_bytes < (size_t)ctx->width * 4 || image_stride_bytes / (size_t)ctx->height < pitch_bytes)
            return fail(ctx, LFI_EINVAL, "lfi_compare_views: bad pitch (>= width * 4) or image stride (>= pitch * height)");
    }
    else if(!ctx->kept)
        return fail(ctx, LFI_EINVAL, "lfi_compare_views: no reference images and no kept views (lfi_keep_views)");
    else if(v0 < ctx->kept_v0 || v0 + n > ctx->kept_v0 + ctx->kept_n)
        return fail(ctx, LFI_EINVAL, "lfi_compare_views: the kept views do not cover [v0, v0 + n)");
    return run_compare_views(ctx, v0, n, references_rgba, pitch_bytes, image_stride_bytes, out, out_all);
}

// lfi_compare_views' code for one view and one host reference whose rows follow each other: the same sums, in the same order
int lfi_compare_view(lfi_ctx *ctx, int v, const uint8_t *reference_rgba, size_t pitch_bytes, lfi_quality *out)
{
    if(!ctx || !out)
        return LFI_EINVAL;
    if(int rc = check_rendered(ctx))
        return rc;
    if(v < 0 || v >= ctx->views_n || !reference_rgba || pitch_bytes < (size_t)ctx->width * 4)
        return fail(ctx, LFI_EINVAL, "bad view index, pointer or pitch");
    if(ctx->windowed)
        return fail(ctx, LFI_EINVAL, "lfi_compare_view needs the whole view (no row window)");
    lfi_view_quality one;
    if(int rc = run_compare_views(ctx, v, 1, reference_rgba, pitch_bytes, pitch_bytes * ctx->height, &one, nullptr))
        return rc;
    *out = one.q;
    return LFI_OK;
}

int lfi_sync(lfi_ctx *ctx)
{
    if(!ctx)
        return LFI_EINVAL;
    if(int rc = bind(ctx))
        return rc;
    if(int rc = join_uploads(ctx))
        return rc;
    if(int rc = join_filter(ctx))
        return rc;
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LFI_OK;
}

int lfi_timer_start(lfi_ctx *ctx)
{
    if(!ctx)
        return LFI_EINVAL;
    if(int rc = bind(ctx))
        return rc;
    LFI_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    return LFI_OK;
}

int lfi_timer_stop(lfi_ctx *ctx, float *out_ms)
{
    if(!ctx || !out_ms)
        return LFI_EINVAL;
    if(int rc = bind(ctx))
        return rc;
    if(int rc = join_filter(ctx)) // a timed region ends when ALL its work has: the side stream's filter included
        return rc;
    LFI_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    LFI_HIP(ctx, hipEventSynchronize(ctx->ev1));
    LFI_HIP(ctx, hipEventElapsedTime(out_ms, ctx->ev0, ctx->ev1));
    return LFI_OK;
}

int lfi_benchmark(lfi_ctx *ctx, int method, int all_focus, int v0, int v1, int warmup, int runs, lfi_bench_stats *out)
{
    if(int rc = check_render_args(ctx, method, v0, v1))
        return rc;
    if(!out || runs < 1 || warmup < 0)
        return fail(ctx, LFI_EINVAL, "lfi_benchmark: runs must be ≥ 1 and out_stats non-NULL");
    if(int rc = bind(ctx))
        return rc;
    const KernelArgs a = make_args(ctx, v0, v1, method);
    // the derived input copy is (re)built here, not inside the first timed launch — and so are the deep planes allocated (LFI_FLAG_DEEP_VIEWS)
    bool planar = false;
    if(ctx->flags & LFI_FLAG_LINEAR_LIGHT)
    {
        if(int rc = flagged_refused(ctx, LFI_FLAG_LINEAR_LIGHT, all_focus, a))
            return rc;
        (void)ensure_planar(ctx, true);
    }
    else if(ctx->flags & LFI_FLAG_IN_FRAME)
    {
        if(int rc = flagged_refused(ctx, LFI_FLAG_IN_FRAME, all_focus, a))
            return rc;
        (void)ensure_planar(ctx, true);
    }
    else if(ctx->flags & LFI_FLAG_DEEP_VIEWS)
    {
        if(int rc = flagged_refused(ctx, LFI_FLAG_DEEP_VIEWS, all_focus, a))
            return rc;
        (void)ensure_planar(ctx, true);
        if(int rc = ensure_deep_planes(ctx))
            return rc;
    }
    else if(const ViewRowsKind rows = view_rows_of(ctx, all_focus))
    {
        if(int rc = view_rows_ready(ctx, rows, all_focus, a, &planar))
            return rc;
    }
    else if(route_blend(ctx, method, all_focus != 0, a, true).reads_copy)
        (void)ensure_planar(ctx, true);
    for(int i = 0; i < warmup; i++)
        if(int rc = launch_blend(ctx, method, all_focus, a))
            return rc;
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<float> t(runs);
    for(int i = 0; i < runs; i++)
    {
        LFI_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        if(int rc = launch_blend(ctx, method, all_focus, a))
            return rc;
        LFI_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        LFI_HIP(ctx, hipEventSynchronize(ctx->ev1));
        LFI_HIP(ctx, hipEventElapsedTime(&t[i], ctx->ev0, ctx->ev1));
    }
    float b2b = 0;
    LFI_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    for(int i = 0; i < runs; i++)
        if(int rc = launch_blend(ctx, method, all_focus, a))
            return rc;
    LFI_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    LFI_HIP(ctx, hipEventSynchronize(ctx->ev1));
    LFI_HIP(ctx, hipEventElapsedTime(&b2b, ctx->ev0, ctx->ev1));
    std::vector<float> s = t;
    std::sort(s.begin(), s.end());
    double sum = 0;
    for(float x : t)
        sum += x;
    out->runs = runs;
    out->mean_ms = float(sum / runs);
    out->median_ms = (runs & 1) ? s[runs / 2] : 0.5f * (s[runs / 2 - 1] + s[runs / 2]);
    out->min_ms = s.front();
    out->max_ms = s.back();
    out->back_to_back_ms = b2b / runs;
    return LFI_OK;
}

// ONE quilt_assemble launch on the context's stream: views v0 … v0 + n − 1 of src → tiles first … first + n − 1 of `quilt`
static hipError_t enqueue_quilt_assemble(lfi_ctx *ctx, const lfi::ViewsSrc &src, bool planar, uint32_t *quilt, int n, int v0, int first, int tiles_x)
{
    const dim3 grid(((src.W + 3) / 4 + 255) / 256, src.H, n), block(256);
    if(planar)
        hipLaunchKernelGGL(lfi::quilt_assemble<true>, grid, block, 0, ctx->stream, src, quilt, v0, first, tiles_x);
    else
        hipLaunchKernelGGL(lfi::quilt_assemble<false>, grid, block, 0, ctx->stream, src, quilt, v0, first, tiles_x);
    return hipGetLastError();
}

int lfi_download_view(lfi_ctx *ctx, int v, uint8_t *rgba, size_t pitch_bytes)
{
    if(!ctx)
        return LFI_EINVAL;
    if(int rc = check_rendered(ctx))
        return rc;
    if(v < 0 || v >= ctx->views_n || !rgba || pitch_bytes < (size_t)ctx->width * 4)
        return fail(ctx, LFI_EINVAL, "bad view index, pointer or pitch");
    if(int rc = bind(ctx))
        return rc;
    // the view as an RGBA plane of out_rows rows: the view itself, or (planar layout) its expansion into the context's one-plane staging
    // buffer — the one tile of a quilt one tile wide
    bool planar;
    const lfi::ViewsSrc view = rendered_views(ctx, v, &planar);
    const uint8_t *src = view.base;
    if(planar)
    {
        LFI_HIP(ctx, ctx->dl_plane.fit(rgba_out_plane_bytes(ctx)));
        LFI_HIP(ctx, enqueue_quilt_assemble(ctx, view, true, ctx->dl_plane.as<uint32_t>(), 1, 0, 0, 1));
        src = ctx->dl_plane.get();
    }
    // rgba addresses row 0 of the whole view; the rows this context rendered are written at their place
    LFI_HIP(ctx, hipMemcpy2DAsync(rgba + (size_t)ctx->out_y0 * pitch_bytes, pitch_bytes, src,
                                  (size_t)ctx->width * 4, (size_t)ctx->width * 4, ctx->out_rows, hipMemcpyDeviceToHost, ctx->stream));
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LFI_OK;
}

int lfi_download_map(lfi_ctx *ctx, int k, uint8_t *rgba, size_t pitch_bytes)
{
    if(!ctx)
        return LFI_EINVAL;
    if(!ctx->maps)
        return fail(ctx, LFI_EINVAL, "lfi_set_grid has not been called");
    if(k < 0 || k > 1 || !rgba || pitch_bytes < (size_t)ctx->width * 4)
        return fail(ctx, LFI_EINVAL, "bad map index, pointer or pitch");
    if(int rc = bind(ctx))
        return rc;
    if(int rc = join_filter(ctx))
        return rc;
    LFI_HIP(ctx, hipMemcpy2DAsync(rgba, pitch_bytes, ctx->maps.get() + plane_bytes(ctx) * k, (size_t)ctx->width * 4,
                                  (size_t)ctx->width * 4, ctx->height, hipMemcpyDeviceToHost, ctx->stream));
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LFI_OK;
}

// the tiles and views the two quilt calls refuse alike
static int check_quilt_tiles(lfi_ctx *ctx, int tiles_x, int tiles_y, int first_tile, int n, int v0)
{
    if(tiles_x < 1 || tiles_y < 1 || first_tile < 0 || n < 1 || (long)first_tile + n > (long)tiles_x * tiles_y || v0 < 0 || (long)v0 + n > ctx->views_n)
        return fail(ctx, LFI_EINVAL, "quilt needs the tiles inside the quilt and as many views starting at v0 inside [0, views)");
    return LFI_OK;
}

// the tile sizes and view spans the scaled quilt and the native image refuse alike
static int check_scaled_tiles(lfi_ctx *ctx, int tile_w, int tile_h)
{
    if(tile_w < 1 || tile_w > ctx->width || tile_h < 1 || tile_h > ctx->height)
        return fail(ctx, LFI_EINVAL, "scaled quilt tiles are 1 … width by 1 … height pixels (downscaling or identity only)");
    if((uint32_t)ctx->width > lfi::LFI_AREA_SPAN_MAX || (uint32_t)ctx->height > lfi::LFI_AREA_SPAN_MAX)
        return fail(ctx, LFI_EINVAL, "scaled quilts take views of up to 65535 pixels per axis");
    return LFI_OK;
}

// what lfi_download_quilt_tiles_scaled and lfi_download_quilt_yuv refuse alike before they look at the destination
static int check_scaled_quilt(lfi_ctx *ctx, int tiles_x, int tiles_y, int first_tile, int n, int v0, int tile_w, int tile_h)
{
    if(int rc = check_rendered(ctx))
        return rc;
    if(ctx->windowed)
        return fail(ctx, LFI_EINVAL, "a scaled quilt needs whole views: a tile's rows average source rows the row window's band does not hold");
    if(int rc = check_quilt_tiles(ctx, tiles_x, tiles_y, first_tile, n, v0))
        return rc;
    return check_scaled_tiles(ctx, tile_w, tile_h);
}

// Tiles [first, first + n) of a quilt tiles_x tiles wide → the host image, on the compute stream.  The quilt buffer holds the rows of tiles
// they touch, from row first / tiles_x on, a tile tile_bytes wide and dev_rows high; in the host image a tile is host_rows high and the
// device's rows are its rows from host_y0 on (a row window: only the band's rows of every tile exist).  One rectangle — or three when the
// first / last row of tiles is only partly this context's (a trajectory sharded over several GPUs: every context fills its own tiles of
// the same host image).
static hipError_t enqueue_quilt_copies(lfi_ctx *ctx, int tiles_x, int first, int n, size_t tile_bytes, int dev_rows, int host_rows, int host_y0, uint8_t *rgba,
                                       size_t pitch_bytes)
{
    const int tr0 = first / tiles_x, tr1 = (first + n - 1) / tiles_x, c_first = first % tiles_x, c_last = (first + n - 1) % tiles_x;
    const size_t qrow = tiles_x * tile_bytes;
    // rows of tiles [ra, rb] × tile columns [ca, cb]
    auto copy_rect = [&](int ra, int rb, int ca, int cb) -> hipError_t {
        // dev_rows == host_rows: the tiles' rows are contiguous in the host image too, one copy for all rows of tiles
        const int step = dev_rows == host_rows ? rb - ra + 1 : 1;
        for(int r = ra; r <= rb; r += step)
        {
            const hipError_t e = hipMemcpy2DAsync(rgba + ((size_t)r * host_rows + host_y0) * pitch_bytes + ca * tile_bytes, pitch_bytes,
                                                  ctx->quilt.get() + (size_t)(r - tr0) * dev_rows * qrow + ca * tile_bytes, qrow, (cb - ca + 1) * tile_bytes,
                                                  (size_t)step * dev_rows, hipMemcpyDeviceToHost, ctx->stream);
            if(e != hipSuccess)
                return e;
        }
        return hipSuccess;
    };
    if(tr0 == tr1)
        return copy_rect(tr0, tr0, c_first, c_last);
    // a partly filled first row of tiles, a partly filled last one, the whole rows between them
    const int full0 = c_first != 0 ? tr0 + 1 : tr0, full1 = c_last != tiles_x - 1 ? tr1 - 1 : tr1;
    hipError_t e = hipSuccess;
    if(full0 != tr0)
        e = copy_rect(tr0, tr0, c_first, tiles_x - 1);
    if(e == hipSuccess && full1 != tr1)
        e = copy_rect(tr1, tr1, 0, c_last);
    if(e == hipSuccess && full0 <= full1)
        e = copy_rect(full0, full1, 0, tiles_x - 1);
    return e;
}

int lfi_download_quilt_tiles(lfi_ctx *ctx, int tiles_x, int tiles_y, int first_tile, int n, int v0, uint8_t *rgba, size_t pitch_bytes)
{
    if(!ctx)
        return LFI_EINVAL;
    if(int rc = check_rendered(ctx))
        return rc;
    if(int rc = check_quilt_tiles(ctx, tiles_x, tiles_y, first_tile, n, v0))
        return rc;
    if(!rgba || pitch_bytes < (size_t)tiles_x * ctx->width * 4)
        return fail(ctx, LFI_EINVAL, "bad quilt pointer or pitch");
    if(int rc = bind(ctx))
        return rc;
    // The rows of tiles these tiles touch, assembled on the device by ONE kernel (planar views are expanded on the fly: no per-view
    // conversion pass), then copied to the host (enqueue_quilt_copies).
    const int tr0 = first_tile / tiles_x, tr1 = (first_tile + n - 1) / tiles_x;
    const int W = ctx->width, rows = ctx->out_rows;
    const size_t qrow = (size_t)tiles_x * W * 4;
    const size_t need = qrow * rows * (size_t)(tr1 - tr0 + 1);
    LFI_HIP(ctx, ctx->quilt.reserve(need));
    bool planar;
    const lfi::ViewsSrc views = rendered_views(ctx, 0, &planar);
    LFI_HIP(ctx, enqueue_quilt_assemble(ctx, views, planar, ctx->quilt.as<uint32_t>(), n, v0, first_tile, tiles_x));
    LFI_HIP(ctx, enqueue_quilt_copies(ctx, tiles_x, first_tile, n, (size_t)W * 4, rows, ctx->height, ctx->out_y0, rgba, pitch_bytes));
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LFI_OK;
}

int lfi_download_quilt(lfi_ctx *ctx, int tiles_x, int tiles_y, int v0, uint8_t *rgba, size_t pitch_bytes)
{
    if(ctx && (tiles_x < 1 || tiles_y < 1))
        return fail(ctx, LFI_EINVAL, "quilt needs tiles_x*tiles_y views starting at v0 inside [0, views)");
    return lfi_download_quilt_tiles(ctx, tiles_x, tiles_y, 0, tiles_x * tiles_y, v0, rgba, pitch_bytes);
}

int lfi_download_quilt_tiles_scaled(lfi_ctx *ctx, int tiles_x, int tiles_y, int first_tile, int n, int v0, int tile_w, int tile_h, uint8_t *rgba, size_t pitch_bytes)
{
    if(!ctx)
        return LFI_EINVAL;
    if(int rc = check_scaled_quilt(ctx, tiles_x, tiles_y, first_tile, n, v0, tile_w, tile_h))
        return rc;
    if(!rgba || pitch_bytes < (size_t)tiles_x * tile_w * 4)
        return fail(ctx, LFI_EINVAL, "bad quilt pointer or pitch");
    if(int rc = bind(ctx))
        return rc;
    // As lfi_download_quilt_tiles: the rows of tiles these tiles touch are made on the device by ONE kernel, in the same buffer, and only
    // their bytes — tile_w × tile_h per tile — are copied.
    const int tr0 = first_tile / tiles_x, tr1 = (first_tile + n - 1) / tiles_x;
    const size_t qrow = (size_t)tiles_x * tile_w * 4;
    LFI_HIP(ctx, ctx->quilt.reserve(qrow * tile_h * (size_t)(tr1 - tr0 + 1)));
    bool planar;
    lfi::QuiltScaleArgs q{};
    q.src = rendered_views(ctx, 0, &planar);
    q.quilt = ctx->quilt.as<uint32_t>();
    q.tile_w = tile_w, q.tile_h = tile_h;
    q.v0 = v0, q.first = first_tile, q.tiles_x = tiles_x;
    LFI_HIP(ctx, lfi::launch_quilt_scale(ctx->stream, planar, q, n));
    LFI_HIP(ctx, enqueue_quilt_copies(ctx, tiles_x, first_tile, n, (size_t)tile_w * 4, tile_h, tile_h, 0, rgba, pitch_bytes));
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LFI_OK;
}

int lfi_download_quilt_scaled(lfi_ctx *ctx, int tiles_x, int tiles_y, int v0, int tile_w, int tile_h, uint8_t *rgba, size_t pitch_bytes)
{
    if(ctx && (tiles_x < 1 || tiles_y < 1))
        return fail(ctx, LFI_EINVAL, "quilt needs tiles_x*tiles_y views starting at v0 inside [0, views)");
    return lfi_download_quilt_tiles_scaled(ctx, tiles_x, tiles_y, 0, tiles_x * tiles_y, v0, tile_w, tile_h, rgba, pitch_bytes);
}

int lfi_download_quilt_yuv(lfi_ctx *ctx, int tiles_x, int tiles_y, int v0, int tile_w, int tile_h, int matrix, int range, const lfi_yuv_surfaces *dst)
{
    static const char *who = "lfi_download_quilt_yuv";
    if(!ctx)
        return LFI_EINVAL;
    // what lfi_download_quilt_scaled refuses, in its words and order (n = 0, which the check refuses, where the product is no count of tiles)
    const long tiles = (long)tiles_x * tiles_y;
    const int n = tiles_x >= 1 && tiles_y >= 1 && tiles <= INT32_MAX ? (int)tiles : 0;
    if(int rc = check_scaled_quilt(ctx, tiles_x, tiles_y, 0, n, v0, tile_w, tile_h))
        return rc;
    if(int rc = check_yuv_out(ctx, who, matrix, range))
        return rc;
    if((long)tiles_x * tile_w > INT32_MAX || (long)tiles_y * tile_h > INT32_MAX)
        return fail(ctx, LFI_EINVAL, std::string(who) + ": the frame is more than 2^31 - 1 pixels wide or high");
    const int QW = tiles_x * tile_w, QH = tiles_y * tile_h;
    size_t extent = 0;
    if(const char *fault = yuv_surfaces_fault(dst, QW, QH, 1, &extent))
        return fail(ctx, LFI_EINVAL, std::string(who) + ": " + fault);
    // the caller's frame in place, or the staged frame and the copies of its own bytes; a host frame may pack
    YuvDelivery d;
    if(int rc = open_yuv_delivery(ctx, who, *dst, extent, QW, QH, 1, true, &d))
        return rc;
    bool planar;
    lfi::QuiltScaleArgs q{};
    q.src = rendered_views(ctx, 0, &planar);
    q.tile_w = tile_w, q.tile_h = tile_h;
    q.v0 = v0, q.first = 0, q.tiles_x = tiles_x;
    if(tile_w % 2 == 0 && tile_h % 2 == 0 && ctx->yuv_out_siting == LFI_YUV_SITING_CENTRE && yuv_bps(dst->format) == 1)
    {
        // centre-sited, every 2 x 2 block lies inside one tile: ONE launch, no RGBA quilt
        lfi::QuiltYuvArgs a{};
        a.q = q, a.s = d.frames, a.k = lfi::YUV_COEFFS[matrix * 2 + range];
        LFI_HIP(ctx, lfi::launch_quilt_yuv_scale(ctx->stream, planar, dst->format, a, n));
    }
    else
    {
        // blocks straddle tiles, or (left-sited) the chroma filter reaches across tile edges, or the frame is 10-bit (no fused kernel): the RGBA quilt of lfi_download_quilt_scaled in the quilt buffer, converted as ONE RGBA view of QW x QH
        const size_t quilt_bytes = (size_t)QW * 4 * QH;
        LFI_HIP(ctx, ctx->quilt.reserve(quilt_bytes));
        q.quilt = ctx->quilt.as<uint32_t>();
        LFI_HIP(ctx, lfi::launch_quilt_scale(ctx->stream, planar, q, n));
        const lfi::ViewsSrc quilt{ctx->quilt.get(), quilt_bytes, (uint32_t)QW, (uint32_t)QH, 0u};
        LFI_HIP(ctx, enqueue_yuv_convert(ctx->stream, quilt, false, 1, matrix, range, dst->format, ctx->yuv_out_siting, d.frames));
    }
    return finish_yuv_delivery(ctx, *dst, 1, d);
}

int lfi_download_rgbd_yuv(lfi_ctx *ctx, int v0, int n, int map_k, uint32_t flags, int tile_w, int tile_h, int matrix, int range, const lfi_yuv_surfaces *dst)
{
    static const char *who = "lfi_download_rgbd_yuv";
    if(!ctx)
        return LFI_EINVAL;
    // the views and the coefficient set as lfi_download_views_yuv refuses them (nothing rendered, the range of views, a row window, matrix
    // and range), the tiles as lfi_download_quilt_scaled does
    if(int rc = check_yuv_download(ctx, who, v0, n, matrix, range))
        return rc;
    if(dst && yuv_format_deep(dst->format))
        return fail(ctx, LFI_EINVAL, std::string(who) + ": " + kDeepFormatRefused);
    if(dst && (dst->format & LFI_YUV_10BIT))
        return fail(ctx, LFI_EINVAL, std::string(who) + ": 10-bit frames (LFI_YUV_I010, LFI_YUV_P010) are not supported: RGB-D frames are 8-bit");
    if(ctx->yuv_out_siting != LFI_YUV_SITING_CENTRE)
        return fail(ctx, LFI_EINVAL, std::string(who) + ": left-sited output (lfi_set_yuv_siting) is not supported: the chroma filter would mix the colour "
                                                        "and the depth half in the column between them");
    if(int rc = check_scaled_tiles(ctx, tile_w, tile_h))
        return rc;
    if(tile_w % 2 || tile_h % 2)
        return fail(ctx, LFI_EINVAL, std::string(who) + ": tile_w and tile_h must be even: no 2x2 chroma block may straddle the colour and the depth half");
    if(map_k < 0 || map_k > 1 || (flags & ~(uint32_t)(LFI_RGBD_INVERT | LFI_RGBD_VIEW_MAPS)))
        return fail(ctx, LFI_EINVAL, std::string(who) + ": bad map index (0 or 1) or unknown flags (LFI_RGBD_INVERT, LFI_RGBD_VIEW_MAPS)");
    const bool view_maps = flags & LFI_RGBD_VIEW_MAPS;
    if(view_maps && (!ctx->view_maps_set || !ctx->view_maps || ctx->view_maps.bytes() < plane_bytes(ctx) * 2 * ctx->views_n))
        return fail(ctx, LFI_EINVAL, std::string(who) + ": LFI_RGBD_VIEW_MAPS needs the per-view focus maps in use (lfi_view_focus_maps)");
    if(!view_maps && !ctx->maps)
        return fail(ctx, LFI_EINVAL, std::string(who) + ": the context has no focus maps");
    size_t extent = 0;
    if(const char *fault = yuv_surfaces_fault(dst, 2 * tile_w, tile_h, n, &extent))
        return fail(ctx, LFI_EINVAL, std::string(who) + ": " + fault);
    // n frames routed as lfi_download_views_yuv routes them: the caller's surfaces in place, or the staged frames and copies of their bytes
    YuvDelivery d;
    if(int rc = open_yuv_delivery(ctx, who, *dst, extent, 2 * tile_w, tile_h, n, false, &d))
        return rc;
    if(!view_maps)
        if(int rc = join_filter(ctx)) // map 1 may still be in the making on the side stream; the per-view maps are made on the compute stream
            return rc;
    bool planar;
    lfi::RgbdYuvArgs a{};
    a.q.src = rendered_views(ctx, 0, &planar);
    a.q.tile_w = tile_w, a.q.tile_h = tile_h;
    a.q.v0 = v0, a.q.first = 0, a.q.tiles_x = 2;
    // the map as views of one RGBA plane each: the context's map for every frame, or plane map_k of each view's pair
    const size_t plane = plane_bytes(ctx);
    a.map = view_maps ? lfi::ViewsSrc{ctx->view_maps.get() + plane * (2 * (size_t)v0 + map_k), 2 * plane, (uint32_t)ctx->width, (uint32_t)ctx->height, 0u}
                      : lfi::ViewsSrc{ctx->maps.get() + plane * map_k, 0, (uint32_t)ctx->width, (uint32_t)ctx->height, 0u};
    a.s = d.frames, a.k = lfi::YUV_COEFFS[matrix * 2 + range];
    a.flip = flags & LFI_RGBD_INVERT ? 255u : 0u;
    LFI_HIP(ctx, lfi::launch_rgbd_yuv_scale(ctx->stream, planar, dst->format, a, n));
    return finish_yuv_delivery(ctx, *dst, n, d);
}

int lfi_download_native(lfi_ctx *ctx, const lfi_lenticular *lens, int v0, int out_w, int out_h, int tile_w, int tile_h, uint8_t *rgba, size_t pitch_bytes)
{
    if(!ctx)
        return LFI_EINVAL;
    if(int rc = check_rendered(ctx))
        return rc;
    if(ctx->windowed)
        return fail(ctx, LFI_EINVAL, "a native image needs whole views: its subpixels read rows the row window's band does not hold");
    if(!lens)
        return fail(ctx, LFI_EINVAL, "a native image needs a lens description (lfi_lenticular)");
    if(lens->flags & ~uint32_t(LFI_LENT_INVERT | LFI_LENT_BGR | LFI_LENT_BILINEAR | LFI_LENT_BLEND))
        return fail(ctx, LFI_EINVAL, "unknown lfi_lenticular flag bits");
    if(lens->views < 1 || v0 < 0 || (long)v0 + lens->views > ctx->views_n)
        return fail(ctx, LFI_EINVAL, "a native image needs lens views >= 1 and as many views starting at v0 inside [0, views)");
    if(int rc = check_scaled_tiles(ctx, tile_w, tile_h))
        return rc;
    const int W = ctx->width, H = ctx->height;
    if(out_w < 1 || out_h < 1 || (uint32_t)out_w > lfi::NATIVE_MAX || (uint32_t)out_h > lfi::NATIVE_MAX)
        return fail(ctx, LFI_EINVAL, "native images are 1 … 65535 pixels per axis");
    if(!rgba || pitch_bytes < (size_t)out_w * 4)
        return fail(ctx, LFI_EINVAL, "bad native image pointer or pitch");
    if(int rc = bind(ctx))
        return rc;
    const int n = lens->views;
    const bool scaled = tile_w != W || tile_h != H;
    LFI_HIP(ctx, ctx->native.reserve((size_t)out_w * out_h * 4));
    bool planar;
    lfi::NativeArgs a{};
    a.src = rendered_views(ctx, v0, &planar); // the views in place, in the layout they were rendered in
    a.out = ctx->native.as<uint32_t>();
    a.out_w = out_w, a.out_h = out_h;
    a.x_step = lens->x_step, a.y_step = lens->y_step, a.phase0 = lens->phase0, a.n = n;
    a.invert = (lens->flags & LFI_LENT_INVERT) ? 1u : 0u;
    if(scaled)
    {
        // stage 1: the n scaled tiles as a quilt ONE tile wide in the quilt buffer — RGBA views of tile_w × tile_h; none of it is copied
        const size_t tile_bytes = (size_t)tile_w * tile_h * 4;
        LFI_HIP(ctx, ctx->quilt.reserve(tile_bytes * n));
        lfi::QuiltScaleArgs q{};
        q.src = rendered_views(ctx, 0, &planar);
        q.quilt = ctx->quilt.as<uint32_t>();
        q.tile_w = tile_w, q.tile_h = tile_h;
        q.v0 = v0, q.first = 0, q.tiles_x = 1;
        LFI_HIP(ctx, lfi::launch_quilt_scale(ctx->stream, planar, q, n));
        a.src = lfi::ViewsSrc{ctx->quilt.get(), tile_bytes, (uint32_t)tile_w, (uint32_t)tile_h, 0u};
    }
    // any filter flag takes native_filter; bilinear taps of a tile of the output's size all have weight 0: nearest, the flag dropped
    uint32_t filter = lens->flags & (LFI_LENT_BGR | LFI_LENT_BILINEAR | LFI_LENT_BLEND);
    if(tile_w == out_w && tile_h == out_h)
        filter &= ~uint32_t(LFI_LENT_BILINEAR);
    if(filter)
        LFI_HIP(ctx, lfi::launch_native_filter(ctx->stream, planar && !scaled, (filter & LFI_LENT_BILINEAR) != 0, (filter & LFI_LENT_BLEND) != 0,
                                               lfi::NativeFilterArgs{a, (filter & LFI_LENT_BGR) ? 1u : 0u}));
    else
        LFI_HIP(ctx, lfi::launch_native_interlace(ctx->stream, planar && !scaled, a));
    LFI_HIP(ctx, hipMemcpy2DAsync(rgba, pitch_bytes, ctx->native.get(), (size_t)out_w * 4, (size_t)out_w * 4, out_h, hipMemcpyDeviceToHost, ctx->stream));
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LFI_OK;
}

int lfi_alloc_pinned(size_t bytes, void **out_ptr)
{
    if(!out_ptr || bytes == 0)
        return LFI_EINVAL;
    *out_ptr = nullptr;
    const hipError_t e = hipHostMalloc(out_ptr, bytes, hipHostMallocDefault);
    if(e != hipSuccess)
    {
        g_create_error = std::string("hipHostMalloc: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? LFI_ENOMEM : LFI_EHIP;
    }
    return LFI_OK;
}

int lfi_free_pinned(void *ptr)
{
    if(!ptr)
        return LFI_OK;
    return hipHostFree(ptr) == hipSuccess ? LFI_OK : LFI_EHIP;
}

int lfi_upload_map(lfi_ctx *ctx, int k, const uint8_t *rgba, size_t pitch_bytes)
{
    if(!ctx)
        return LFI_EINVAL;
    if(!ctx->maps)
        return fail(ctx, LFI_EINVAL, "lfi_set_grid has not been called");
    if(k < 0 || k > 1 || !rgba || pitch_bytes < (size_t)ctx->width * 4)
        return fail(ctx, LFI_EINVAL, "bad map index, pointer or pitch");
    if(int rc = bind(ctx))
        return rc;
    if(int rc = join_filter(ctx))
        return rc;
    LFI_HIP(ctx, hipMemcpy2DAsync(ctx->maps.get() + plane_bytes(ctx) * k, (size_t)ctx->width * 4, rgba, pitch_bytes,
                                  (size_t)ctx->width * 4, ctx->height, hipMemcpyHostToDevice, ctx->stream));
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LFI_OK;
}

const char *lfi_list_variants(int method)
{
    static std::string ten, std_;
    if(ten.empty())
    {
        for(int i = 0; i < kNumTenVariants; i++)
            ten += std::string(ten.empty() ? "" : ",") + kTenVariants[i].name;
        for(int i = 0; i < kNumStdVariants; i++)
            std_ += std::string(std_.empty() ? "" : ",") + kStdVariants[i].name;
    }
    if(method == LFI_METHOD_TEN_WM)
        return ten.c_str();
    if(method == LFI_METHOD_STD)
        return std_.c_str();
    if(method == LFI_KERNEL_FOCUS_ESTIMATE)
        return "factored,lds,packed_p2,plain,factored_direct";
    return "";
}

int lfi_set_variant(lfi_ctx *ctx, int method, const char *name)
{
    if(!ctx || !name)
        return LFI_EINVAL;
    const bool is_auto = std::strcmp(name, "auto") == 0;
    if(method == LFI_METHOD_TEN_WM)
    {
        if(is_auto)
        {
            ctx->ten_variant = 0;
            return LFI_OK;
        }
        for(int i = 0; i < kNumTenVariants; i++)
            if(std::strcmp(name, kTenVariants[i].name) == 0)
            {
                ctx->ten_variant = int(i);
                return LFI_OK;
            }
    }
    else if(method == LFI_METHOD_STD)
    {
        if(is_auto)
        {
            ctx->std_variant = 0;
            return LFI_OK;
        }
        for(int i = 0; i < kNumStdVariants; i++)
            if(std::strcmp(name, kStdVariants[i].name) == 0)
            {
                ctx->std_variant = int(i);
                return LFI_OK;
            }
    }
    else if(method == LFI_KERNEL_FOCUS_ESTIMATE)
    {
        static const char *const names[] = {"factored", "lds", "packed_p2", "plain", "factored_direct"};
        if(is_auto)
        {
            ctx->focus_variant = 0;
            return LFI_OK;
        }
        for(int i = 0; i < 5; i++)
            if(std::strcmp(name, names[i]) == 0)
            {
                ctx->focus_variant = i;
                return LFI_OK;
            }
    }
    return fail(ctx, LFI_EINVAL, std::string("unknown kernel variant ") + name);
}

int lfi_download_coords(lfi_ctx *ctx, int g, int all_focus, int map_index, lfi_int2 *out_hw)
{
    if(!ctx)
        return LFI_EINVAL;
    if(ctx->inputs_released)
        return fail(ctx, LFI_EINVAL, "the RGBA inputs were released (lfi_release_inputs): lfi_set_grid and upload the images again");
    if(!ctx->grid || !ctx->have_params)
        return fail(ctx, LFI_EINVAL, "lfi_set_grid / lfi_set_params have not been called");
    if(g < 0 || g >= ctx->n || !out_hw || map_index < 0 || map_index > 1)
        return fail(ctx, LFI_EINVAL, "bad image index, map index or pointer");
    if(ctx->windowed)
        return fail(ctx, LFI_EINVAL, "coordinate dumps are not supported with a row window");
    if(int rc = bind(ctx))
        return rc;
    if(int rc = join_filter(ctx))
        return rc;
    const size_t bytes = sizeof(lfi_int2) * (size_t)ctx->width * ctx->height;
    DeviceBuffer d; // freed on every way out
    LFI_HIP(ctx, d.reserve(bytes));
    KernelArgs a = make_args(ctx, 0, ctx->views_n, LFI_METHOD_STD);
    a.map_index = map_index;
    hipLaunchKernelGGL(lfi::dump_coords, pixel_grid(ctx), dim3(256), 0, ctx->stream, a, g, all_focus, d.as<lfi_int2>());
    LFI_HIP(ctx, hipGetLastError());
    LFI_HIP(ctx, hipMemcpyAsync(out_hw, d.get(), bytes, hipMemcpyDeviceToHost, ctx->stream));
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LFI_OK;
}

int lfi_download_prequant(lfi_ctx *ctx, int method, int all_focus, int v, float *out_hw3)
{
    if(int rc = check_render_args(ctx, method, v, v + 1))
        return rc;
    if(!out_hw3)
        return fail(ctx, LFI_EINVAL, "out_hw3 is NULL");
    if(int rc = bind(ctx))
        return rc;
    const size_t bytes = sizeof(float) * 3 * (size_t)ctx->width * ctx->height;
    KernelArgs a = make_args(ctx, v, v + 1, method);
    if(ctx->flags & LFI_FLAG_LINEAR_LIGHT) // refused by name before anything is reserved
        return fail(ctx, LFI_EINVAL, std::string("LFI_FLAG_LINEAR_LIGHT is set: ") + kLinearNoPrequant);
    if(ctx->flags & LFI_FLAG_IN_FRAME) // refused by name before anything is reserved
        return fail(ctx, LFI_EINVAL, std::string("LFI_FLAG_IN_FRAME is set: ") + kInFrameNoPrequant);
    if(ctx->flags & LFI_FLAG_DEEP_VIEWS) // refused by name before anything is reserved
        return fail(ctx, LFI_EINVAL, std::string("LFI_FLAG_DEEP_VIEWS is set: ") + kDeepNoPrequant);
    LFI_HIP(ctx, ctx->prequant.reserve(bytes));
    a.prequant = ctx->prequant.as<float>();
    a.prequant_view = v;
    if(int rc = launch_blend(ctx, method, all_focus, a))
        return rc;
    LFI_HIP(ctx, hipMemcpyAsync(out_hw3, ctx->prequant.get(), bytes, hipMemcpyDeviceToHost, ctx->stream));
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LFI_OK;
}

int lfi_debug_mfma_f16(lfi_ctx *ctx, const uint16_t *a_32x16, const uint16_t *b_16x32, float *c_32x32)
{
    if(!ctx || !a_32x16 || !b_16x32 || !c_32x32)
        return LFI_EINVAL;
    if(int rc = bind(ctx))
        return rc;
    DeviceBuffer buf;
    LFI_HIP(ctx, buf.reserve(1024 + 1024 + 4096));
    uint8_t *const d = buf.get();
    LFI_HIP(ctx, hipMemcpyAsync(d, a_32x16, 1024, hipMemcpyHostToDevice, ctx->stream));
    LFI_HIP(ctx, hipMemcpyAsync(d + 1024, b_16x32, 1024, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(lfi::probe_mfma_f16, dim3(1), dim3(64), 0, ctx->stream, reinterpret_cast<const uint16_t *>(d),
                       reinterpret_cast<const uint16_t *>(d + 1024), reinterpret_cast<float *>(d + 2048));
    LFI_HIP(ctx, hipGetLastError());
    LFI_HIP(ctx, hipMemcpyAsync(c_32x32, d + 2048, 4096, hipMemcpyDeviceToHost, ctx->stream));
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LFI_OK;
}

int lfi_debug_pk_minmax3_f16(lfi_ctx *ctx, uint32_t *out_mismatches)
{
    if(!ctx || !out_mismatches)
        return LFI_EINVAL;
    if(int rc = bind(ctx))
        return rc;
    DeviceBuffer buf;
    LFI_HIP(ctx, buf.reserve(sizeof(uint32_t)));
    uint32_t *const d = buf.as<uint32_t>();
    LFI_HIP(ctx, hipMemsetAsync(d, 0, sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(lfi::probe_pk_minmax3, dim3(1u << 16), dim3(256), 0, ctx->stream, d);
    LFI_HIP(ctx, hipGetLastError());
    LFI_HIP(ctx, hipMemcpyAsync(out_mismatches, d, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LFI_OK;
}

int lfi_debug_mfma_f16_chain(lfi_ctx *ctx, int shape, int k, const uint16_t *a_32xk, const uint16_t *b_kx32, float *c_32x32)
{
    if(!ctx || !a_32xk || !b_kx32 || !c_32x32 || (shape != 0 && shape != 1) || k < 32 || k > 256 || k % 32)
        return LFI_EINVAL;
    if(int rc = bind(ctx))
        return rc;
    const size_t ab = (size_t)32 * k * sizeof(uint16_t);
    DeviceBuffer buf;
    LFI_HIP(ctx, buf.reserve(2 * ab + 4096));
    uint8_t *const d = buf.get();
    LFI_HIP(ctx, hipMemcpyAsync(d, a_32xk, ab, hipMemcpyHostToDevice, ctx->stream));
    LFI_HIP(ctx, hipMemcpyAsync(d + ab, b_kx32, ab, hipMemcpyHostToDevice, ctx->stream));
    const uint16_t *da = reinterpret_cast<const uint16_t *>(d), *db = reinterpret_cast<const uint16_t *>(d + ab);
    float *dc = reinterpret_cast<float *>(d + 2 * ab);
    if(shape == 0)
        hipLaunchKernelGGL(lfi::probe_mfma_f16_chain<0>, dim3(1), dim3(64), 0, ctx->stream, da, db, k, dc);
    else
        hipLaunchKernelGGL(lfi::probe_mfma_f16_chain<1>, dim3(1), dim3(64), 0, ctx->stream, da, db, k, dc);
    LFI_HIP(ctx, hipGetLastError());
    LFI_HIP(ctx, hipMemcpyAsync(c_32x32, d + 2 * ab, 4096, hipMemcpyDeviceToHost, ctx->stream));
    LFI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LFI_OK;
}

int lfi_debug_poison(lfi_ctx *ctx, uint32_t what, uint8_t byte)
{
    if(!ctx)
        return LFI_EINVAL;
    if(what & ~uint32_t(LFI_POISON_VIEWS | LFI_POISON_SCRATCH | LFI_POISON_MAPS | LFI_POISON_FOCUS_WORKSPACE | LFI_POISON_DERIVED | LFI_POISON_VIEW_MAPS | LFI_POISON_DEEP))
        return fail(ctx, LFI_EINVAL, "lfi_debug_poison: unknown LFI_POISON_* bits");
    if((what & LFI_POISON_DERIVED) && ctx->inputs_released)
        return fail(ctx, LFI_EINVAL, "lfi_debug_poison: the planar copy is the only copy of the inputs after lfi_release_inputs");
    if(int rc = bind(ctx))
        return rc;
    // in stream order like every other call: behind the uploads (the eager planar refresh) and the focus map's filter on the side stream
    if(int rc = join_uploads(ctx))
        return rc;
    if(int rc = join_filter(ctx))
        return rc;
    hipStream_t st = ctx->stream;
    auto fill = [&](const DeviceBuffer &b, size_t bytes) -> int {
        if(b && bytes)
            LFI_HIP(ctx, hipMemsetAsync(b.get(), byte, bytes, st));
        return LFI_OK;
    };
    int rc = LFI_OK;
    if(what & LFI_POISON_VIEWS)
        rc = rc ? rc : fill(ctx->views, ctx->views ? out_plane_bytes(ctx) * ctx->views_n : 0);
    if(what & LFI_POISON_SCRATCH)
    {
        rc = rc ? rc : fill(ctx->rgba_scratch, ctx->rgba_scratch.bytes());
        rc = rc ? rc : fill(ctx->dl_plane, ctx->dl_plane.bytes());
        rc = rc ? rc : fill(ctx->prequant, ctx->prequant.bytes());
        rc = rc ? rc : fill(ctx->quilt, ctx->quilt.bytes());
        rc = rc ? rc : fill(ctx->native, ctx->native.bytes());
        rc = rc ? rc : fill(ctx->yuv[0], ctx->yuv[0].bytes());
        rc = rc ? rc : fill(ctx->yuv[1], ctx->yuv[1].bytes());
        rc = rc ? rc : fill(ctx->yuv_in, ctx->yuv_in.bytes());
        rc = rc ? rc : fill(ctx->views2, ctx->views2.bytes());
        rc = rc ? rc : fill(ctx->cmp_stage[0], ctx->cmp_stage[0].bytes());
        rc = rc ? rc : fill(ctx->cmp_stage[1], ctx->cmp_stage[1].bytes());
        rc = rc ? rc : fill(ctx->cmp_ws, ctx->cmp_ws.bytes());
    }
    if(what & LFI_POISON_DEEP)
        rc = rc ? rc : fill(ctx->deep, ctx->deep.bytes());
    if(what & LFI_POISON_MAPS)
        rc = rc ? rc : fill(ctx->maps, ctx->maps ? plane_bytes(ctx) * 2 : 0);
    if(what & LFI_POISON_VIEW_MAPS)
        rc = rc ? rc : fill(ctx->view_maps, ctx->view_maps.bytes());
    if(what & LFI_POISON_FOCUS_WORKSPACE)
    {
        rc = rc ? rc : fill(ctx->focus_ws, ctx->focus_ws.bytes());
        rc = rc ? rc : fill(ctx->curve_ws, ctx->curve_ws.bytes());
        ctx->pad_version = 0; // the padded planes of the estimate are rebuilt in full by the next lfi_focus_map
    }
    if(what & LFI_POISON_DERIVED)
    {
        rc = rc ? rc : fill(ctx->planar, ctx->planar.bytes());
        if(ctx->planar)
            touch_all(ctx); // as lfi_grid_modified: the next render that reads the copy rebuilds all of it
    }
    return rc;
}

#if LFI_SX_TRACE
// measurement builds only (blend_stdx.hpp): the per-workgroup unit clocks of the last blend_stdx launch; not part of include/lfi.h
int lfi_debug_sx_trace(unsigned long long *out, int n_words)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(lfi::lfi_sx_trace_buf), sizeof(unsigned long long) * std::min(n_words, 1024 * 32)) == hipSuccess ? 0 : 1;
}
#endif
#if FRT_TRACE
// measurement builds only (focus_factored.hpp): clocks per wave and category of the last focus_range_t launch; not part of include/lfi.h
int lfi_debug_frt_trace(unsigned long long *out, int n_words)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(lfi::lfi_frt_trace_buf), sizeof(unsigned long long) * std::min(n_words, 256 * 16 * 8)) == hipSuccess ? 0 : 1;
}
#endif
#if LFI_P3_TRACE
// measurement builds only (blend_p3.hpp): the per-workgroup unit clocks of the last blend_p3 launch; not part of include/lfi.h
int lfi_debug_p3_trace(unsigned long long *out, int n_words)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(lfi::lfi_p3_trace_buf), sizeof(unsigned long long) * std::min(n_words, 1024 * 8)) == hipSuccess ? 0 : 1;
}
#endif
} // extern "C"

