// lfi_context.hpp — the context behind include/lfi.h's opaque lfi_ctx: device memory, streams and events, the parameter block, and
// the small helpers every entry point uses (error convention, stream joins, plane sizes, the kernel-argument block).
// This is the device-facing state of the reference's Interpolator (reference src/interpolator.cu:36-154: surfaces, __constant__ symbols,
// the weights allocation) as one object per GPU.  Included by lfi_hip.hip only (one translation unit).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/lfi.h"
#include "lfi_device.hpp"
#include "quality_batch.hpp"
#include "views_src.hpp"

using lfi::KernelArgs;

namespace {

thread_local std::string g_create_error;

} // namespace

// ---- owners: every device allocation, pinned buffer, event and stream below belongs to exactly one of these and goes with it --------------
// (DESIGN.md §3 "Lifetimes" lists each one: who allocates it under which policy, which calls release it, whether the stream is drained first)

// A device allocation (or, attached, a caller's memory that is only pointed at).  Freed with hipFree, which waits for the work in flight;
// a site whose stream must be drained BEFORE the old allocation goes synchronises it itself, in front of reserve.
class DeviceBuffer
{
public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer &&o) noexcept : p_(o.p_), bytes_(o.bytes_), owns_(o.owns_) { o.forget(); }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept
    {
        if(this != &o)
        {
            release();
            p_ = o.p_, bytes_ = o.bytes_, owns_ = o.owns_;
            o.forget();
        }
        return *this;
    }
    ~DeviceBuffer() { release(); }

    // grow only: nothing happens while the capacity is at least `need` (a larger allocation serves smaller needs too)
    hipError_t reserve(size_t need, bool *reallocated = nullptr) { return bytes_ >= need ? hipSuccess : replace(need, reallocated); }
    // exact fit: a new allocation whenever the capacity differs from `need`
    hipError_t fit(size_t need, bool *reallocated = nullptr) { return bytes_ == need ? hipSuccess : replace(need, reallocated); }
    void attach(void *p, size_t bytes) { adopt(p, bytes), owns_ = false; } // the caller's memory: never freed here
    void adopt(void *p, size_t bytes)                                      // an allocation made elsewhere (alloc_views), owned from now on
    {
        release();
        p_ = p, bytes_ = bytes, owns_ = true;
    }
    void release()
    {
        if(owns_ && p_)
            (void)hipFree(p_);
        forget();
    }

    uint8_t *get() const { return static_cast<uint8_t *>(p_); }
    template <class T>
    T *as() const { return static_cast<T *>(p_); }
    size_t bytes() const { return bytes_; } // capacity; of an attached buffer, the size the caller gave
    bool owned() const { return owns_; }
    explicit operator bool() const { return p_ != nullptr; }

private:
    void *p_ = nullptr;
    size_t bytes_ = 0;
    bool owns_ = false;

    void forget() { p_ = nullptr, bytes_ = 0, owns_ = false; }
    hipError_t replace(size_t need, bool *reallocated)
    {
        release();
        if(reallocated)
            *reallocated = true; // the old allocation and its contents are gone, whether or not the new one succeeds
        if(hipError_t e = hipMalloc(&p_, need))
        {
            p_ = nullptr;
            return e;
        }
        bytes_ = need, owns_ = true;
        return hipSuccess;
    }
};

// A page-locked host allocation
class PinnedBuffer
{
public:
    PinnedBuffer() = default;
    PinnedBuffer(const PinnedBuffer &) = delete;
    PinnedBuffer &operator=(const PinnedBuffer &) = delete;
    ~PinnedBuffer() { release(); }

    hipError_t reserve(size_t need) { return bytes_ >= need ? hipSuccess : replace(need); } // grow only
    hipError_t fit(size_t need) { return bytes_ == need ? hipSuccess : replace(need); }     // exact fit
    void release()
    {
        if(p_)
            (void)hipHostFree(p_);
        p_ = nullptr, bytes_ = 0;
    }
    uint8_t *get() const { return static_cast<uint8_t *>(p_); }
    size_t bytes() const { return bytes_; }

private:
    void *p_ = nullptr;
    size_t bytes_ = 0;

    hipError_t replace(size_t need)
    {
        release();
        if(hipError_t e = hipHostMalloc(&p_, need, hipHostMallocDefault))
        {
            p_ = nullptr;
            return e;
        }
        bytes_ = need;
        return hipSuccess;
    }
};

// An event / a stream handle that destroys itself; ensure() creates it on first use.  Both convert to the bare handle for the runtime's calls.
struct Event
{
    hipEvent_t h = nullptr;

    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() { release(); }
    hipError_t ensure(unsigned flags = hipEventDisableTiming) { return h ? hipSuccess : hipEventCreateWithFlags(&h, flags); }
    void release()
    {
        if(h)
            (void)hipEventDestroy(h);
        h = nullptr;
    }
    operator hipEvent_t() const { return h; }
};

struct Stream
{
    hipStream_t h = nullptr;

    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream()
    {
        if(h)
            (void)hipStreamDestroy(h);
    }
    hipError_t ensure() { return h ? hipSuccess : hipStreamCreateWithFlags(&h, hipStreamNonBlocking); }
    hipError_t ensure_with_priority(int priority) { return h ? hipSuccess : hipStreamCreateWithPriority(&h, hipStreamNonBlocking, priority); }
    operator hipStream_t() const { return h; }
};

// Two page-locked buffers, one event each: the host fills the current buffer, a copy out of it is enqueued on a stream, and the buffer is
// not written again before that copy has run (two uses later) — uploads in stream order without draining the stream.
struct StagingRing
{
    PinnedBuffer buf[2]; // of one capacity
    Event ev[2];
    int slot = 0;

    // the current buffer, at least `need` bytes and free to write: both buffers grow once their copies have run; else this one's copy has run
    template <class T>
    hipError_t acquire(size_t need, T **out)
    {
        if(std::min(buf[0].bytes(), buf[1].bytes()) < need)
        {
            for(int i = 0; i < 2; i++)
            {
                if(ev[i])
                    if(hipError_t e = hipEventSynchronize(ev[i]))
                        return e;
                buf[i].release();
            }
            for(int i = 0; i < 2; i++)
            {
                if(hipError_t e = ev[i].ensure())
                    return e;
                if(hipError_t e = buf[i].reserve(need))
                    return e;
            }
        }
        else if(hipError_t e = hipEventSynchronize(ev[slot]))
            return e;
        *out = reinterpret_cast<T *>(buf[slot].get());
        return hipSuccess;
    }

    // the copy out of the current buffer has been enqueued on s: mark its end and move to the other buffer
    hipError_t commit(hipStream_t s)
    {
        if(hipError_t e = hipEventRecord(ev[slot], s))
            return e;
        slot ^= 1;
        return hipSuccess;
    }

    hipEvent_t committed() const { return ev[slot ^ 1]; } // the event the last commit recorded

    void release() // waits for the copies out of the buffers
    {
        for(int i = 0; i < 2; i++)
        {
            if(ev[i])
                (void)hipEventSynchronize(ev[i]);
            buf[i].release();
            ev[i].release();
        }
        slot = 0;
    }
};

// One element of type T per (view, image), on the device as [N][pitch] (views contiguous, pitch = v_pad, zero padding views), written in
// stream order out of a staging ring (stage_view_rows)
template <class T>
struct ViewRows
{
    bool set = false;
    DeviceBuffer dev;
    int pitch = 0;
    StagingRing ring;

    const T *rows() const { return dev.as<const T>(); }

    void release() // the caller has drained the stream
    {
        set = false;
        dev.release();
        ring.release();
    }
};

struct lfi_ctx
{
    int device = 0;
    int cu_count = 256;
    // The streams are declared first: members are destroyed in reverse order of declaration, so every buffer and event below goes before
    // the streams do (lfi_destroy has synchronised all three and the device is current when `delete` runs).
    Stream own_stream;
    // asynchronous uploads (lfi_upload_image_async) and downloads of lfi_render_stream: a copy stream, created on first use
    Stream copy_stream;
    // side stream of the factored focus-map estimate (its small passes overlap the large ones), created on first use with high priority
    Stream aux_stream;
    hipStream_t stream = nullptr; // the compute stream: own_stream or the caller's (lfi_set_stream)
    Event ev0, ev1;               // timing events (created with hipEventDefault)
    Event ev_order;               // orders the work of the stream a caller switches away from before the stream it switches to
    bool uploads_pending = false; // copies enqueued on copy_stream that the compute stream has not been ordered after yet
    Event ev_uploads;
    Event ev_fork, ev_pad, ev_join;
    // the focus map's filter (map 0 → map 1) runs on the side stream behind the pick: an all-focus TEN_WM render, which reads map 0
    // (src/kernels.cu:430), does not wait for it; whatever reads map 1 or writes either map joins it first (join_filter)
    Event ev_pick, ev_filter;
    bool filter_pending = false;
    int cols = 0, rows = 0, n = 0, width = 0, height = 0;
    // row window (lfi_set_row_window): input rows held / output rows rendered; the whole image by default
    int in_y0 = 0, in_rows = 0, out_y0 = 0, out_rows = 0;
    bool windowed = false;
    DeviceBuffer grid; // N input planes of in_rows rows: the library's own (lfi_set_grid / lfi_set_row_window) or attached (lfi_attach_grid)
    // lfi_release_inputs: the RGBA planes are gone, the derived planar copy is the only copy of the inputs (fixed-focus renders through
    // the planar kernels only); a later lfi_upload_image goes through a one-image staging plane straight into the copy
    bool inputs_released = false;
    DeviceBuffer stage_plane;
    // set by lfi_prepare for a render that reads the planar copy: from then on images that arrive (lfi_upload_image, lfi_fill_synthetic_images)
    // refresh their planes of the copy AT ONCE instead of at the next render — the first render after a load is then only a launch
    bool eager_planar = false;
    DeviceBuffer maps;                // focus maps 0 and 1, whole-image planes
    DeviceBuffer views;               // the library's own (alloc_views) or attached (lfi_attach_views)
    int out_layout = LFI_LAYOUT_RGBA; // device layout of the views (lfi_set_output_layout)
    // deep views (LFI_FLAG_DEEP_VIEWS, deep_blend.hpp): 10-bit planes [views_n][3: R,G,B][out_rows][deep_pitch] of little-endian u16 beside the planar
    // views; allocated by lfi_prepare or the first deep render, released with the views.  They hold views [deep_v0, deep_v1) of the last
    // deep launch; empty after any launch that writes views without the flag
    DeviceBuffer deep;
    int deep_v0 = 0, deep_v1 = 0;
    DeviceBuffer rgba_scratch;        // planar layout: RGBA planes of all views for the kernels that only write RGBA (converted after the launch)
    DeviceBuffer dl_plane;            // planar layout: one RGBA plane that downloads expand a view into
    DeviceBuffer quilt;               // lfi_download_quilt[_tiles]: the quilt's rows of tiles as one RGBA image (grows, kept); lfi_download_native: its scaled tiles
    DeviceBuffer native;              // lfi_download_native: the native image, out_h × out_w dwords (grows, kept)
    // lfi_download_views_yuv420, lfi_download_views_yuv into host or unaligned device surfaces: the staged frames of a call's views (the padded
    // planes of yuv_geometry, dev_frame_bytes each, I420 or NV12) in yuv[0]; lfi_render_stream_yuv420: a block's staged frames in either, one
    // copied to the host while the next block is converted into the other (grow, kept)
    DeviceBuffer yuv[2];
    // lfi_upload_images_yuv420, lfi_upload_images_yuv from host or unaligned device surfaces: a chunk's staged frames, as yuvs_expand reads
    // them; written and read on the copy stream only, in stream order (grows, kept)
    DeviceBuffer yuv_in;
    // lfi_debug_set_mosaic_chunk_cap: the cap of the mosaic YUV uploads' staging chunks in bytes; 0: the calls' own 256 MiB
    size_t mosaic_chunk_cap = 0;
    // parameter block
    bool have_params = false;
    int views_n = 0, k_pad = 0, v_pad = 0, n_focus_ids = 0;
    DeviceBuffer param_blob; // one allocation holding all parameter arrays, twice (see param_half)
    size_t param_total = 0;  // bytes of ONE copy of the arrays as lfi_set_params laid them out: an equal total is replaced in place
    // lfi_set_params with an unchanged blob size (a focus sweep, a new trajectory with as many views): the new arrays go through the
    // staging ring and a stream-ordered copy — no synchronisation, no allocation
    StagingRing param_ring;
    // … and there are TWO copies of the arrays on the device: a replacement is copied into the idle one on the copy stream, beside the renders
    // still running from the other (round 5: in stream order behind them it cost a fixed-focus sweep 22 µs per step, profiles/r05_notes.md)
    size_t param_half_stride = 0;
    int param_half = 0;
    Event ev_half_done[2]; // recorded on the compute stream when the context switches away from a half
    bool half_done_recorded[2] = {false, false};
    size_t blob_off_w16 = 0, blob_weights_bytes = 0; // the four weight arrays inside the blob (what lfi_render_stream replaces per block)
    // lfi_render_stream: page-locked staging for two blocks' weight arrays, a second set of views, events
    PinnedBuffer stream_staging[2];
    DeviceBuffer views2;
    Event ev_h2d[2], ev_rendered[2], ev_d2h[2];
    // lfi_keep_views: a copy of views [kept_v0, kept_v0 + kept_n) in the layout they were rendered in — lfi_compare_views' device-side references
    DeviceBuffer kept;
    int kept_v0 = 0, kept_n = 0;
    // lfi_compare_views: two staging buffers for chunks of host references (a copy into one runs beside the reduction out of the other),
    // and one workspace: the per-view records, then the per-workgroup partial sums (grows, kept)
    DeviceBuffer cmp_stage[2];
    Event ev_cmp_copied[2], ev_cmp_reduced[2];
    DeviceBuffer cmp_ws;
    lfi_int2 *d_focused = nullptr;
    lfi_float2 *d_offsets = nullptr;
    uint16_t *d_w16 = nullptr, *d_w16s = nullptr;
    bool weights_scalable = false; // every weight finite and in [0, 2): the ×2^15 copy is exact and the packed epilogue valid
    bool weights_sum_ok = false;   // … and every view's weights sum to at most 2: blend_planar<STDF>'s error bounds hold (sums < 512)
    float *d_w32 = nullptr, *d_w32t = nullptr;
    int32_t *d_ids = nullptr;
    float focus = 0, range = 0;
    int radius[2] = {1, 1};
    int fo_min[2] = {0, 0}, fo_max[2] = {0, 0}; // bounds of the integer offsets
    uint32_t flags = 0;
    DeviceBuffer prequant; // lfi_download_prequant: [3][H][W] floats
    std::vector<lfi_float2> h_focus_offsets; // offsets of the focus_map_ids images (host copy: sizes the padded planes)
    std::vector<lfi_float2> h_offsets;       // offsets of all images (host copy: row-window coverage checks of all-focus renders)
    // planar copy of the inputs for blend_planar (built on demand; valid while planar_version == grid_version)
    DeviceBuffer planar;
    int planar_pitch = 0, planar_padx = 0, planar_reach = 0; // bytes per plane row; left padding; the largest |x offset| it was built for
    DeviceBuffer d_planar_phase;            // [LFI_MAX_IMAGES] int32 per-image phase of the planar copy (device)
    std::vector<int32_t> planar_phase;      // the same on the host
    StagingRing phase_ring;                 // a rebuild's phases go to the device in stream order, no host wait
    std::vector<lfi_int2> h_focused;        // the integer offsets of the current parameters (host copy)
    unsigned launches_with_offsets = 0;     // fixed-focus launches since the integer offsets last changed
    uint64_t grid_version = 1, planar_version = 0;
    // which images changed: grid_full_version = grid_version at the last change that may have touched every image; img_version[g] = at the
    // last change of image g alone (lfi_upload_image[_async], lfi_fill_synthetic_images).  A derived copy brought up to date at version v
    // holds image g's current pixels iff max(img_version[g], grid_full_version) ≤ v: one replaced image costs one image's planes.
    uint64_t grid_full_version = 1;
    std::vector<uint64_t> img_version;
    bool grid_tracked = true; // every write to the planes goes through this library (or is announced by lfi_grid_modified)
    DeviceBuffer focus_ws; // workspace of the factored focus-map estimate (plan, E, K), allocated on first use
    // the estimate's padded copies of the sampled images (focus_pad, the tail of focus_ws) depend on the inputs and on a BOUND of the
    // candidates' shifts only: kept between lfi_focus_map calls (a focus sweep over one light field — BASELINE config 5 — pads once)
    // while pad_version == grid_version, the same images are sampled with the same block radius, and pad_shift still covers the request
    uint64_t pad_version = 0;
    int pad_shift[2] = {0, 0}, pad_radius[2] = {0, 0};
    std::vector<int32_t> pad_ids, h_focus_ids;
    // lfi_set_focus_steps: the candidates of lfi_focus_map's sweep, a multiple of 32 up to 256; a context setting that lfi_set_grid, lfi_set_params
    // and lfi_set_row_window leave alone.  Above 32 the factored estimate runs one pass per 32 candidates and carries each pixel's minimum
    // between them in focus_ws's carry plane (lfi_focus_sched.hpp)
    int focus_steps = lfi::FOCUS_STEPS;
    // lfi_set_yuv_siting: where the chroma samples of YUV 4:2:0 frames lie (LFI_YUV_SITING_*), of the frames the upload calls read and of the
    // frames the download calls write; a context setting like focus_steps
    int yuv_in_siting = 0, yuv_out_siting = 0;
    DeviceBuffer curve_ws; // lfi_focus_curve: the curve and its result, then the per-workgroup partial sums (grows, kept)
    int ten_variant = 0, std_variant = 0, focus_variant = 0;
    // lfi_focus_route_info: the last estimate call's route, noted where each launch is chosen (route_begin, lfi_focus_sched.hpp); the
    // per-pass counts stay on the device, route_counts_at bytes into focus_ws, until the call asks for them
    lfi_focus_route route = {0, 0, "", "", 0, 0, "", "", 0, 0, 0, {0, 0}, 0, 0, 0, 0, 0, 0, {0}, {0}, {0}};
    size_t route_counts_at = 0;
    int tiles_passes = 0; // the factored passes lfi_focus_tiles_steps' last call ran; 0: it took focus_curve_partial tile by tile (lfi_focus_tiles_passes)
    mutable const char *last_kernel = ""; // the blend kernel the last render launched (lfi_last_kernel_name)
    mutable unsigned sweep_launches = 0;  // blend_p3 / blend_planar alternate their sweep direction from launch to launch
    float derived_build_ms = 0.0f;        // duration of the last planar_build (measured by lfi_prepare only)
    // per-view rows (stage_view_rows): cleared (not freed: renders in flight may still read them) by lfi_set_params and
    // lfi_set_row_window, freed by lfi_set_grid.  lfi_set_view_offsets: integer offsets for fixed-focus renders; lfi_set_view_float_offsets: float offsets for
    // all-focus renders, also kept as given, [views][N], for the row-window check at render time
    ViewRows<lfi_int2> view_offsets;
    int view_offsets_reach = 0;             // max |D.x| over the integer rows set: the padding the planar copy needs to serve them
    ViewRows<lfi_float2> view_float_offsets;
    std::vector<lfi_float2> h_view_float_offsets;
    // per-view focus maps (lfi_view_focus_maps): [views][2][H][W] RGBA, each view's pair laid out like maps 0 / 1; allocated on first use,
    // freed with the per-view rows.  view_maps_set: all-focus renders over the float rows read them — cleared with the float rows
    DeviceBuffer view_maps;
    bool view_maps_set = false;
    // the estimate's own copy of the float rows, [V][N], and each view's ids in pad-slot order, [V][n_ids], staged through view_focus_ring
    DeviceBuffer view_focus_args;
    StagingRing view_focus_ring;
    int view_maps_padded = 0; // planes the last lfi_view_focus_maps padded (focus_pad slots)
    std::string err;
};

namespace {

// Every allocation of the views is ordinary device memory (hipMalloc) and goes back to the runtime with hipFree.  Rounds 2-3 placed the
// library's own planar views in hipDeviceMallocUncached memory (write-only planes that bypass the caches: -3.5 % at config 2 in round 2) and
// then had to keep every such block alive for the whole process, because contexts created after freed uncached ranges had been recycled as
// ordinary memory rendered garbage (profiles/r03_notes.md section 6).  Round 3's own A/B (profiles/r03_views_memory_ab.txt) shows no gain
// left from the placement outside box noise, so round 4 removed it together with the immortal pool: no allocation outlives its context.
// Measurement builds: LFI_VIEWS_MEMORY=uncached|finegrained still selects the other kinds for A/B runs.
hipError_t alloc_views(DeviceBuffer &out, size_t bytes)
{
#ifdef LFI_MEASUREMENT_BUILD
    const char *e = std::getenv("LFI_VIEWS_MEMORY");
    const unsigned kind = e && std::strcmp(e, "uncached") == 0 ? hipDeviceMallocUncached : e && std::strcmp(e, "finegrained") == 0 ? hipDeviceMallocFinegrained : 0;
    if(kind)
    {
        void *p = nullptr;
        const hipError_t err = hipExtMallocWithFlags(&p, bytes, kind);
        if(err == hipSuccess)
            out.adopt(p, bytes);
        return err;
    }
#endif
    return out.fit(bytes);
}

int fail(lfi_ctx *ctx, int code, const std::string &msg)
{
    if(ctx)
        ctx->err = msg;
    else
        g_create_error = msg;
    return code;
}

// what every call that reads the rendered views refuses first, in the same words
int check_rendered(lfi_ctx *ctx)
{
    if(!ctx->views || !ctx->have_params)
        return fail(ctx, LFI_EINVAL, "nothing rendered yet");
    return LFI_OK;
}

#define LFI_HIP(ctx, call)                                                                                           \
    do                                                                                                                \
    {                                                                                                                 \
        hipError_t e_ = (call);                                                                                       \
        if(e_ != hipSuccess)                                                                                          \
            return fail(ctx, e_ == hipErrorOutOfMemory ? LFI_ENOMEM : LFI_EHIP,                                       \
                        std::string(#call) + ": " + hipGetErrorString(e_));                                           \
    } while(0)

int bind(lfi_ctx *ctx)
{
    LFI_HIP(ctx, hipSetDevice(ctx->device));
    return LFI_OK;
}

// Order everything enqueued on the compute stream from now on after the asynchronous uploads issued so far (no host wait).
int join_uploads(lfi_ctx *c)
{
    if(!c->uploads_pending)
        return LFI_OK;
    LFI_HIP(c, hipEventRecord(c->ev_uploads, c->copy_stream));
    LFI_HIP(c, hipStreamWaitEvent(c->stream, c->ev_uploads, 0));
    c->uploads_pending = false;
    return LFI_OK;
}

// Order everything enqueued on the compute stream from now on after the focus-map filter that may still run on the side stream.
int join_filter(lfi_ctx *c)
{
    if(!c->filter_pending)
        return LFI_OK;
    LFI_HIP(c, hipStreamWaitEvent(c->stream, c->ev_filter, 0));
    c->filter_pending = false;
    return LFI_OK;
}

int ensure_copy_stream(lfi_ctx *c)
{
    LFI_HIP(c, c->copy_stream.ensure());
    LFI_HIP(c, c->ev_uploads.ensure());
    return LFI_OK;
}

// the side stream of the factored focus-map estimate and its fork / join events; high priority: the small passes should not queue behind the big ones
int ensure_aux_stream(lfi_ctx *c)
{
    if(c->aux_stream)
        return LFI_OK;
    int prio_low = 0, prio_high = 0; // numerically lower = higher priority
    LFI_HIP(c, hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
    LFI_HIP(c, c->aux_stream.ensure_with_priority(prio_high));
    LFI_HIP(c, c->ev_fork.ensure());
    LFI_HIP(c, c->ev_pad.ensure());
    LFI_HIP(c, c->ev_join.ensure());
    return LFI_OK;
}

size_t plane_bytes(const lfi_ctx *c) // a whole-image plane (focus maps; inputs and outputs without a row window)
{
    return (size_t)c->width * c->height * 4;
}

size_t in_plane_bytes(const lfi_ctx *c)
{
    return (size_t)c->width * c->in_rows * 4;
}

// planar view layout: bytes per row of a byte plane — a multiple of 128, so that every row starts on a cache line and every store
// instruction of blend_p3 (16 lanes × 8 bytes) writes ONE whole line.  With W rounded up to 16 only, a width that is not a multiple of 128
// put the rows at odd line phases and every store wrote two partial lines — into uncached memory: 1904 pixels 385 µs, 1936 pixels
// 366 µs per config-2-like launch against 153 µs at 1920 (tools/plane_skew.py, profiles/r03_plane_skew.txt).
int view_pitch(const lfi_ctx *c)
{
    return (c->width + 127) / 128 * 128;
}

// deep planes: bytes per row of a u16 plane — 2·W rounded up to 128
int deep_pitch(const lfi_ctx *c)
{
    return (2 * c->width + 127) / 128 * 128;
}

size_t deep_bytes(const lfi_ctx *c)
{
    return (size_t)c->views_n * 3 * c->out_rows * deep_pitch(c);
}

void drop_deep_range(lfi_ctx *c)
{
    c->deep_v0 = c->deep_v1 = 0;
}

size_t rgba_out_plane_bytes(const lfi_ctx *c)
{
    return (size_t)c->width * c->out_rows * 4;
}

size_t out_plane_bytes(const lfi_ctx *c) // one view as stored on the device
{
    if(c->out_layout == LFI_LAYOUT_PLANAR_RGB)
        return (size_t)3 * c->out_rows * view_pitch(c);
    return rgba_out_plane_bytes(c);
}

// The rendered views from view v0 on as a kernel reads them, H = the rows the views hold (out_rows).  *planar: the layout, which picks the
// kernel's instantiation
lfi::ViewsSrc rendered_views(const lfi_ctx *c, int v0, bool *planar)
{
    *planar = c->out_layout == LFI_LAYOUT_PLANAR_RGB;
    const size_t stride = out_plane_bytes(c);
    return lfi::ViewsSrc{c->views.get() + (size_t)v0 * stride, stride, (uint32_t)c->width, (uint32_t)c->out_rows, *planar ? (uint32_t)view_pitch(c) : 0u};
}

KernelArgs make_args(const lfi_ctx *c, int v0, int v1, int all_focus_method)
{
    KernelArgs a{};
    a.grid = c->grid.get();
    a.views = c->views.get();
    a.maps = c->maps.get();
    a.focused = c->d_focused;
    a.offsets = c->d_offsets;
    a.w16 = c->d_w16;
    a.w16s = c->d_w16s;
    a.w32 = c->d_w32;
    a.w32t = c->d_w32t;
    a.focus_ids = c->d_ids;
    a.prequant = nullptr;
    a.prequant_view = -1;
    a.width = c->width;
    a.height = c->height;
    a.in_y0 = c->in_y0;
    a.in_rows = c->in_rows;
    a.out_y0 = c->out_y0;
    a.out_rows = c->out_rows;
    a.map_y0 = 0;
    a.map_rows = c->height;
    a.n_images = c->n;
    a.k_pad = c->k_pad;
    a.v_pad = c->v_pad;
    a.v0 = v0;
    a.v1 = v1;
    a.n_focus_ids = c->n_focus_ids;
    a.planar = nullptr; // set by launch_blend when the copy is valid for this launch
    a.planar_phase = c->d_planar_phase.as<int32_t>();
    // blend_planar<STDF> (up to 64 images): chain bound N·2^-16 (half an ulp below 512 per fmaf: arithmetic) + the matrix core's accumulation
    // bound + 2^-11 of margin.  Accumulation bound: ANALYTIC by default since round 4, N·2^-15 (one whole fp16-product ulp per addend: true of
    // any accumulator that keeps ≥ 24 bits, nothing measured) — at these sizes the wider band costs nothing (tools/std_band_cost.py: config 2
    // 0.262 against 0.270 ms).  LFI_FLAG_STD_MEASURED_BAND: N·2^-17, a quarter ulp per addend, MEASURED on gfx950 (chains of
    // v_mfma_f32_32x32x16_f16 on operands built to expose alignment truncation stay within 0.086 ulp per addend;
    // tests/test_gpu_parity.py::test_mfma_f16_accumulation_error_bound asserts the quarter ulp) — rounds 2-3's default.
    a.std_band = float(c->n) * (0x1p-16f + 0x1p-15f) + 0x1p-11f;
    if((c->flags & LFI_FLAG_STD_MEASURED_BAND) && !(c->flags & LFI_FLAG_STD_ANALYTIC_BAND))
        a.std_band = float(c->n) * (0x1p-16f + 0x1p-17f) + 0x1p-11f;
    a.planar_pitch = c->planar_pitch;
    a.planar_padx = c->planar_padx;
    a.views_pitch = view_pitch(c);
    a.fo_min_x = c->fo_min[0];
    a.fo_max_x = c->fo_max[0];
    a.fo_min_y = c->fo_min[1];
    a.fo_max_y = c->fo_max[1];
    a.radius_x = c->radius[0];
    a.radius_y = c->radius[1];
    // the reference reads map 1 in Standard::process and map 0 in Tensors::process (src/kernels.cu:326 vs :430): reproduced by
    // default; LFI_FLAG_UNIFIED_FOCUS_MAP makes both read the filtered map
    a.map_index = 1;
    if(all_focus_method == LFI_METHOD_TEN_WM && !(c->flags & LFI_FLAG_UNIFIED_FOCUS_MAP))
        a.map_index = 0;
    a.focus = c->focus;
    a.range = c->range;
    a.flags = c->flags;
    // the reference's sweep (32 candidates, one pass); lfi_focus_map alone sets the context's focus_steps
    a.focus_steps = lfi::FOCUS_STEPS;
    a.focus_div = float(lfi::FOCUS_STEPS - 1);
    a.focus_i0 = 0;
    return a;
}

dim3 pixel_grid(const lfi_ctx *c)
{
    return dim3((c->width + 63) / 64, (c->height + 3) / 4, 1);
}


inline hipStream_t stream_of(const lfi_ctx *c) { return c->stream; }
inline void note_kernel(const lfi_ctx *c, const char *name) { c->last_kernel = name; }
inline uint32_t flags_of(const lfi_ctx *c) { return c->flags; }
inline dim3 pixel_grid_of(const lfi_ctx *c) { return pixel_grid(c); }
inline int cu_count_of(const lfi_ctx *c) { return c->cu_count; }

// The four device forms of a block of `rows` weight rows: fp16 as given, ×2^15 (exact; valid iff every weight is finite and in
// [0, 2)), f32, and f32 transposed — written at base + 0 / off_w16s / off_w32 / off_w32t (the region must be zero-initialised:
// padding rows and images stay zero).  *scalable / *sums_ok: the dispatch conditions lfi_set_params records.
void fill_weight_arrays(const uint16_t *weights_fp16, int rows, int n, int k_pad, int v_pad, uint8_t *base, size_t off_w16s, size_t off_w32, size_t off_w32t,
                        bool *scalable_out, bool *sums_ok_out)
{
    uint16_t *w16 = reinterpret_cast<uint16_t *>(base);
    uint16_t *w16s = reinterpret_cast<uint16_t *>(base + off_w16s);
    float *w32 = reinterpret_cast<float *>(base + off_w32);
    float *w32t = reinterpret_cast<float *>(base + off_w32t);
    bool scalable = true;
    for(int v = 0; v < rows; v++)
        for(int g = 0; g < n; g++)
        {
            const uint16_t h = weights_fp16[(size_t)v * n + g];
            const float f = static_cast<float>(__builtin_bit_cast(_Float16, h)); // half → float is exact
            w16[(size_t)v * k_pad + g] = h;
            // × 2^15 is exact in fp16 for every finite weight in [0, 2) (subnormals become normal, 1.999 → 65472)
            if(!(f >= 0.0f && f < 2.0f))
                scalable = false;
            else
                w16s[(size_t)v * k_pad + g] = __builtin_bit_cast(uint16_t, static_cast<_Float16>(f * 32768.0f));
            w32[(size_t)v * k_pad + g] = f;
            w32t[(size_t)g * v_pad + v] = f;
        }
    bool sums_ok = scalable;
    for(int v = 0; v < rows && sums_ok; v++)
    {
        double sum = 0;
        for(int g = 0; g < n; g++)
            sum += w32[(size_t)v * k_pad + g];
        sums_ok = sum <= 2.0;
    }
    *scalable_out = scalable;
    *sums_ok_out = sums_ok;
}

// every image may have changed / images [g0, g1) changed
void touch_all(lfi_ctx *c)
{
    c->grid_full_version = ++c->grid_version;
}

void touch_images(lfi_ctx *c, int g0, int g1)
{
    ++c->grid_version;
    if((int)c->img_version.size() != c->n)
    {
        c->img_version.assign(c->n, 0);
        c->grid_full_version = c->grid_version; // no per-image record yet
        return;
    }
    for(int g = g0; g < g1; g++)
        c->img_version[g] = c->grid_version;
}

bool image_changed_since(const lfi_ctx *c, int g, uint64_t version)
{
    // no per-image record (nothing but whole-grid changes so far: touch_images starts the record and bumps grid_full_version when it does):
    // the whole-grid version decides.  (Round 3 answered "changed" here, and contexts filled only by whole-grid calls — lfi_fill_synthetic_scene,
    // an attached grid + lfi_grid_modified — re-padded all sampled images on EVERY lfi_focus_map, one launch per image: 0.5 ms at 4K.)
    if((int)c->img_version.size() != c->n)
        return c->grid_full_version > version;
    return c->grid_full_version > version || c->img_version[g] > version;
}

// ---- what each API call invalidates (DESIGN.md §3 "Lifetimes" is the table these are checked against) -----------------------------------

void free_params(lfi_ctx *c)
{
    c->param_blob.release();
    c->param_total = 0;
    c->param_half = 0;
    c->half_done_recorded[0] = c->half_done_recorded[1] = false;
    c->have_params = false;
    c->view_offsets.set = c->view_float_offsets.set = false;
    c->view_maps_set = false;
}

// both sets of per-view rows' buffers and the per-view maps; the caller has drained the stream
void free_view_rows(lfi_ctx *c)
{
    c->view_offsets.release();
    c->view_float_offsets.release();
    c->h_view_float_offsets.clear();
    c->view_maps_set = false;
    c->view_maps.release();
    c->view_focus_args.release();
    c->view_focus_ring.release();
}

// The shared tail of lfi_set_view_offsets / lfi_set_view_float_offsets: rows at(v, g) of views [0, views_n) to r's device buffer as
// [N][v_pad] (views contiguous: one scalar run per image and chunk of views; padding views zero), in stream order like lfi_set_params —
// the copy runs behind the renders already enqueued, out of r's staging ring.
template <class T, class At>
int stage_view_rows(lfi_ctx *ctx, ViewRows<T> &r, At at)
{
    const int n = ctx->n, views = ctx->views_n, pitch = ctx->v_pad;
    const size_t bytes = sizeof(T) * (size_t)n * pitch;
    if(r.dev.bytes() < bytes)
    {
        LFI_HIP(ctx, hipStreamSynchronize(ctx->stream)); // renders in flight may read the old buffer
        r.set = false;
        LFI_HIP(ctx, r.dev.reserve(bytes));
    }
    T *staged = nullptr;
    LFI_HIP(ctx, r.ring.acquire(bytes, &staged));
    std::memset(staged, 0, bytes);
    for(int v = 0; v < views; v++)
        for(int g = 0; g < n; g++)
            staged[(size_t)g * pitch + v] = at(v, g);
    LFI_HIP(ctx, hipMemcpyAsync(r.dev.get(), staged, bytes, hipMemcpyHostToDevice, ctx->stream));
    LFI_HIP(ctx, r.ring.commit(ctx->stream));
    r.pitch = pitch;
    r.set = true;
    return LFI_OK;
}

// the copy of the parameter arrays that launches enqueued from now on read
uint8_t *param_base(const lfi_ctx *c)
{
    return c->param_blob.get() + (size_t)c->param_half * c->param_half_stride;
}

void free_views(lfi_ctx *c)
{
    c->views.release();
    c->deep.release();
    drop_deep_range(c);
    c->rgba_scratch.release();
    c->dl_plane.release();
    c->quilt.release();
    c->native.release();
    c->yuv[0].release();
    c->yuv[1].release();
    c->views2.release();
    c->cmp_stage[0].release();
    c->cmp_stage[1].release();
    c->cmp_ws.release();
}

// the kept views belong to the views' count, size and layout: lfi_set_grid, lfi_set_row_window, lfi_set_output_layout, and a
// lfi_set_params that changes the number of views (the callers have drained the stream)
void drop_kept(lfi_ctx *c)
{
    c->kept.release();
    c->kept_v0 = c->kept_n = 0;
}

// the one-image staging plane of uploads after lfi_release_inputs is sized by the row window in force when it was allocated, and the eager
// refresh lfi_prepare switched on belongs to the planes it was switched on for: both go whenever the input planes are replaced
void drop_stage_plane(lfi_ctx *c)
{
    c->stage_plane.release();
    c->eager_planar = false;
}

// the input planes go (lfi_set_grid, lfi_set_row_window, lfi_attach_grid, lfi_release_inputs): an attached grid is only forgotten
void drop_inputs(lfi_ctx *c)
{
    c->grid.release();
    c->inputs_released = false;
    drop_stage_plane(c);
}

void free_grid(lfi_ctx *c)
{
    drop_inputs(c);
    c->maps.release();
    c->prequant.release();
    c->focus_ws.release();
    c->pad_version = 0;
    // the geometry the released planes had goes with them: left in place, the next grid's planes "grow" from it (a quarter more padding than
    // asked for, or the old grid's larger reach) and a reused context allocates more than a fresh one
    c->pad_shift[0] = c->pad_shift[1] = c->pad_radius[0] = c->pad_radius[1] = 0;
    c->pad_ids.clear();
    c->curve_ws.release();
    c->planar.release();
    c->planar_version = 0;
    c->planar_pitch = c->planar_padx = c->planar_reach = 0;
    c->planar_phase.clear();
    c->launches_with_offsets = 0;
    c->d_planar_phase.release();
    c->phase_ring.release();
    c->yuv_in.release();
}

} // namespace
