// host_capi.cpp — C entry points over the host parameterisation, so that the Python plumbing (bench.py, tests) computes
// the kernel parameters with the very code the C++ Interpolator uses (params.cpp).
#include <cstring>
#include <exception>
#include <stdexcept>
#include <vector>

#include "../area_span.h"
#include "../linear_light.h"
#include "../native_taps.h"
#include "lenticular.h"
#include "params.h"
#include "y4m.h"

namespace {

// the error convention of the entry points below: the message into err (truncated to err_len − 1 bytes), -1
int report(const std::exception &e, char *err, size_t err_len)
{
    if(err && err_len)
    {
        std::strncpy(err, e.what(), err_len - 1);
        err[err_len - 1] = 0;
    }
    return -1;
}

} // namespace

extern "C" {

// Fills the caller's arrays: focused[N], offsets[N], weights[views*N], ids[32]; returns 0 or -1 (message in err).
int lfi_host_build_params(int cols, int rows, int width, int height, const char *trajectory, float focus, float range,
                          float effect, float aspect, int views, lfi_int2 *focused, lfi_float2 *offsets, uint16_t *weights,
                          int32_t *ids, int32_t *n_ids, int32_t block_radius[2], char *err, size_t err_len)
{
    try
    {
        lfi::Parameterizer p({cols, rows}, {width, height, 4});
        lfi::HostParams hp = p.build(trajectory, focus, range, effect, aspect, views);
        std::memcpy(focused, hp.focusedOffsets.data(), sizeof(lfi_int2) * hp.focusedOffsets.size());
        std::memcpy(offsets, hp.offsets.data(), sizeof(lfi_float2) * hp.offsets.size());
        std::memcpy(weights, hp.weights.data(), sizeof(uint16_t) * hp.weights.size());
        std::memcpy(ids, hp.focusMapIDs.data(), sizeof(int32_t) * hp.focusMapIDs.size());
        *n_ids = static_cast<int32_t>(hp.focusMapIDs.size());
        block_radius[0] = hp.blockRadius[0];
        block_radius[1] = hp.blockRadius[1];
        return 0;
    }
    catch(const std::exception &e)
    {
        return report(e, err, err_len);
    }
}

// per-view focus: out[views] = f0 + ((f1 − f0) / (views − 1))·i in float (views = 1: f0); returns 0, or -1 for views < 1
int lfi_host_focus_ramp(float f0, float f1, int views, float *out)
{
    if(views < 1 || !out)
        return -1;
    const std::vector<float> ramp = lfi::focusRamp(f0, f1, views);
    std::memcpy(out, ramp.data(), sizeof(float) * ramp.size());
    return 0;
}

// the focus candidates of lfi_focus_curve: out[steps] = fmaf(range / (steps − 1), i, focus) in float; returns 0, or -1 for steps < 2
int lfi_host_focus_candidates(float focus, float range, int steps, float *out)
{
    if(steps < 2 || !out)
        return -1;
    const std::vector<float> f = lfi::focusCandidates(focus, range, steps);
    std::memcpy(out, f.data(), sizeof(float) * f.size());
    return 0;
}

// tile (tx, ty) of lfi_focus_tiles' tiles_x × tiles_y grid over a width × height frame: rect = {x0, y0, x1, y1}; returns 0, or -1 for a grid
// outside [1, width] × [1, height] or a tile outside the grid
int lfi_host_focus_tile_rect(int width, int height, int tiles_x, int tiles_y, int tx, int ty, int32_t rect[4])
{
    if(!rect || tiles_x < 1 || tiles_y < 1 || tiles_x > width || tiles_y > height || tx < 0 || ty < 0 || tx >= tiles_x || ty >= tiles_y)
        return -1;
    const std::array<int, 4> r = lfi::focusTileRect(width, height, tiles_x, tiles_y, tx, ty);
    for(int k = 0; k < 4; k++)
        rect[k] = r[k];
    return 0;
}

// output pixel o of the area resize of lfi_download_quilt_scaled along one axis of src source pixels and dst output pixels (../area_span.h, the
// code the kernel runs): out = {first, last, w_first, w_last} — the source pixels o overlaps and the overlaps with the first and the last
// one; every source pixel between them weighs dst.  Returns 0, or -1 unless 1 <= dst <= src <= 65535 and 0 <= o < dst
int lfi_host_area_span(int src, int dst, int o, int32_t out[4])
{
    if(!out || dst < 1 || src < dst || static_cast<uint32_t>(src) > lfi::LFI_AREA_SPAN_MAX || o < 0 || o >= dst)
        return -1;
    const lfi::AreaSpan s = lfi::area_span(static_cast<uint32_t>(src), static_cast<uint32_t>(dst), static_cast<uint32_t>(o));
    out[0] = static_cast<int32_t>(s.first);
    out[1] = static_cast<int32_t>(s.last);
    out[2] = static_cast<int32_t>(s.w_first);
    out[3] = static_cast<int32_t>(s.w_last);
    return 0;
}

// the tables of linear-light blending (LFI_FLAG_LINEAR_LIGHT; ../linear_light.h, the bits the kernel loads): d16[256] the fp16 bit patterns of
// the decode table D, t32[256] the fp32 bit patterns of the thresholds T (entry 0 a placeholder).  Returns 0, or -1 for a NULL pointer
int lfi_host_linear_tables(uint16_t *d16, uint32_t *t32)
{
    if(!d16 || !t32)
        return -1;
    for(int b = 0; b < 256; b++)
        d16[b] = lfi::LINEAR_D16_BITS[b], t32[b] = lfi::LINEAR_T_BITS[b];
    return 0;
}

// out[i] = E(s[i]) for n fp32 sums, by the epilogue the kernel runs (../linear_light.h): the threshold array and the first-guess table set up as
// the kernel sets them up, then linear_encode.  Returns 0, or -1 for a NULL pointer
int lfi_host_linear_encode(const float *s, size_t n, uint8_t *out)
{
    if(!s || !out)
        return -1;
    static const struct Tables
    {
        float thr[257];
        uint8_t guess[lfi::LINEAR_CELLS];
        Tables()
        {
            for(int b = 0; b <= 256; b++)
                thr[b] = lfi::linear_threshold(b);
            for(int cell = 0; cell < lfi::LINEAR_CELLS; cell++)
                guess[cell] = lfi::linear_guess(thr, cell);
        }
    } tables;
    for(size_t i = 0; i < n; i++)
        out[i] = static_cast<uint8_t>(lfi::linear_encode(s[i], tables.guess, tables.thr));
    return 0;
}

// a lenticular display's calibration as the lens description of lfi_download_native (lenticular.h): pitch, slope, center, dpi and invert for
// an output of out_w × out_h pixels interlacing n views; returns 0 or -1 (message in err)
int lfi_host_lenticular(double pitch, double slope, double center, double dpi, int invert, int out_w, int out_h, int n, lfi_lenticular *out, char *err,
                        size_t err_len)
{
    try
    {
        if(!out)
            throw std::runtime_error("out must be non-NULL");
        lfi::LensCalibration c;
        c.pitch = pitch, c.slope = slope, c.center = center, c.dpi = dpi, c.invert = invert != 0;
        *out = lfi::lenticularFromCalibration(c, out_w, out_h, n);
        return 0;
    }
    catch(const std::exception &e)
    {
        return report(e, err, err_len);
    }
}

// lfi_host_lenticular from a display's calibration FILE (lenticular.h: a flat JSON object): the same arithmetic on the file's pitch, slope,
// center and DPI; invView becomes LFI_LENT_INVERT and flipSubp LFI_LENT_BGR in out->flags; screen = {screenW, screenH} as the file states
// them (0: not stated; may be NULL); returns 0 or -1 (message in err, naming the key at fault)
int lfi_host_lenticular_json(const char *path, int out_w, int out_h, int n, lfi_lenticular *out, int32_t screen[2], char *err, size_t err_len)
{
    try
    {
        if(!path || !out)
            throw std::runtime_error("path and out must be non-NULL");
        const lfi::LensFile file = lfi::lensCalibrationFromFile(path);
        *out = lfi::lenticularFromCalibration(file.lens, out_w, out_h, n);
        out->flags |= file.flags;
        if(screen)
            screen[0] = file.screenW, screen[1] = file.screenH;
        return 0;
    }
    catch(const std::exception &e)
    {
        return report(e, err, err_len);
    }
}

// output pixel o of lfi_download_native's bilinear tile sampling along one axis of src tile pixels and dst output pixels (../native_taps.h, the
// code the kernel runs): out = {p0, p1, f} — the two taps and the weight of p1 in 1/256.  Returns 0, or -1 unless 1 <= src, dst <= 65535 and
// 0 <= o < dst
int lfi_host_native_taps(int src, int dst, int o, int32_t out[3])
{
    if(!out || src < 1 || dst < 1 || src > 65535 || dst > 65535 || o < 0 || o >= dst)
        return -1;
    const lfi::NativeTaps t = lfi::native_taps(static_cast<uint32_t>(o), static_cast<uint32_t>(src), static_cast<uint32_t>(dst));
    out[0] = static_cast<int32_t>(t.p0);
    out[1] = static_cast<int32_t>(t.p1);
    out[2] = static_cast<int32_t>(t.f);
    return 0;
}

// the interval an all-focus render should search, from the tiles' best candidates of a search over [focus, focus + range] (--auto-range):
// the tiles chose from `steps` candidates (lfi_focus_tiles_steps: a multiple of 32 from 32 to 256), those of lfi_host_focus_candidates(focus,
// range, steps); the candidates kept are lo_hi = {max(min index − 1, 0), min(max index + 1, steps − 1)}, *out_focus = candidate lo,
// *out_range = candidate hi − candidate lo in float; returns 0, or -1 for no tiles, steps the tiles do not take, an index outside
// [0, steps − 1] or range <= 0
int lfi_host_focus_auto_range_steps(const int32_t *best_index, int tiles, int steps, float focus, float range, float *out_focus, float *out_range,
                                    int32_t lo_hi[2])
{
    if(!best_index || tiles < 1 || !out_focus || !out_range || !lo_hi || !(range > 0.0f))
        return -1;
    if(steps < LFI_FOCUS_TILE_STEPS || steps > 256 || steps % LFI_FOCUS_TILE_STEPS != 0)
        return -1;
    for(int t = 0; t < tiles; t++)
        if(best_index[t] < 0 || best_index[t] >= steps)
            return -1;
    const lfi::FocusAutoRange r = lfi::focusAutoRange(best_index, static_cast<size_t>(tiles), focus, range, steps);
    *out_focus = r.focus;
    *out_range = r.range;
    lo_hi[0] = r.lo;
    lo_hi[1] = r.hi;
    return 0;
}

// (the 32 candidates of lfi_focus_tiles)
int lfi_host_focus_auto_range(const int32_t *best_index, int tiles, float focus, float range, float *out_focus, float *out_range, int32_t lo_hi[2])
{
    return lfi_host_focus_auto_range_steps(best_index, tiles, LFI_FOCUS_TILE_STEPS, focus, range, out_focus, out_range, lo_hi);
}

// per-view focus: out_vn[views][N] = the focused offsets of Parameterizer::offsets at focus_v[v] (the rows lfi_set_view_offsets takes)
int lfi_host_build_view_offsets(int cols, int rows, int width, int height, const char *trajectory, float aspect, const float *focus_v,
                                int views, lfi_int2 *out_vn, char *err, size_t err_len)
{
    try
    {
        if(views < 1 || !focus_v || !out_vn)
            throw std::runtime_error("views must be positive and the arrays non-NULL");
        lfi::Parameterizer p({cols, rows}, {width, height, 4});
        const std::vector<lfi_int2> d = p.viewOffsets(aspect, std::vector<float>(focus_v, focus_v + views), p.interpretTrajectory(trajectory));
        std::memcpy(out_vn, d.data(), sizeof(lfi_int2) * d.size());
        return 0;
    }
    catch(const std::exception &e)
    {
        return report(e, err, err_len);
    }
}

// each view shifted about its own camera: offsets_vn / focused_vn [views][N] = Parameterizer::offsets at focus_v[v] for the trajectory
// collapsed onto camera v (the rows lfi_set_view_float_offsets / lfi_set_view_offsets take); either output may be NULL
int lfi_host_build_view_centred_offsets(int cols, int rows, int width, int height, const char *trajectory, float aspect, const float *focus_v,
                                        int views, lfi_float2 *offsets_vn, lfi_int2 *focused_vn, char *err, size_t err_len)
{
    try
    {
        if(views < 1 || !focus_v)
            throw std::runtime_error("views must be positive and focus_v non-NULL");
        lfi::Parameterizer p({cols, rows}, {width, height, 4});
        std::vector<lfi_float2> o;
        std::vector<lfi_int2> d;
        p.viewCentredOffsets(aspect, std::vector<float>(focus_v, focus_v + views), p.interpretTrajectory(trajectory), o, d);
        if(offsets_vn)
            std::memcpy(offsets_vn, o.data(), sizeof(lfi_float2) * o.size());
        if(focused_vn)
            std::memcpy(focused_vn, d.data(), sizeof(lfi_int2) * d.size());
        return 0;
    }
    catch(const std::exception &e)
    {
        return report(e, err, err_len);
    }
}

// each view's focus-map images: ids_vk[views][*n_ids] (room for views × 32), row v = the ids lfi_host_build_params selects for the trajectory
// collapsed onto camera v (the rows lfi_view_focus_maps takes)
int lfi_host_build_view_focus_ids(int cols, int rows, const char *trajectory, int views, int32_t *ids_vk, int32_t *n_ids, char *err, size_t err_len)
{
    try
    {
        if(views < 1 || !ids_vk || !n_ids)
            throw std::runtime_error("views must be positive and the arrays non-NULL");
        lfi::Parameterizer p({cols, rows}, {1, 1, 4});
        const std::vector<int32_t> ids = p.viewFocusMapIDs(p.interpretTrajectory(trajectory), views);
        std::memcpy(ids_vk, ids.data(), sizeof(int32_t) * ids.size());
        *n_ids = static_cast<int32_t>(ids.size() / views);
        return 0;
    }
    catch(const std::exception &e)
    {
        return report(e, err, err_len);
    }
}

// the Y4M writer (y4m.h): bytes of one I420 frame (0 for a size below 1), and n frames — frame k at frames + k·frame_stride_bytes — written
// as one file at fps_num:fps_den frames per second with XCOLORRANGE=FULL or LIMITED; returns 0 or -1 (message in err)
size_t lfi_host_y4m_frame_bytes(int width, int height)
{
    return lfi::y4mFrameBytes(width, height);
}

int lfi_host_y4m_write(const char *path, const uint8_t *frames, int n, size_t frame_stride_bytes, int width, int height, int fps_num, int fps_den, int full_range,
                       char *err, size_t err_len)
{
    try
    {
        if(!path)
            throw std::runtime_error("path must be non-NULL");
        lfi::writeY4m(path, frames, n, frame_stride_bytes, width, height, fps_num, fps_den, full_range != 0);
        return 0;
    }
    catch(const std::exception &e)
    {
        return report(e, err, err_len);
    }
}

// lfi_host_y4m_write with the chroma's siting: left_sited != 0 writes C420mpeg2 in place of C420jpeg
int lfi_host_y4m_write_sited(const char *path, const uint8_t *frames, int n, size_t frame_stride_bytes, int width, int height, int fps_num, int fps_den,
                             int full_range, int left_sited, char *err, size_t err_len)
{
    try
    {
        if(!path)
            throw std::runtime_error("path must be non-NULL");
        lfi::writeY4m(path, frames, n, frame_stride_bytes, width, height, fps_num, fps_den, full_range != 0, left_sited != 0);
        return 0;
    }
    catch(const std::exception &e)
    {
        return report(e, err, err_len);
    }
}

// the 10-bit twins (y4m.h: C420p10, I010 frames of twice the bytes).  lfi_host_y4m_write_deep writes frames of `depth` bits (8 or 10; 10 ignores
// left_sited: the tag has no siting); lfi_host_y4m_info_deep and lfi_host_y4m_read_deep accept C420p10 files beside the 8-bit ones, out[7] is
// the depth and the frames are frame_bytes·(depth == 10 ? 2 : 1) long
size_t lfi_host_y4m_frame_bytes_deep(int width, int height, int depth)
{
    return depth == 8 || depth == 10 ? lfi::y4mFrameBytes(width, height, depth) : 0;
}

int lfi_host_y4m_write_deep(const char *path, const uint8_t *frames, int n, size_t frame_stride_bytes, int width, int height, int fps_num, int fps_den,
                            int full_range, int left_sited, int depth, char *err, size_t err_len)
{
    try
    {
        if(!path)
            throw std::runtime_error("path must be non-NULL");
        if(depth != 8 && depth != 10)
            throw std::runtime_error("Y4M frames are written with 8 or 10 bits per sample");
        lfi::writeY4m(path, frames, n, frame_stride_bytes, width, height, fps_num, fps_den, full_range != 0, left_sited != 0, depth);
        return 0;
    }
    catch(const std::exception &e)
    {
        return report(e, err, err_len);
    }
}

int lfi_host_y4m_info_deep(const char *path, int32_t out[8], char *chroma_tag, size_t chroma_tag_len, char *err, size_t err_len)
{
    try
    {
        if(!path || !out)
            throw std::runtime_error("path and out must be non-NULL");
        lfi::Y4mReader reader(path, true);
        const lfi::Y4mInfo &info = reader.info();
        const int32_t values[8] = {info.width, info.height, info.fpsNum, info.fpsDen, info.frames, info.fullRange, info.centreSited ? 1 : 0, info.depth};
        std::memcpy(out, values, sizeof(values));
        if(chroma_tag && chroma_tag_len)
        {
            std::strncpy(chroma_tag, info.chroma.c_str(), chroma_tag_len - 1);
            chroma_tag[chroma_tag_len - 1] = 0;
        }
        return 0;
    }
    catch(const std::exception &e)
    {
        return report(e, err, err_len);
    }
}

int lfi_host_y4m_read_deep(const char *path, int first, int n, uint8_t *frames, size_t frame_stride_bytes, char *err, size_t err_len)
{
    try
    {
        if(!path)
            throw std::runtime_error("path must be non-NULL");
        lfi::Y4mReader reader(path, true);
        if(n < 0 || (n > 0 && (!frames || frame_stride_bytes < reader.frameBytes())))
            throw std::runtime_error("Y4M frames are missing or closer together than a frame's bytes (" + std::string(path) + ")");
        for(int k = 0; k < n; k++)
            reader.readFrame(first + k, frames + frame_stride_bytes * k);
        return 0;
    }
    catch(const std::exception &e)
    {
        return report(e, err, err_len);
    }
}

// y4mInputSiting (y4m.h): the siting (0 centre, 1 left) a file tagged C<chroma_tag> is read with under mode 0 centre, 1 left, 2 auto; -1 for
// a NULL tag or an unknown mode
int lfi_host_y4m_input_siting(const char *chroma_tag, int mode)
{
    if(!chroma_tag || mode < lfi::Y4M_SITE_CENTRE || mode > lfi::Y4M_SITE_AUTO)
        return -1;
    return lfi::y4mInputSiting(chroma_tag, mode);
}

// the Y4M reader (y4m.h): out = {width, height, fps_num, fps_den, frames, full_range (1, 0, -1: no XCOLORRANGE), centre_sited, 0}, the C tag
// without its C into chroma_tag (may be NULL); returns 0 or -1 (message in err)
int lfi_host_y4m_info(const char *path, int32_t out[8], char *chroma_tag, size_t chroma_tag_len, char *err, size_t err_len)
{
    try
    {
        if(!path || !out)
            throw std::runtime_error("path and out must be non-NULL");
        lfi::Y4mReader reader(path);
        const lfi::Y4mInfo &info = reader.info();
        const int32_t values[8] = {info.width, info.height, info.fpsNum, info.fpsDen, info.frames, info.fullRange, info.centreSited ? 1 : 0, 0};
        std::memcpy(out, values, sizeof(values));
        if(chroma_tag && chroma_tag_len)
        {
            std::strncpy(chroma_tag, info.chroma.c_str(), chroma_tag_len - 1);
            chroma_tag[chroma_tag_len - 1] = 0;
        }
        return 0;
    }
    catch(const std::exception &e)
    {
        return report(e, err, err_len);
    }
}

// frames [first, first + n) of a Y4M file, frame k at frames + k·frame_stride_bytes; returns 0 or -1 (message in err)
int lfi_host_y4m_read(const char *path, int first, int n, uint8_t *frames, size_t frame_stride_bytes, char *err, size_t err_len)
{
    try
    {
        if(!path)
            throw std::runtime_error("path must be non-NULL");
        lfi::Y4mReader reader(path);
        if(n < 0 || (n > 0 && (!frames || frame_stride_bytes < reader.frameBytes())))
            throw std::runtime_error("Y4M frames are missing or closer together than a frame's bytes (" + std::string(path) + ")");
        for(int k = 0; k < n; k++)
            reader.readFrame(first + k, frames + frame_stride_bytes * k);
        return 0;
    }
    catch(const std::exception &e)
    {
        return report(e, err, err_len);
    }
}

uint16_t lfi_host_float_to_half(float v)
{
    return lfi::floatToHalfBits(v);
}

float lfi_host_half_to_float(uint16_t h)
{
    return lfi::halfBitsToFloat(h);
}

} // extern "C"

// ---- image I/O and the loader, for the tests of the steps either side of the hot path ----------------------------------
#include "image_io.h"
#include "lfLoader.h"

extern "C" {

// decode a PNG / PPM into caller memory (RGBA8); call with rgba == NULL to query the size
int lfi_host_load_image(const char *path, int *width, int *height, uint8_t *rgba, char *err, size_t err_len)
{
    try
    {
        lfi::Image img = lfi::loadImage(path);
        *width = img.width;
        *height = img.height;
        if(rgba)
            std::memcpy(rgba, img.pixels.data(), img.pixels.size());
        return 0;
    }
    catch(const std::exception &e)
    {
        return report(e, err, err_len);
    }
}

int lfi_host_write_png(const char *path, int width, int height, int channels, const uint8_t *data, char *err, size_t err_len)
{
    try
    {
        lfi::writePng(path, width, height, channels, data, static_cast<size_t>(width) * channels);
        return 0;
    }
    catch(const std::exception &e)
    {
        return report(e, err, err_len);
    }
}

// LfLoader::loadData on a directory: returns cols/rows/resolution and (if planes != NULL) the images in g = col*rows+row order
int lfi_host_load_grid(const char *path, int *cols, int *rows, int *width, int *height, uint8_t *planes, char *err, size_t err_len)
{
    try
    {
        LfLoader loader;
        loader.loadData(path);
        const lfi::IVec2 cr = loader.getColsRows();
        const lfi::IVec3 res = loader.imageResolution();
        *cols = cr.x;
        *rows = cr.y;
        *width = res.x;
        *height = res.y;
        if(planes)
            for(int col = 0; col < cr.x; col++)
                for(int row = 0; row < cr.y; row++)
                    std::memcpy(planes + loader.imageSize() * (static_cast<size_t>(col) * cr.y + row), loader.image({col, row}).data(), loader.imageSize());
        return 0;
    }
    catch(const std::exception &e)
    {
        return report(e, err, err_len);
    }
}

// LfLoader on a directory of <row>_<col>.y4m files, a light-field video: out = {cols, rows, width, height, frames, full_range (1, 0, -1)},
// and (if frames != NULL) frame t of every camera, image g = col*rows + row at frames + g·frame_stride_bytes; returns 0 or -1 (message in err;
// a directory of images is refused here)
int lfi_host_load_grid_y4m(const char *path, int t, int32_t out[6], uint8_t *frames, size_t frame_stride_bytes, char *err, size_t err_len)
{
    try
    {
        if(!path || !out)
            throw std::runtime_error("path and out must be non-NULL");
        LfLoader loader;
        loader.loadData(path);
        if(!loader.isVideo())
            throw std::runtime_error(std::string("The directory ") + path + " holds images, not .y4m videos");
        if(loader.videoDepth() != 8)
            throw std::runtime_error(std::string("The directory ") + path + " holds 10-bit videos (C420p10): this call delivers 8-bit frames");
        const lfi::IVec2 cr = loader.getColsRows();
        const lfi::IVec3 res = loader.imageResolution();
        const int32_t values[6] = {cr.x, cr.y, res.x, res.y, loader.frameCount(), loader.videoFullRange()};
        std::memcpy(out, values, sizeof(values));
        if(frames)
            loader.loadFrames(t, frames, frame_stride_bytes);
        return 0;
    }
    catch(const std::exception &e)
    {
        return report(e, err, err_len);
    }
}

} // extern "C"
