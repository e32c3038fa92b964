// yuv_surfaces.hpp — the YUV 4:2:0 kernels, over SURFACES: I420 or NV12 planes with a pitch, at offsets inside a frame, frames a stride apart —
// the staged frames of a host call (lfi_upload_images_yuv420, lfi_download_views_yuv420, lfi_render_stream_yuv420 and the host side of
// lfi_upload_images_yuv, lfi_download_views_yuv) or the caller's own device surfaces, read and written in place.  The arithmetic is that of
// yuv420.hpp (views → frames) and yuv420_upload.hpp (frames → images): their tables, yuv_in_pixel / yuv_in_clamp, yuv_luma / yuv_chroma and
// their inline pieces; this header says where the bytes lie.
//
// Geometry (include/lfi.h).  cw = (W + 1) >> 1, ch = (H + 1) >> 1.  The Y plane is H rows of y_pitch ≥ W bytes.  I420: Cb at c_offset, Cr at
// cr_offset, ch rows of c_pitch ≥ cw bytes each.  NV12: one plane at c_offset, ch rows of c_pitch ≥ 2·cw bytes, byte 2·cx Cb, 2·cx + 1 Cr.
//
// Decomposition, the same in both kernels: one launch for all frames of a chunk or views of a call (the frame or view is grid.z).  A lane
// owns a block of 8 columns × 2 rows; a wave is 64 neighbouring blocks of ONE block row (512 pixel columns), so the row's offsets are
// wave-uniform and neighbouring lanes touch neighbouring words of a row; a workgroup is four waves = four block rows.  No LDS, no atomics,
// no scratch.
//
// What the launches rely on (the entry points see to it): every plane base and the frame stride are multiples of 8, y_pitch is a multiple
// of 8, c_pitch a multiple of 4 (I420) or 8 (NV12) — in-place surfaces have multiples of 16 throughout, the staged planes are those of
// yuv_geometry (NV12: chroma rows of y_pitch bytes).  Then every load and every word store is aligned and lies inside its own row:
//   Y      8 bytes at 8·bx:            8·bx + 8 ≤ round8(W) ≤ y_pitch
//   I420   the dword at 4·bx:          4·bx + 4 ≤ round4(cw) ≤ c_pitch; the dword right of it only where bx + 1 < blocks_x
//   NV12   8 bytes at 8·bx:            8·bx + 8 ≤ round8(2·cw) ≤ c_pitch; the dword right of it only where bx + 1 < blocks_x, and then
//                                      2·cw ≥ 8·bx + 10, so 8·bx + 12 ≤ round4(2·cw) ≤ c_pitch
// and rows are clamped to the plane's own (an odd H has no Y row 2·ch − 1).
//
//   yuvs_expand<FORMAT, NEAREST>   frames → RGBA images.  A lane reads two 8-byte pieces of Y and its four chroma columns of chroma row by:
//     I420 the dword at 4·bx of each chroma plane, NV12 ONE 8-byte load of the CbCr row.  BILINEAR reads them on rows by − 1, by, by + 1
//     (clamped) and on each also the dword left of them (I420: its top byte is column 4·bx − 1; NV12: its upper two bytes) and the dword
//     right of them (its lowest byte, NV12 its lower two: column 4·bx + 4).  The bytes go into the two six-byte windows of yuv_in_columns /
//     yuv_in_row, so the definition's clamp is the same set of byte positions, computed once.  A wave's Y loads are two runs of 512 bytes,
//     its chroma loads runs of 256 (NV12: 512) bytes that neighbouring lanes share (the repeats hit in cache), its stores two runs of
//     2 KiB as 16-byte stores.  NO value comes from padding or from outside [0, cw − 1] × [0, ch − 1] — a host call copies only the
//     frames' own bytes into the staged planes, and in-place padding is the caller's and may hold anything: the chroma neighbours are
//     clamped as the definition says (a clamped neighbour is a byte of the lane's own columns or row), and the Y bytes beyond the image
//     belong to pixels that are not stored.  Ragged blocks, an odd last row, and images whose rows are not 16-byte aligned (W no multiple
//     of 4) store pixel by pixel as dwords; no lane stores outside the image.
//     Loads, clamps and arithmetic are yuvs_block_pixels, which ends with the block's 16 RGBA dwords; the kernel adds the stores.
//     yuvs_derived_expand (yuv_derived.hpp) calls the same function and puts the pixels into the planar copy of the inputs instead.
//   yuvs_convert<PLANAR, FORMAT>   views → frames.  From RGBA views a lane reads two rows of 32 bytes as 16-byte loads (a wave: two runs of
//     2 KiB), from PLANAR views 3 planes × 2 rows × 8 bytes at the plane pitch (six runs of 512 bytes; no RGBA copy of planar views).
//     Ragged blocks, and RGBA views whose rows are not 16-byte aligned, read pixel by pixel with clamped coordinates; planar rows are as
//     long as their pitch (a multiple of 128 ≥ round8(W)), so the 8-byte loads stay inside the row and the bytes beyond the view are
//     replaced by the last column's: an odd last column or row is replicated, as the definition's clamp says.  It writes ONLY the planes'
//     own bytes — pitch padding keeps its value: every whole block stores words (Y two 8-byte pieces, a wave's run 512 bytes; I420 a dword
//     each of Cb and Cr, runs of 256; NV12 one interleaved 8-byte piece), a ragged last block of a row stores its valid bytes one by one,
//     and a row beyond H is not stored.
//
// LEFT-SITED chroma (lfi_set_yuv_siting; MPEG-2 / H.264 siting, include/lfi.h) has kernels of its own names — tests pin the number of
// yuvs_expand and yuvs_convert bodies — that ARE the bodies above (yuvs_expand_block, yuvs_convert_block) with the filter as a template
// parameter; decomposition, alignment contract, loads of Y and of the views, and every store are the same.
//   yuvs_convert_left<PLANAR, FORMAT>   chroma column i of a lane is v(2i − 1) + 2·v(2i) + v(2i + 1), v(k) the two-row sum of block column k.
//     The one value from outside the block, v(−1), is the left neighbour lane's column 7: its three sums (≤ 510 each) packed into one dword
//     cross with ONE DPP move (wave_shr:1) — no second read of the view.  Lane 0 of a wave with bx > 0 loads pixel column x0 − 1 itself (inside
//     the view: x0 − 1 < W, rows ya and yb); bx = 0 clamps to its own column 0.  The clamp on the right is a column yuv_load_block replicated.
//   yuvs_expand_left<FORMAT>            BILINEAR only (NEAREST is the same bytes under either siting: yuvs_expand<FORMAT, true> is launched).
//     The window of yuv_in_columns / yuv_in_row without its left column: [own four | column 4bx + 4], one load fewer per chroma row and
//     plane; the dword right of the lane's own is read only where bx + 1 < blocks_x, as above, and a clamped column is a byte of the lane's own.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "views_src.hpp"
#include "yuv420.hpp"
#include "yuv420_upload.hpp"

namespace lfi {

struct YuvsInArgs
{
    YuvSurfaces s;       // read only
    uint8_t *dst;        // RGBA plane [H][W] of the first image
    size_t image_stride; // bytes from image to image
    uint32_t W, H, cw, ch;
    uint32_t blocks_x; // (W + 7) / 8
    uint32_t rows16;   // every pixel row of an image starts on a 16-byte boundary (W a multiple of 4)
    YuvInCoeffs k;
};

struct YuvsOutArgs
{
    ViewsSrc src;  // frame i is made of view i
    YuvSurfaces s; // written
    uint32_t cw, ch;
    uint32_t blocks_x; // (W + 7) / 8
    uint32_t rows16;   // RGBA: every pixel row starts on a 16-byte boundary (W a multiple of 4)
    YuvCoeffs k;
};

// NV12: bytes 0, 2 (p = 0: Cb) or 1, 3 (p = 1: Cr) of lo, then of hi
__device__ __forceinline__ uint32_t yuvs_component(const uint32_t lo, const uint32_t hi, const int p)
{
    const uint32_t a = lo >> (8 * p), b = hi >> (8 * p);
    return (a & 0xffu) | ((a >> 8) & 0xff00u) | ((b & 0xffu) << 16) | ((b << 8) & 0xff000000u);
}

// The RGBA dwords px of block (bx, by) of a frame: bx < a.blocks_x, by < a.ch.  Everything yuvs_expand reads and computes — its loads, its
// clamps, its arithmetic —, for the kernels that differ only in where the pixels go: yuvs_expand (the RGBA planes) and yuvs_derived_expand
// (yuv_derived.hpp: the planar copy).  Columns beyond W and the second row of an odd H's last block row hold values that are never stored.
template <int FORMAT, bool NEAREST, bool LEFT = false>
__device__ __forceinline__ void yuvs_block_pixels(const YuvsInArgs &a, const uint8_t *frame, const uint32_t bx, const uint32_t by, uint32_t (&px)[2][8])
{
    const uint32_t x0 = bx * YUV_BLOCK_W, ya = by * YUV_BLOCK_H; // x0 < W, ya < H
    const bool two_rows = ya + 1u < a.H;                         // an odd H's last block row has one pixel row
    const uint8_t *c_plane = frame + a.s.c_offset; // I420: Cb; NV12: CbCr
    // Y: row ya and row ya + 1 (clamped to the plane: its pixels are not stored then), columns x0 … x0 + 7
    uint32_t y[2][8];
    yuv_in_bytes(*reinterpret_cast<const uint2 *>(frame + (size_t)ya * a.s.y_pitch + x0), y[0]);
    yuv_in_bytes(*reinterpret_cast<const uint2 *>(frame + (size_t)(two_rows ? ya + 1u : ya) * a.s.y_pitch + x0), y[1]);
    // chroma in sixteenths of the 16 pixels
    int32_t su[2][8], sv[2][8];
    if constexpr(NEAREST)
    {
        uint32_t u, v;
        if constexpr(FORMAT == YUVS_NV12)
        {
            const uint2 c = *reinterpret_cast<const uint2 *>(c_plane + (size_t)by * a.s.c_pitch + 8u * bx);
            u = yuvs_component(c.x, c.y, 0), v = yuvs_component(c.x, c.y, 1);
        }
        else
        {
            u = *reinterpret_cast<const uint32_t *>(c_plane + (size_t)by * a.s.c_pitch + 4u * bx);
            v = *reinterpret_cast<const uint32_t *>(frame + a.s.cr_offset + (size_t)by * a.s.c_pitch + 4u * bx);
        }
#pragma unroll
        for(int i = 0; i < 8; i++)
            su[0][i] = su[1][i] = 16 * (int32_t)((u >> (8 * (i >> 1))) & 0xffu), sv[0][i] = sv[1][i] = 16 * (int32_t)((v >> (8 * (i >> 1))) & 0xffu);
    }
    else
    {
        // LEFT: the window without its left column — five columns, one load fewer per chroma row
        uint32_t sh[LEFT ? 5 : 6];
        if constexpr(LEFT)
            yuv_in_columns_left(bx, a.cw, sh);
        else
            yuv_in_columns(bx, a.cw, sh);
        constexpr int OWN = LEFT ? 0 : 8; // the bit of the window at which the lane's own four columns begin
        const bool has_l = !LEFT && bx > 0, has_r = bx + 1u < a.blocks_x;
        // rows by − 1, by, by + 1, clamped to [0, ch − 1]
        const uint32_t rows[3] = {by > 0 ? by - 1u : 0u, by, by + 1u < a.ch ? by + 1u : a.ch - 1u};
        int32_t hu[3][8], hv[3][8];
#pragma unroll
        for(int r = 0; r < 3; r++)
        {
            // the windows [column 4bx − 1 | own four | column 4bx + 4] of Cb and Cr; a column that does not exist reads as 0 and is never
            // selected (yuv_in_columns)
            uint64_t win[2];
            if constexpr(FORMAT == YUVS_NV12)
            {
                const uint8_t *row = c_plane + (size_t)rows[r] * a.s.c_pitch + 8u * bx;
                const uint2 own = *reinterpret_cast<const uint2 *>(row);
                uint32_t left = 0u;
                if constexpr(!LEFT)
                    left = has_l ? *reinterpret_cast<const uint32_t *>(row - 4) : 0u;
                const uint32_t right = has_r ? *reinterpret_cast<const uint32_t *>(row + 8) : 0u;
#pragma unroll
                for(int p = 0; p < 2; p++)
                    win[p] = (uint64_t)((left >> (16 + 8 * p)) & 0xffu) | ((uint64_t)yuvs_component(own.x, own.y, p) << OWN) |
                             ((uint64_t)((right >> (8 * p)) & 0xffu) << (32 + OWN));
            }
            else
            {
#pragma unroll
                for(int p = 0; p < 2; p++)
                {
                    const uint32_t *row = reinterpret_cast<const uint32_t *>(frame + (p ? a.s.cr_offset : a.s.c_offset) + (size_t)rows[r] * a.s.c_pitch) + bx;
                    uint32_t left = 0u;
                    if constexpr(!LEFT)
                        left = has_l ? row[-1] : 0u;
                    const uint32_t own = row[0], right = has_r ? row[1] : 0u;
                    win[p] = (uint64_t)(left >> 24) | ((uint64_t)own << OWN) | ((uint64_t)(right & 0xffu) << (32 + OWN));
                }
            }
            if constexpr(LEFT)
                yuv_in_row_left(win[0], sh, hu[r]), yuv_in_row_left(win[1], sh, hv[r]);
            else
                yuv_in_row(win[0], sh, hu[r]), yuv_in_row(win[1], sh, hv[r]);
        }
        // 9·a + 3·b + 3·c + d = 3·(3a + b) + (3c + d): an even row's neighbour row is the one above, an odd row's the one below (LEFT: the
        // rows' h are in quarters, 3·h(cy) + h(ny))
#pragma unroll
        for(int j = 0; j < 2; j++)
#pragma unroll
            for(int i = 0; i < 8; i++)
                su[j][i] = 3 * hu[1][i] + hu[j ? 2 : 0][i], sv[j][i] = 3 * hv[1][i] + hv[j ? 2 : 0][i];
    }
#pragma unroll
    for(int j = 0; j < 2; j++)
#pragma unroll
        for(int i = 0; i < 8; i++)
            px[j][i] = yuv_in_pixel(a.k, (int32_t)y[j][i], su[j][i], sv[j][i]);
}

template <int FORMAT, bool NEAREST, bool LEFT>
__device__ __forceinline__ void yuvs_expand_block(const YuvsInArgs &a)
{
    const uint32_t bx = blockIdx.x * YUV_LANES_X + threadIdx.x;
    const uint32_t by = blockIdx.y * YUV_BLOCK_ROWS + threadIdx.y; // wave-uniform
    if(bx >= a.blocks_x || by >= a.ch)
        return;
    const uint32_t x0 = bx * YUV_BLOCK_W, ya = by * YUV_BLOCK_H; // x0 < W, ya < H
    uint32_t px[2][8];
    yuvs_block_pixels<FORMAT, NEAREST, LEFT>(a, a.s.base + (size_t)blockIdx.z * a.s.frame_stride, bx, by, px);
    uint32_t *out = reinterpret_cast<uint32_t *>(a.dst + (size_t)blockIdx.z * a.image_stride) + (size_t)ya * a.W + x0;
    yuv_in_store(out, a.W, x0, ya + 1u < a.H, a.rows16, px);
}

template <int FORMAT, bool NEAREST>
__global__ void __launch_bounds__(YUV_LANES_X *YUV_BLOCK_ROWS) yuvs_expand(const YuvsInArgs a)
{
    yuvs_expand_block<FORMAT, NEAREST, false>(a);
}

// left-sited chroma, BILINEAR (NEAREST is yuvs_expand's under either siting)
template <int FORMAT>
__global__ void __launch_bounds__(YUV_LANES_X *YUV_BLOCK_ROWS) yuvs_expand_left(const YuvsInArgs a)
{
    yuvs_expand_block<FORMAT, false, true>(a);
}

template <bool PLANAR, int FORMAT, bool LEFT>
__device__ __forceinline__ void yuvs_convert_block(const YuvsOutArgs &a)
{
    const uint32_t bx = blockIdx.x * YUV_LANES_X + threadIdx.x;
    const uint32_t by = blockIdx.y * YUV_BLOCK_ROWS + threadIdx.y; // wave-uniform
    if(bx >= a.blocks_x || by >= a.ch)
        return;
    const uint32_t x0 = bx * YUV_BLOCK_W;
    const bool two_rows = by * YUV_BLOCK_H + 1u < a.src.H;
    const uint32_t ya = by * YUV_BLOCK_H, yb = two_rows ? ya + 1u : ya; // ya < H: by < ch
    const bool whole = x0 + YUV_BLOCK_W <= a.src.W;                       // all 8 columns inside the view
    uint32_t r[2][8], g[2][8], b[2][8];
    const uint8_t *view = a.src.base + (size_t)blockIdx.z * a.src.view_stride;
    // LEFT: lane 0 of a wave has no lane to its left and loads pixel column x0 − 1 itself (bx > 0: it lies inside the view) — issued here, ahead
    // of the block's own loads and added up only where the chroma needs it, so that it costs the wave no memory round trip of its own
    [[maybe_unused]] YuvColumn<PLANAR> edge{};
    if constexpr(LEFT)
        if(threadIdx.x == 0 && bx)
            edge = yuv_load_column<PLANAR>(view, a.src.W, a.src.H, a.src.pitch, x0 - 1u, ya, yb);
    yuv_load_block<PLANAR>(view, a.src.W, a.src.H, a.src.pitch, a.rows16, x0, ya, yb, whole, r, g, b);
    uint8_t *frame = a.s.base + (size_t)blockIdx.z * a.s.frame_stride;
    // Y: the row's own bytes only, and no row beyond H
#pragma unroll
    for(int j = 0; j < 2; j++)
    {
        uint32_t y[8];
#pragma unroll
        for(int i = 0; i < 8; i++)
            y[i] = yuv_luma(a.k, r[j][i], g[j][i], b[j][i]);
        uint8_t *row = frame + (size_t)(ya + j) * a.s.y_pitch + x0;
        if(j && !two_rows)
            continue;
        if(whole)
            *reinterpret_cast<uint2 *>(row) = uint2{y[0] | (y[1] << 8) | (y[2] << 16) | (y[3] << 24), y[4] | (y[5] << 8) | (y[6] << 16) | (y[7] << 24)};
        else
        {
#pragma unroll
            for(int i = 0; i < 7; i++) // a ragged block holds at most 7 columns
                if(x0 + i < a.src.W)
                    row[i] = (uint8_t)y[i];
        }
    }
    uint32_t cb[4], cr[4];
    if constexpr(LEFT)
    {
        // The one value from outside the block: the two-row sums of pixel column x0 − 1, the left neighbour lane's column 7, which that lane
        // holds in registers — ONE cross-lane move (DPP wave_shr:1: lane l takes lane l − 1's) in place of a second read of the view.  The
        // move stands behind the early return: the lanes with bx ≥ blocks_x are off, but a source lane bx − 1 < bx is always on, and it is
        // always a whole block (8·bx ≤ W − 1), so its column 7 is pixel column x0 − 1 and no replicated one.  Lane 0 of a wave has no
        // source lane and keeps `old`: it takes the column x0 − 1 it loaded above, or clamps to its own column 0 where bx = 0
        const uint32_t mine = yuv_pack_sums(r[0][7] + r[1][7], g[0][7] + g[1][7], b[0][7] + b[1][7]);
        uint32_t left = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mine, 0x138, 0xf, 0xf, false);
        if(threadIdx.x == 0)
            left = bx ? yuv_column_sums<PLANAR>(edge)
                      : yuv_pack_sums(r[0][0] + r[1][0], g[0][0] + g[1][0], b[0][0] + b[1][0]);
        // xr = min(2cx + 1, W − 1) is a column of the block: yuv_load_block has replicated the last column into those beyond the view
#pragma unroll
        for(int i = 0; i < 4; i++)
            yuv_block_chroma_left(a.k, r, g, b, left, i, cb[i], cr[i]);
    }
    else
    {
#pragma unroll
        for(int i = 0; i < 4; i++)
            yuv_block_chroma(a.k, r, g, b, i, cb[i], cr[i]);
    }
    const uint32_t c0 = 4u * bx; // < cw: x0 < W
    const bool c_whole = c0 + 4u <= a.cw;
    if constexpr(FORMAT == YUVS_NV12)
    {
        uint8_t *row = frame + a.s.c_offset + (size_t)by * a.s.c_pitch + 8u * bx;
        if(c_whole)
            *reinterpret_cast<uint2 *>(row) = uint2{cb[0] | (cr[0] << 8) | (cb[1] << 16) | (cr[1] << 24), cb[2] | (cr[2] << 8) | (cb[3] << 16) | (cr[3] << 24)};
        else
        {
#pragma unroll
            for(int i = 0; i < 3; i++)
                if(c0 + i < a.cw)
                    row[2 * i] = (uint8_t)cb[i], row[2 * i + 1] = (uint8_t)cr[i];
        }
    }
    else
    {
        uint8_t *u_row = frame + a.s.c_offset + (size_t)by * a.s.c_pitch + c0, *v_row = frame + a.s.cr_offset + (size_t)by * a.s.c_pitch + c0;
        if(c_whole)
        {
            *reinterpret_cast<uint32_t *>(u_row) = cb[0] | (cb[1] << 8) | (cb[2] << 16) | (cb[3] << 24);
            *reinterpret_cast<uint32_t *>(v_row) = cr[0] | (cr[1] << 8) | (cr[2] << 16) | (cr[3] << 24);
        }
        else
        {
#pragma unroll
            for(int i = 0; i < 3; i++)
                if(c0 + i < a.cw)
                    u_row[i] = (uint8_t)cb[i], v_row[i] = (uint8_t)cr[i];
        }
    }
}

template <bool PLANAR, int FORMAT>
__global__ void __launch_bounds__(YUV_LANES_X *YUV_BLOCK_ROWS) yuvs_convert(const YuvsOutArgs a)
{
    yuvs_convert_block<PLANAR, FORMAT, false>(a);
}

// left-sited chroma
template <bool PLANAR, int FORMAT>
__global__ void __launch_bounds__(YUV_LANES_X *YUV_BLOCK_ROWS) yuvs_convert_left(const YuvsOutArgs a)
{
    yuvs_convert_block<PLANAR, FORMAT, true>(a);
}

inline dim3 yuvs_grid(const uint32_t blocks_x, const uint32_t ch, const int n)
{
    return dim3((blocks_x + YUV_LANES_X - 1) / YUV_LANES_X, (ch + YUV_BLOCK_ROWS - 1) / YUV_BLOCK_ROWS, n);
}

// Enqueues the ONE yuvs_expand launch for n frames.  The caller has checked sizes, alignment and memory: n ≥ 1, a.s describes n frames the
// device may read, a.dst holds n images.
inline hipError_t launch_yuvs_expand(hipStream_t stream, const int format, const bool nearest, const bool left, const YuvsInArgs &a, const int n)
{
    const dim3 grid = yuvs_grid(a.blocks_x, a.ch, n), block(YUV_LANES_X, YUV_BLOCK_ROWS);
    if(left && !nearest) // a left-sited nearest upload is the nearest kernel: the same bytes
    {
        if(format == YUVS_NV12)
            hipLaunchKernelGGL((yuvs_expand_left<YUVS_NV12>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((yuvs_expand_left<YUVS_I420>), grid, block, 0, stream, a);
    }
    else if(format == YUVS_NV12)
    {
        if(nearest)
            hipLaunchKernelGGL((yuvs_expand<YUVS_NV12, true>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((yuvs_expand<YUVS_NV12, false>), grid, block, 0, stream, a);
    }
    else
    {
        if(nearest)
            hipLaunchKernelGGL((yuvs_expand<YUVS_I420, true>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((yuvs_expand<YUVS_I420, false>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

// Enqueues the ONE yuvs_convert launch for n views.  The caller has checked sizes, alignment and memory: a.s describes n frames the device
// may write.
inline hipError_t launch_yuvs_convert(hipStream_t stream, const bool planar, const int format, const bool left, const YuvsOutArgs &a, const int n)
{
    const dim3 grid = yuvs_grid(a.blocks_x, a.ch, n), block(YUV_LANES_X, YUV_BLOCK_ROWS);
    if(left)
    {
        if(planar)
        {
            if(format == YUVS_NV12)
                hipLaunchKernelGGL((yuvs_convert_left<true, YUVS_NV12>), grid, block, 0, stream, a);
            else
                hipLaunchKernelGGL((yuvs_convert_left<true, YUVS_I420>), grid, block, 0, stream, a);
        }
        else
        {
            if(format == YUVS_NV12)
                hipLaunchKernelGGL((yuvs_convert_left<false, YUVS_NV12>), grid, block, 0, stream, a);
            else
                hipLaunchKernelGGL((yuvs_convert_left<false, YUVS_I420>), grid, block, 0, stream, a);
        }
    }
    else if(planar)
    {
        if(format == YUVS_NV12)
            hipLaunchKernelGGL((yuvs_convert<true, YUVS_NV12>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((yuvs_convert<true, YUVS_I420>), grid, block, 0, stream, a);
    }
    else
    {
        if(format == YUVS_NV12)
            hipLaunchKernelGGL((yuvs_convert<false, YUVS_NV12>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((yuvs_convert<false, YUVS_I420>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

} // namespace lfi
