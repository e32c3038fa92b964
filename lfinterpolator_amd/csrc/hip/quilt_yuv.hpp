// quilt_yuv.hpp — the scaled quilt as ONE 8-bit YUV 4:2:0 frame, made on the device without an RGBA quilt (lfi_download_quilt_yuv with even
// tile sizes): a frame of a quilt video.
//
// Definition (include/lfi.h): with Q the RGBA image of lfi_download_quilt_scaled — QW = tiles_x·tile_w by QH = tiles_y·tile_h, the exact area
// filter of quilt_scaled.hpp — the frame is what lfi_download_views_yuv420's definition (yuv420.hpp) makes of Q taken as one view.  No new
// arithmetic: quilt_scale_row (quilt_scaled.hpp) computes Q's pixels, yuv_luma and yuv_chroma (yuv420.hpp) convert them, YUV_COEFFS is the
// table.  With tile_w and tile_h EVEN every 2 × 2 block of Q lies inside one tile, and that is the only case this kernel takes; an odd tile
// size goes through quilt_scale and yuvs_convert (the entry point routes).
//
//   quilt_yuv_scale<PLANAR, FORMAT>  one workgroup (four waves) per (tile, band of 4 output rows, chunk of cols_per_wg ≤ 512 output columns),
//     quilt_scale's decomposition with cols_per_wg EVEN: bands start on even rows (4 and tile_h are even) and chunks on even columns, so no
//     2 × 2 block crosses a workgroup's rectangle.
//     Phase 1, per output row: quilt_scale_row, the code quilt_scale runs — vertical sums in registers, horizontal sums through 12 KiB of
//     LDS, the corrected quotient — leaves each thread the finished pixels of its columns oc0 + t and oc0 + t + 256.
//     Phase 2 replaces the RGBA store and needs no memory: a thread keeps the pixels of an even row in registers, and after the odd row
//     below it holds its column's two pixels of the row pair.  The chunk's first column is even, so lanes 2i and 2i + 1 of a wave hold the
//     two columns of ONE 2 × 2 block: every lane computes its two Y values (yuv_luma) and its column's sums of R, G and B, one DPP
//     quad-permute each (lanes 0 ↔ 1, 2 ↔ 3) hands them to the neighbour, and the EVEN lane stores the block: two Y bytes per row, and Cb
//     and Cr (yuv_chroma) of the four pixels' sums.  All 256 threads stay busy; there is no second LDS buffer and no further barrier.
//
// Where the bytes go.  fx = tcol·tile_w + oc0 + t (+ 256) is the even lane's FRAME column, even because tile_w, oc0 and t are; the pair's
// frame rows are fy = trow·tile_h + oy − 1 (even) and fy + 1 < QH, its chroma row fy / 2 < ch = QH / 2, its chroma column fx / 2 < cw = QW / 2.
//   Y      2 bytes at fx of rows fy and fy + 1:  plane base and y_pitch are even (multiples of 8), so the store is 2-byte aligned; fx + 2 ≤ QW ≤ y_pitch
//   I420   the single bytes fx / 2 of the Cb and the Cr row
//   NV12   2 bytes (Cb, Cr) at fx of the CbCr row: plane base and c_pitch are even; fx + 2 ≤ QW = 2·cw ≤ c_pitch
// A wave's 32 storing lanes write 64 (chroma I420: 32) contiguous bytes of a row per instruction.  Every block is written by exactly one
// lane, with stores no wider than the block: workgroups of neighbouring chunks and tiles never share a byte, there is no read of dst, no
// read-modify-write and no atomic, and bytes outside the planes' own (pitch padding, gaps) are never written.  The launches rely on even
// plane bases, offsets and pitches only — in-place surfaces have multiples of 16 throughout, the staged frame is yuv_geometry's.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "quilt_scaled.hpp"
#include "yuv420.hpp"

namespace lfi {

struct QuiltYuvArgs
{
    QuiltScaleArgs q; // quilt unused; first = 0: the whole quilt
    YuvSurfaces s;    // the one frame, written
    YuvCoeffs k;
};

// the value of the lane's neighbour in its pair: lanes 0 ↔ 1, 2 ↔ 3 of every quad
__device__ __forceinline__ uint32_t quilt_yuv_pair(const uint32_t v)
{
    return uint32_t(__builtin_amdgcn_mov_dpp(int(v), 0xB1, 0xf, 0xf, false)); // quad_perm [1, 0, 3, 2]
}

// One workgroup's rectangle of ONE tile — view v0 + v resized to tile `tile` of a frame s that is tiles_x tiles wide — both phases: the
// body of quilt_yuv_scale, and of the colour half of rgbd_yuv_scale (rgbd_yuv.hpp).  Called by every thread of the workgroup; col is its
// 12 KiB.  The arguments by VALUE: with references into the kernel's argument block the compiler keeps quilt_yuv_scale's I420
// instantiations at 102 / 76 registers instead of 96 / 72
template <bool PLANAR, int FORMAT>
__device__ __forceinline__ void quilt_yuv_tile(const QuiltScaleArgs q, const YuvSurfaces s, const YuvCoeffs kc, const int v, const int tile,
                                               const int tiles_x, uint32_t (*col)[QUILT_SCALE_PIECE])
{
    const uint32_t tw = q.tile_w, th = q.tile_h;
    const uint32_t t = threadIdx.x;
    const uint32_t trow = (uint32_t)(tile / tiles_x), tcol = (uint32_t)(tile % tiles_x);
    const uint8_t *view = q.src.base + (size_t)(q.v0 + v) * q.src.view_stride;
    QuiltScaleChunk c;
    if(!quilt_scale_chunk(q, c))
        return;
    const uint32_t oy0 = blockIdx.y * q.rows_per_wg, oy1 = min(oy0 + q.rows_per_wg, th); // both even
    const uint32_t fx0 = tcol * tw + c.oc0 + t;                                           // the frame column of the thread's first column
    const bool stores = !(t & 1u); // oc1 − oc0 is even: the lanes of a pair own their columns together

    uint32_t upper[2] = {};
    for(uint32_t oy = oy0; oy < oy1; oy++)
    {
        uint32_t out[2];
        quilt_scale_row<PLANAR>(q, view, col, c, oy, out);
        if(!(oy & 1u))
        {
            upper[0] = out[0], upper[1] = out[1];
            continue;
        }
        const uint32_t fy = trow * th + oy - 1u; // even; fy + 1 < QH
#pragma unroll
        for(int k = 0; k < 2; k++)
        {
            // the column's two pixels; every lane takes part in the exchange (a lane that owns no column holds alpha only and stores nothing)
            const uint32_t p0 = upper[k], p1 = out[k];
            const uint32_t y = yuv_luma(kc, p0 & 0xffu, (p0 >> 8) & 0xffu, (p0 >> 16) & 0xffu) |
                               (yuv_luma(kc, p1 & 0xffu, (p1 >> 8) & 0xffu, (p1 >> 16) & 0xffu) << 16);
            const uint32_t rb = (p0 & 0x00ff00ffu) + (p1 & 0x00ff00ffu); // ΣR | ΣB << 16 of the column: ≤ 510 each
            const uint32_t g = ((p0 >> 8) & 0xffu) + ((p1 >> 8) & 0xffu);
            const uint32_t y_n = quilt_yuv_pair(y), rb_n = quilt_yuv_pair(rb), g_n = quilt_yuv_pair(g);
            if(stores && c.own[k])
            {
                const uint32_t fx = fx0 + uint32_t(k) * QUILT_SCALE_THREADS; // even
                uint8_t *y_row = s.base + (size_t)fy * s.y_pitch + fx;
                *reinterpret_cast<uint16_t *>(y_row) = (uint16_t)((y & 0xffu) | ((y_n & 0xffu) << 8));
                *reinterpret_cast<uint16_t *>(y_row + s.y_pitch) = (uint16_t)(((y >> 16) & 0xffu) | ((y_n >> 16) << 8));
                const uint32_t sum = rb + rb_n, sr = sum & 0xffffu, sb = sum >> 16, sg = g + g_n; // over the four pixels: ≤ 1020
                const uint32_t cb = yuv_chroma(kc.cb, sr, sg, sb), cr = yuv_chroma(kc.cr, sr, sg, sb);
                const size_t c_row = (size_t)(fy >> 1) * s.c_pitch;
                if constexpr(FORMAT == YUVS_NV12)
                    *reinterpret_cast<uint16_t *>(s.base + s.c_offset + c_row + fx) = (uint16_t)(cb | (cr << 8));
                else
                {
                    s.base[s.c_offset + c_row + (fx >> 1)] = (uint8_t)cb;
                    s.base[s.cr_offset + c_row + (fx >> 1)] = (uint8_t)cr;
                }
            }
        }
    }
}

template <bool PLANAR, int FORMAT>
__global__ void __launch_bounds__(QUILT_SCALE_THREADS) quilt_yuv_scale(const QuiltYuvArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t col[3][QUILT_SCALE_PIECE];
    const QuiltScaleArgs &q = a.q;
    const int i = blockIdx.z;
    quilt_yuv_tile<PLANAR, FORMAT>(q, a.s, a.k, i, i, q.tiles_x, col);
}

// Enqueues the ONE quilt_yuv_scale launch for the n = tiles_x·tiles_y tiles of a quilt.  The caller has checked what launch_quilt_scale's
// caller checks, that tile_w and tile_h are even, and that a.s describes one frame of tiles_x·tile_w × tiles_y·tile_h the device may write,
// aligned as the header says.
inline hipError_t launch_quilt_yuv_scale(hipStream_t stream, const bool planar, const int format, QuiltYuvArgs a, const int n)
{
    const dim3 grid = quilt_scale_plan(a.q, n, true), block(QUILT_SCALE_THREADS); // quilt_scale's decomposition, chunks of an even width
    if(planar)
    {
        if(format == YUVS_NV12)
            hipLaunchKernelGGL((quilt_yuv_scale<true, YUVS_NV12>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((quilt_yuv_scale<true, YUVS_I420>), grid, block, 0, stream, a);
    }
    else
    {
        if(format == YUVS_NV12)
            hipLaunchKernelGGL((quilt_yuv_scale<false, YUVS_NV12>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((quilt_yuv_scale<false, YUVS_I420>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

} // namespace lfi
