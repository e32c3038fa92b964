// quilt_scaled.hpp — the quilt with every view resized to a tile size on the device (lfi_download_quilt[_tiles]_scaled): an exact area
// (box) resize, downscaling or identity, each axis on its own.
//
// Definition (include/lfi.h): a view of W × H pixels becomes a tile of tile_w × tile_h; the weights wx(ox, sx), wy(oy, sy) are the integer
// overlaps of ../area_span.h, and per colour channel  out = (Σ_sy Σ_sx wy·wx·p[sy][sx] + W·H / 2) / (W·H)  in integers; alpha is 255.
// Every sum is an integer, so the result is exact in any order.
//
//   quilt_scale<PLANAR>  one workgroup (four waves) per (tile, band of rows_per_wg output rows, chunk of cols_per_wg ≤ 512 output columns).
//     Per output row the workgroup walks the chunk's source columns [s0, s1) in pieces of 1024 pixels (ONE piece where the launch code can
//     arrange it, which is every ratio below 1019 : 1): a lane owns four adjacent source pixels of the piece, reads them from every source
//     row of the output row's span with one 16-byte load (RGBA planes) or one dword load per colour plane (PLANAR: the byte planes are
//     read as they are, there is no RGBA copy) — a wave reads 1 KiB / 3 × 256 B of contiguous bytes per instruction — and keeps the
//     vertical sums Σ wy·p per pixel and channel in twelve registers (u32: ≤ 255·H).  The lane sums go to LDS (3 × 1024 u32), and thread t
//     then adds up the horizontal spans of output columns t and t + 256 of the chunk out of LDS (u64: ≤ 255·W·H), carries them over the
//     pieces in registers, divides and stores one RGBA pixel per column: neighbouring threads, neighbouring dwords of the quilt.
//     A source row that two output rows share is read once for each of them — by the same workgroup back to back unless the band ends
//     between them; nothing else is read twice, and lanes past the chunk's last source column do not load.  No atomics.
//   quilt_scale_chunk, quilt_scale_row  the chunk's columns and spans, and one output row of it up to the finished pixels: what quilt_scale
//     runs before its store, and what quilt_yuv_scale (quilt_yuv.hpp) runs before it converts the pixels to YUV 4:2:0 instead.
//   The division: q = ⌊n / A⌋ with n < 256·A is estimated in float (relative error < 2⁻²¹, so the estimate is off by one at most) and
//     corrected with two exact u64 products.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../area_span.h"
#include "views_src.hpp"

namespace lfi {

constexpr int QUILT_SCALE_THREADS = 256;
constexpr int QUILT_SCALE_PIECE = QUILT_SCALE_THREADS * 4; // source pixels per piece: four per lane
constexpr int QUILT_SCALE_COLS = QUILT_SCALE_THREADS * 2;  // output columns per workgroup at most: two per thread
constexpr int QUILT_SCALE_ROWS = 4;                        // output rows per workgroup

struct QuiltScaleArgs
{
    ViewsSrc src;    // the context's views: tile i is made of view v0 + i
    uint32_t *quilt; // RGBA image of the rows of tiles these tiles touch, tiles_x·tile_w pixels wide
    uint32_t tile_w, tile_h;
    int32_t v0, first, tiles_x;
    uint32_t cols_per_wg; // ≤ QUILT_SCALE_COLS
    uint32_t rows_per_wg;
    float rcp_area; // 1 / (W·H) in float, for the estimate of the quotient
};

using quilt_u32x4 = uint32_t __attribute__((ext_vector_type(4)));
// a pixel row of an RGBA plane starts at a multiple of 4 bytes only (W·4 bytes per row, any W)
struct __attribute__((packed, aligned(4))) quilt_px4
{
    quilt_u32x4 v;
};

// The chunk of a workgroup along x: its output columns [oc0, oc1) of the tile, the source columns [s0, s1) they overlap (s0 rounded down to
// a lane's four pixels), and the spans of the thread's two output columns oc0 + t and oc0 + t + 256 (own[k]: the column is the chunk's)
struct QuiltScaleChunk
{
    uint32_t oc0, oc1, s0, s1;
    AreaSpan sx[2];
    bool own[2];
};

// false: the chunk lies beyond the tile (chunks of equal width can cover the tile with fewer chunks than were launched): the whole
// workgroup leaves
__device__ __forceinline__ bool quilt_scale_chunk(const QuiltScaleArgs &q, QuiltScaleChunk &c)
{
    const uint32_t W = q.src.W, tw = q.tile_w, t = threadIdx.x;
    c.oc0 = blockIdx.x * q.cols_per_wg, c.oc1 = min(c.oc0 + q.cols_per_wg, tw);
    if(c.oc0 >= tw)
        return false;
    c.s0 = area_span(W, tw, c.oc0).first & ~3u, c.s1 = area_span(W, tw, c.oc1 - 1u).last + 1u;
#pragma unroll
    for(int k = 0; k < 2; k++)
    {
        const uint32_t ox = c.oc0 + t + uint32_t(k) * QUILT_SCALE_THREADS;
        c.own[k] = ox < c.oc1;
        c.sx[k] = area_span(W, tw, c.own[k] ? ox : c.oc0);
    }
    return true;
}

// Output row oy of the chunk: out[k] = the finished pixel (R | G << 8 | B << 16 | 255 << 24) of the thread's output column k, where own[k].
// Called by every thread of the workgroup (it holds barriers); col is the workgroup's 12 KiB of LDS, free again on return.
template <bool PLANAR>
__device__ __forceinline__ void quilt_scale_row(const QuiltScaleArgs &q, const uint8_t *view, uint32_t (*col)[QUILT_SCALE_PIECE], const QuiltScaleChunk &c,
                                                const uint32_t oy, uint32_t (&out)[2])
{
    const uint32_t W = q.src.W, H = q.src.H, tw = q.tile_w, th = q.tile_h;
    const uint32_t t = threadIdx.x;
    const uint32_t s0 = c.s0, s1 = c.s1;
    const uint64_t area = (uint64_t)W * H;
    const AreaSpan sy = area_span(H, th, oy); // wave-uniform
    uint64_t acc[2][3] = {};
    for(uint32_t p0 = s0; p0 < s1; p0 += QUILT_SCALE_PIECE)
    {
        const uint32_t x = p0 + t * 4u;
        uint32_t v[3][4] = {};
        if(x < s1) // ⇒ x < W
            for(uint32_t y = sy.first; y <= sy.last; y++)
            {
                const uint32_t wy = area_weight(sy, th, y);
                if constexpr(PLANAR)
                {
                    uint32_t p[3];
#pragma unroll
                    for(int ch = 0; ch < 3; ch++) // x is a multiple of 4 below W: the dword lies inside the row's pitch
                        p[ch] = *reinterpret_cast<const uint32_t *>(view + ((size_t)ch * H + y) * q.src.pitch + x);
#pragma unroll
                    for(int ch = 0; ch < 3; ch++)
#pragma unroll
                        for(int k = 0; k < 4; k++)
                            v[ch][k] += wy * ((p[ch] >> (8 * k)) & 0xffu);
                }
                else
                {
                    const uint32_t *src = reinterpret_cast<const uint32_t *>(view) + (size_t)y * W + x;
                    uint32_t px[4];
                    if(x + 3u < W)
                    {
                        const quilt_u32x4 p = reinterpret_cast<const quilt_px4 *>(src)->v;
                        px[0] = p.x, px[1] = p.y, px[2] = p.z, px[3] = p.w;
                    }
                    else
#pragma unroll
                        for(int k = 0; k < 4; k++)
                            px[k] = x + k < W ? src[k] : 0u;
#pragma unroll
                    for(int ch = 0; ch < 3; ch++)
#pragma unroll
                        for(int k = 0; k < 4; k++)
                            v[ch][k] += wy * ((px[k] >> (8 * ch)) & 0xffu);
                }
            }
#pragma unroll
        for(int ch = 0; ch < 3; ch++)
            *reinterpret_cast<quilt_u32x4 *>(&col[ch][t * 4u]) = quilt_u32x4{v[ch][0], v[ch][1], v[ch][2], v[ch][3]};
        __syncthreads();
#pragma unroll
        for(int k = 0; k < 2; k++)
            if(c.own[k])
            {
                const uint32_t lo = max(c.sx[k].first, p0), hi = min(c.sx[k].last, p0 + uint32_t(QUILT_SCALE_PIECE - 1));
                for(uint32_t s = lo; s <= hi; s++)
                {
                    const uint32_t w = area_weight(c.sx[k], tw, s);
#pragma unroll
                    for(int ch = 0; ch < 3; ch++)
                        acc[k][ch] += (uint64_t)w * col[ch][s - p0];
                }
            }
        __syncthreads(); // the next piece / row overwrites col
    }
#pragma unroll
    for(int k = 0; k < 2; k++)
    {
        out[k] = 0xff000000u;
        if(c.own[k])
#pragma unroll
            for(int ch = 0; ch < 3; ch++)
            {
                const uint64_t n = acc[k][ch] + area / 2u;
                uint32_t r = (uint32_t)((float)n * q.rcp_area);
                if((uint64_t)r * area > n)
                    r--;
                else if((uint64_t)(r + 1u) * area <= n)
                    r++;
                out[k] |= r << (8 * ch);
            }
    }
}

template <bool PLANAR>
__global__ void __launch_bounds__(QUILT_SCALE_THREADS) quilt_scale(const QuiltScaleArgs q)
{
    __shared__ __attribute__((aligned(16))) uint32_t col[3][QUILT_SCALE_PIECE];
    const uint32_t tw = q.tile_w, th = q.tile_h;
    const uint32_t t = threadIdx.x;
    const int i = blockIdx.z;
    const int tile = q.first + i, trow = tile / q.tiles_x - q.first / q.tiles_x, tcol = tile % q.tiles_x;
    const uint8_t *view = q.src.base + (size_t)(q.v0 + i) * q.src.view_stride;
    QuiltScaleChunk c;
    if(!quilt_scale_chunk(q, c))
        return;
    const uint32_t oy0 = blockIdx.y * q.rows_per_wg, oy1 = min(oy0 + q.rows_per_wg, th);
    uint32_t *qrow0 = q.quilt + ((size_t)trow * th) * ((size_t)q.tiles_x * tw) + (size_t)tcol * tw;

    for(uint32_t oy = oy0; oy < oy1; oy++)
    {
        uint32_t out[2];
        quilt_scale_row<PLANAR>(q, view, col, c, oy, out);
#pragma unroll
        for(int k = 0; k < 2; k++)
            if(c.own[k])
                qrow0[(size_t)oy * ((size_t)q.tiles_x * tw) + c.oc0 + t + uint32_t(k) * QUILT_SCALE_THREADS] = out[k];
    }
}

// The decomposition of a launch for n tiles, shared by quilt_scale and quilt_yuv_scale (quilt_yuv.hpp): fills in q's cols_per_wg,
// rows_per_wg and rcp_area and returns the grid.  even_cols (tile_w even): chunks of an even number of columns
inline dim3 quilt_scale_plan(QuiltScaleArgs &q, const int n, const bool even_cols)
{
    // the most output columns whose source columns fit one piece: m columns overlap at most m·W / tile_w + 2 source columns, and the
    // chunk starts up to 3 columns before its first one; then as many chunks as that takes, of equal width.  A ratio so high that no
    // column (even_cols: no two) fits takes chunks of one (two) and several pieces
    const uint64_t fit = (uint64_t)(QUILT_SCALE_PIECE - 5) * q.tile_w / q.src.W;
    uint32_t most = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(fit, 1), QUILT_SCALE_COLS);
    if(even_cols)
        most = std::max(most & ~1u, 2u);
    const uint32_t chunks = (q.tile_w + most - 1) / most;
    q.cols_per_wg = (q.tile_w + chunks - 1) / chunks;
    if(even_cols)
        q.cols_per_wg = (q.cols_per_wg + 1u) & ~1u; // ≤ most, which is even
    q.rows_per_wg = QUILT_SCALE_ROWS;
    q.rcp_area = 1.0f / (float)((uint64_t)q.src.W * q.src.H);
    return dim3(chunks, (q.tile_h + q.rows_per_wg - 1) / q.rows_per_wg, n);
}

// Enqueues ONE quilt_scale launch for n tiles.  The caller has checked 1 ≤ tile_w ≤ W ≤ LFI_AREA_SPAN_MAX, likewise in y, and n ≥ 1.
inline hipError_t launch_quilt_scale(hipStream_t stream, const bool planar, QuiltScaleArgs q, const int n)
{
    const dim3 grid = quilt_scale_plan(q, n, false), block(QUILT_SCALE_THREADS);
    if(planar)
        hipLaunchKernelGGL(quilt_scale<true>, grid, block, 0, stream, q);
    else
        hipLaunchKernelGGL(quilt_scale<false>, grid, block, 0, stream, q);
    return hipGetLastError();
}

} // namespace lfi
