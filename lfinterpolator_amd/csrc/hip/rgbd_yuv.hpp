// rgbd_yuv.hpp — RGB-D video frames (lfi_download_rgbd_yuv): a view and a focus map side by side in one 8-bit YUV 4:2:0 frame, made on the
// device without the grey image of the map.
//
// Definition (include/lfi.h): frame k of the call is what lfi_download_quilt_yuv's definition makes of the 2 × 1 quilt {V, D}: V = view
// v0 + k, D = the RGBA image (d, d, d, 255) of d = M or 255 − M, M the R byte plane of the chosen map.  tile_w and tile_h are EVEN, so the
// frame is 2·tile_w × tile_h, no 2 × 2 block straddles the halves, and quilt_yuv.hpp's kernel body applies to the left half as it stands.
//
// What D's greyness makes of the right half (YUV_COEFFS, yuv420.hpp):
//   - the area filter treats the channels alike, so the resized D is grey: s = the rounded area mean of d, one quotient per pixel;
//   - Y = y_off + ((yR·s + yG·s + yB·s + 2¹⁵) >> 16) = y_off + ((S·s + 2¹⁵) >> 16) with S = yR + yG + yB = 56284 (limited) or 65536 (full:
//     Y = s) — one multiply, exact by distributivity in integers;
//   - the chroma coefficients of a row sum to 0, so uR·4s' + uG·4s' + uB·4s' vanishes for any block sums and every chroma sample is
//     (2²⁵ + 2¹⁷) >> 18 = 128: a constant, no arithmetic.
//
//   rgbd_yuv_scale<PLANAR, FORMAT>  ONE launch for the 2n halves of n frames: blockIdx.z = 2k + half, quilt_scale_plan's decomposition with
//     even chunk widths (quilt_scaled.hpp), one workgroup per (half, band of 4 output rows, chunk of ≤ 512 output columns).
//     half 0  quilt_yuv_tile (quilt_yuv.hpp), the body of quilt_yuv_scale: view v0 + k into tile (0, 0) of frame k.
//     half 1  the one-channel row, rgbd_depth_row: lanes load the map's dwords as quilt_scale_row<false> loads an RGBA view's, keep the
//       R byte (XOR 255 where the call inverts: 255 − M, before any sum), and hold FOUR vertical sums instead of twelve; one LDS column
//       array of 4 KiB instead of three (the first of the workgroup's 12 KiB); one u64 horizontal sum and one corrected quotient per output
//       column.  After an odd row a lane holds its column's two values of the row pair: one multiply each gives the two Y, ONE DPP pair
//       exchange (quilt_yuv_pair) hands them to the neighbour, and the even lane stores the two 2-byte Y pieces and the constant chroma,
//       one byte 128 in each of the Cb and Cr rows (I420) or the two bytes 0x8080 (NV12).
//   The branch on `half` is uniform per workgroup (blockIdx.z); each half holds its own barriers.
//
// Where the bytes go: quilt_yuv.hpp's header, with QW = 2·tile_w, QH = tile_h and the frame's base = s.base + k·frame_stride.  The depth
// half's frame column fx = tile_w + oc0 + t (+ 256) is even on even lanes because tile_w, oc0 and t are, so the same alignment argument
// holds: 2-byte stores at even offsets of even bases and pitches (in-place surfaces: multiples of 16 throughout, frame_stride included;
// staged frames: yuv_geometry's, dev_frame_bytes a multiple of 8), every block written by exactly one lane, no read of dst, no atomics,
// nothing outside the planes' own bytes.
// What is read: rows [0, H) and columns [0, W) of the map plane of frame k — map.base + k·map.view_stride, W·H dwords; the 16-byte load is
// taken only where x + 3 < W, as in quilt_scale_row.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "quilt_yuv.hpp"

namespace lfi {

struct RgbdYuvArgs
{
    QuiltScaleArgs q; // src: the views, frame k is made of view v0 + k; quilt and first unused, tiles_x = 2 is not read
    ViewsSrc map;     // RGBA map planes of the views' size (pitch 0), frame k reads base + k·view_stride: 0 = one map for every frame
    YuvSurfaces s;    // the n frames of 2·tile_w × tile_h, written
    YuvCoeffs k;
    uint32_t flip;    // 255: d = 255 − M (= M ^ 255 on a byte); 0: d = M
};

// Output row oy of the depth half's chunk: out[k] = s, the rounded area mean of d over the thread's output column k, where own[k].  Called
// by every thread of the workgroup (it holds barriers); col is 4 KiB of LDS, free again on return.  quilt_scale_row<false> for one channel.
__device__ __forceinline__ void rgbd_depth_row(const QuiltScaleArgs &q, const uint8_t *map, const uint32_t flip, uint32_t *col, const QuiltScaleChunk &c,
                                               const uint32_t oy, uint32_t (&out)[2])
{
    const uint32_t W = q.src.W, H = q.src.H, tw = q.tile_w, th = q.tile_h;
    const uint32_t t = threadIdx.x;
    const uint32_t s0 = c.s0, s1 = c.s1;
    const uint64_t area = (uint64_t)W * H;
    const AreaSpan sy = area_span(H, th, oy); // wave-uniform
    uint64_t acc[2] = {};
    for(uint32_t p0 = s0; p0 < s1; p0 += QUILT_SCALE_PIECE)
    {
        const uint32_t x = p0 + t * 4u;
        uint32_t v[4] = {};
        if(x < s1) // ⇒ x < W
            for(uint32_t y = sy.first; y <= sy.last; y++)
            {
                const uint32_t wy = area_weight(sy, th, y);
                const uint32_t *src = reinterpret_cast<const uint32_t *>(map) + (size_t)y * W + x;
                uint32_t px[4];
                if(x + 3u < W)
                {
                    const quilt_u32x4 p = reinterpret_cast<const quilt_px4 *>(src)->v;
                    px[0] = p.x, px[1] = p.y, px[2] = p.z, px[3] = p.w;
                }
                else
#pragma unroll
                    for(int k = 0; k < 4; k++)
                        px[k] = x + k < W ? src[k] : 0u; // a column past W enters no output column's span: its sum is never read
#pragma unroll
                for(int k = 0; k < 4; k++)
                    v[k] += wy * ((px[k] & 0xffu) ^ flip);
            }
        *reinterpret_cast<quilt_u32x4 *>(&col[t * 4u]) = quilt_u32x4{v[0], v[1], v[2], v[3]};
        __syncthreads();
#pragma unroll
        for(int k = 0; k < 2; k++)
            if(c.own[k])
            {
                const uint32_t lo = max(c.sx[k].first, p0), hi = min(c.sx[k].last, p0 + uint32_t(QUILT_SCALE_PIECE - 1));
                for(uint32_t s = lo; s <= hi; s++)
                    acc[k] += (uint64_t)area_weight(c.sx[k], tw, s) * col[s - p0];
            }
        __syncthreads(); // the next piece / row overwrites col
    }
#pragma unroll
    for(int k = 0; k < 2; k++)
    {
        out[k] = 0u;
        if(c.own[k])
        {
            const uint64_t n = acc[k] + area / 2u;
            uint32_t r = (uint32_t)((float)n * q.rcp_area);
            if((uint64_t)r * area > n)
                r--;
            else if((uint64_t)(r + 1u) * area <= n)
                r++;
            out[k] = r;
        }
    }
}

// The depth half of one frame: the map plane resized to tile (0, 1) of the frame s, luma by one multiply, chroma constant
template <int FORMAT>
__device__ __forceinline__ void rgbd_depth_tile(const QuiltScaleArgs &q, const YuvSurfaces &s, const YuvCoeffs &kc, const uint8_t *map, const uint32_t flip,
                                                uint32_t *col)
{
    const uint32_t tw = q.tile_w, th = q.tile_h;
    const uint32_t t = threadIdx.x;
    QuiltScaleChunk c;
    if(!quilt_scale_chunk(q, c))
        return;
    const uint32_t oy0 = blockIdx.y * q.rows_per_wg, oy1 = min(oy0 + q.rows_per_wg, th); // both even
    const uint32_t fx0 = tw + c.oc0 + t;                                                  // the frame column of the thread's first column
    const bool stores = !(t & 1u);
    const uint32_t S = (uint32_t)(kc.y[0] + kc.y[1] + kc.y[2]); // 56284 or 65536

    uint32_t upper[2] = {};
    for(uint32_t oy = oy0; oy < oy1; oy++)
    {
        uint32_t out[2];
        rgbd_depth_row(q, map, flip, col, c, oy, out);
        if(!(oy & 1u))
        {
            upper[0] = out[0], upper[1] = out[1];
            continue;
        }
        const uint32_t fy = oy - 1u; // even; fy + 1 < tile_h
#pragma unroll
        for(int k = 0; k < 2; k++)
        {
            // the column's two Y values, rows fy | fy + 1 << 16; every lane takes part in the exchange
            const uint32_t y = (kc.y_off + ((S * upper[k] + 0x8000u) >> 16)) | ((kc.y_off + ((S * out[k] + 0x8000u) >> 16)) << 16);
            const uint32_t y_n = quilt_yuv_pair(y);
            if(stores && c.own[k])
            {
                const uint32_t fx = fx0 + uint32_t(k) * QUILT_SCALE_THREADS; // even
                uint8_t *y_row = s.base + (size_t)fy * s.y_pitch + fx;
                *reinterpret_cast<uint16_t *>(y_row) = (uint16_t)((y & 0xffu) | ((y_n & 0xffu) << 8));
                *reinterpret_cast<uint16_t *>(y_row + s.y_pitch) = (uint16_t)(((y >> 16) & 0xffu) | ((y_n >> 16) << 8));
                const size_t c_row = (size_t)(fy >> 1) * s.c_pitch;
                if constexpr(FORMAT == YUVS_NV12)
                    *reinterpret_cast<uint16_t *>(s.base + s.c_offset + c_row + fx) = (uint16_t)0x8080u;
                else
                {
                    s.base[s.c_offset + c_row + (fx >> 1)] = (uint8_t)128u;
                    s.base[s.cr_offset + c_row + (fx >> 1)] = (uint8_t)128u;
                }
            }
        }
    }
}

template <bool PLANAR, int FORMAT>
__global__ void __launch_bounds__(QUILT_SCALE_THREADS) rgbd_yuv_scale(const RgbdYuvArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t col[3][QUILT_SCALE_PIECE];
    const uint32_t k = blockIdx.z >> 1;
    YuvSurfaces s = a.s;
    s.base += (size_t)k * s.frame_stride;
    if(!(blockIdx.z & 1u))
        quilt_yuv_tile<PLANAR, FORMAT>(a.q, s, a.k, (int)k, 0, 1, col); // view v0 + k as tile 0 of a frame one tile wide: at the frame's origin
    else
        rgbd_depth_tile<FORMAT>(a.q, s, a.k, a.map.base + (size_t)k * a.map.view_stride, a.flip, col[0]);
}

// Enqueues the ONE rgbd_yuv_scale launch for n frames.  The caller has checked what launch_quilt_yuv_scale's caller checks for n tiles of
// views [v0, v0 + n), that a.map's planes are of the views' size and n of them exist where view_stride != 0, and that a.s describes n
// frames of 2·tile_w × tile_h the device may write, aligned as the header says.
inline hipError_t launch_rgbd_yuv_scale(hipStream_t stream, const bool planar, const int format, RgbdYuvArgs a, const int n)
{
    const dim3 grid = quilt_scale_plan(a.q, 2 * n, true), block(QUILT_SCALE_THREADS);
    if(planar)
    {
        if(format == YUVS_NV12)
            hipLaunchKernelGGL((rgbd_yuv_scale<true, YUVS_NV12>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((rgbd_yuv_scale<true, YUVS_I420>), grid, block, 0, stream, a);
    }
    else
    {
        if(format == YUVS_NV12)
            hipLaunchKernelGGL((rgbd_yuv_scale<false, YUVS_NV12>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((rgbd_yuv_scale<false, YUVS_I420>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

} // namespace lfi
