// native_image.hpp — the native image of a lenticular display (lfi_download_native): every subpixel of a display-sized picture takes its
// value from the one view that its phase under the slanted lens sheet selects.  A pure gather, defined in unsigned integers.
//
// Definition (include/lfi.h): for output pixel (x, y) and colour channel c,  phase = phase0 + (3·x + c)·x_step + y·y_step (mod 2³²),
// k = (u64(phase)·n) >> 32 (LFI_LENT_INVERT: n − 1 − k), and out[y][x][c] = T_{v0+k}[sy][sx][c] with (sx, sy) the tile pixel under the output
// pixel's centre; alpha is 255.  T_v is view v itself (read in place, either layout) or its scaled tile out of the device-resident quilt
// that launch_quilt_scale wrote as RGBA planes [view][tile_h][tile_w] (a quilt one tile wide).
//
//   native_interlace<PLANAR>  one workgroup (four waves) per (output row, 256 output columns); a lane owns ONE output pixel: it computes
//     the three phases, picks the three views, loads one byte from each (RGBA planes: byte c of the pixel; PLANAR: plane c at the row
//     pitch — no RGBA copy of planar views) and stores the assembled dword: neighbouring lanes, neighbouring dwords of one row.  A wave
//     stays in one output row, so sy, the row's offset inside a plane and y·y_step are wave-uniform (scalar registers); per lane remain
//     sx (two u32 divisions, see below), three multiplies for the views and three 64-bit address additions.  The loads are a gather by
//     nature — neighbouring subpixels read (almost) the same (sy, sx) of DIFFERENT views — and each source byte is used about once, so
//     nothing is staged in LDS: a wave's loads fall into one short segment of one row per view, and neighbouring waves and rows find
//     the rest of those cache lines in L2.  No LDS, no atomics, no byte stores.
//   sx in 32 bits: (2·x + 1)·tile_w reaches 2³³, so with q, r = quotient and remainder of x·tile_w by out_w (x·tile_w < 65535²),
//     sx = ((2·x + 1)·tile_w) / (2·out_w) = q + (2·r + tile_w) / (2·out_w), and 2·r + tile_w < 3·65535.  sy likewise, once per workgroup.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "views_src.hpp"

namespace lfi {

constexpr int NATIVE_THREADS = 256;
constexpr uint32_t NATIVE_MAX = 65535u; // the largest output / tile size along an axis: what keeps native_nearest in 32 bits

struct NativeArgs
{
    ViewsSrc src;  // the T_v, view 0 = the first view interlaced: the views in place, or their scaled tiles as a quilt one tile wide
    uint32_t *out; // the native image, out_h × out_w dwords
    uint32_t out_w, out_h;
    uint32_t x_step, y_step, phase0, n;
    uint32_t invert; // 0 / 1
};

// ((2·o + 1)·src) / (2·dst) for o < dst ≤ 65535, src ≤ 65535: the source pixel under the centre of output pixel o, below src
__host__ __device__ inline uint32_t native_nearest(const uint32_t o, const uint32_t src, const uint32_t dst)
{
    const uint32_t num = o * src, q = num / dst, r = num - q * dst;
    return q + (2u * r + src) / (2u * dst);
}

template <bool PLANAR>
__global__ void __launch_bounds__(NATIVE_THREADS) native_interlace(const NativeArgs a)
{
    const uint32_t x = blockIdx.x * NATIVE_THREADS + threadIdx.x, y = blockIdx.y; // y < out_h: the grid has out_h rows
    if(x >= a.out_w)
        return;
    const uint32_t sy = native_nearest(y, a.src.H, a.out_h);  // wave-uniform
    const uint32_t row_phase = a.phase0 + y * a.y_step;        // wave-uniform
    const uint32_t sx = native_nearest(x, a.src.W, a.out_w);
    // byte (sy, sx, channel 0) inside a view
    const size_t at = PLANAR ? (size_t)sy * a.src.pitch + sx : ((size_t)sy * a.src.W + sx) * 4u;
    const size_t channel = PLANAR ? (size_t)a.src.H * a.src.pitch : 1u; // bytes from channel to channel
    uint32_t px = 0xff000000u;
#pragma unroll
    for(uint32_t c = 0; c < 3; c++)
    {
        const uint32_t phase = row_phase + (3u * x + c) * a.x_step;
        uint32_t k = __umulhi(phase, a.n); // < n
        if(a.invert)
            k = a.n - 1u - k;
        px |= (uint32_t)a.src.base[(size_t)k * a.src.view_stride + at + c * channel] << (8u * c);
    }
    a.out[(size_t)y * a.out_w + x] = px;
}

// Enqueues the ONE native_interlace launch.  The caller has checked 1 ≤ out_w, out_h, W, H ≤ NATIVE_MAX and n ≥ 1.
inline hipError_t launch_native_interlace(hipStream_t stream, const bool planar, const NativeArgs &a)
{
    const dim3 grid((a.out_w + NATIVE_THREADS - 1) / NATIVE_THREADS, a.out_h), block(NATIVE_THREADS);
    if(planar)
        hipLaunchKernelGGL(native_interlace<true>, grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL(native_interlace<false>, grid, block, 0, stream, a);
    return hipGetLastError();
}

} // namespace lfi
