// native_filter.hpp — the FILTERED native image of lfi_download_native: what LFI_LENT_BGR, LFI_LENT_BILINEAR and LFI_LENT_BLEND ask for
// (include/lfi.h).  native_image.hpp's native_interlace stays the kernel of a call with none of the three.
//
// Definition, all in unsigned integers: for output pixel (x, y) and colour channel c, s = c (LFI_LENT_BGR: 2 − c),
// phase = phase0 + (3·x + s)·x_step + y·y_step (mod 2³²), k = __umulhi(phase, n), f = (phase·n) >> 24 (the top eight bits of the fraction).
//   LFI_LENT_BLEND     f ≥ 128: ka = k, kb = min(k + 1, n − 1), wb = f − 128; else ka = max(k, 1) − 1, kb = k, wb = f + 128 — the ends clamp;
//                      out = ((256 − wb)·S_ka + wb·S_kb + 128) >> 8.  Without it out = S_k.  LFI_LENT_INVERT maps every index q to n − 1 − q.
//   LFI_LENT_BILINEAR  S_v = ((256 − fy)·h_0 + fy·h_1 + 2¹⁵) >> 16, h_j = (256 − fx)·T_v[y_j][x0][c] + fx·T_v[y_j][x1][c], the taps and weights of
//                      ../native_taps.h along each axis.  Without it S_v = T_v[sy][sx][c], native_image.hpp's nearest pixel.
//   Bounds: h_j ≤ 256·255, the sum before the shift ≤ 2²⁴ − 2¹⁶ + 2¹⁵, the blend's ≤ 256·255 + 128: all below 2²⁴.
//
//   native_filter<PLANAR, BILINEAR, BLEND>  native_interlace's ownership: one workgroup (four waves) per (output row, 256 output columns), a
//     lane owns ONE output pixel and stores ONE dword, neighbouring lanes neighbouring dwords.  The row's taps (y0, y1, fy), their two
//     offsets inside a plane and y·y_step are wave-uniform; x0, x1 and fx are computed once per lane (three u32 divisions) for all three
//     channels and both views.  Per channel the lane loads one byte per (view, row, tap): 1, 2, 4 or 8 of them — byte c of the RGBA pixel,
//     or plane c of a planar view at the row pitch.  When the tile is smaller than the output neighbouring lanes read the same taps and
//     the cache serves them, so nothing is staged: no LDS, no atomics, no byte stores.  BGR is a wave-uniform argument.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../native_taps.h"
#include "native_image.hpp"

namespace lfi {

struct NativeFilterArgs
{
    NativeArgs n;
    uint32_t bgr; // 0 / 1: the panel's subpixels run B, G, R
};

template <bool PLANAR, bool BILINEAR, bool BLEND>
__global__ void __launch_bounds__(NATIVE_THREADS) native_filter(const NativeFilterArgs f)
{
    const NativeArgs &a = f.n;
    const uint32_t x = blockIdx.x * NATIVE_THREADS + threadIdx.x, y = blockIdx.y; // y < out_h: the grid has out_h rows
    if(x >= a.out_w)
        return;
    constexpr uint32_t PX = PLANAR ? 1u : 4u;                                     // bytes from pixel to pixel of a row
    const size_t row_bytes = PLANAR ? (size_t)a.src.pitch : (size_t)a.src.W * 4u;
    const size_t channel = PLANAR ? (size_t)a.src.H * a.src.pitch : 1u;           // bytes from channel to channel
    const uint32_t row_phase = a.phase0 + y * a.y_step;                           // wave-uniform
    // the taps: rows wave-uniform, columns per lane; nearest sampling is one tap of full weight
    uint32_t fx = 0, fy = 0, o0, o1;
    size_t r0, r1;
    if(BILINEAR)
    {
        const NativeTaps ty = native_taps(y, a.src.H, a.out_h), tx = native_taps(x, a.src.W, a.out_w);
        r0 = ty.p0 * row_bytes, r1 = ty.p1 * row_bytes, fy = ty.f;
        o0 = tx.p0 * PX, o1 = tx.p1 * PX, fx = tx.f;
    }
    else
    {
        r0 = r1 = native_nearest(y, a.src.H, a.out_h) * row_bytes;
        o0 = o1 = native_nearest(x, a.src.W, a.out_w) * PX;
    }
    // S_q(c): the tile sample of selected index q
    const auto sample = [&](uint32_t q, const uint32_t c) -> uint32_t {
        if(a.invert)
            q = a.n - 1u - q;
        const uint8_t *p = a.src.base + (size_t)q * a.src.view_stride + c * channel;
        if(!BILINEAR)
            return p[r0 + o0];
        const uint32_t h0 = (256u - fx) * p[r0 + o0] + fx * p[r0 + o1], h1 = (256u - fx) * p[r1 + o0] + fx * p[r1 + o1];
        return ((256u - fy) * h0 + fy * h1 + 32768u) >> 16;
    };
    uint32_t px = 0xff000000u;
#pragma unroll
    for(uint32_t c = 0; c < 3; c++)
    {
        const uint32_t s = f.bgr ? 2u - c : c;
        const uint32_t phase = row_phase + (3u * x + s) * a.x_step;
        const uint32_t k = __umulhi(phase, a.n); // < n
        uint32_t v;
        if(BLEND)
        {
            const uint32_t frac = (phase * a.n) >> 24, upper = frac >= 128u;
            const uint32_t ka = upper ? k : (k ? k - 1u : 0u), kb = upper ? (k + 1u < a.n ? k + 1u : a.n - 1u) : k;
            const uint32_t wb = upper ? frac - 128u : frac + 128u;
            v = ((256u - wb) * sample(ka, c) + wb * sample(kb, c) + 128u) >> 8;
        }
        else
            v = sample(k, c);
        px |= v << (8u * c);
    }
    a.out[(size_t)y * a.out_w + x] = px;
}

// Enqueues the ONE native_filter launch.  The caller has checked 1 ≤ out_w, out_h, W, H ≤ NATIVE_MAX and n ≥ 1.
inline hipError_t launch_native_filter(hipStream_t stream, const bool planar, const bool bilinear, const bool blend, const NativeFilterArgs &f)
{
    const dim3 grid((f.n.out_w + NATIVE_THREADS - 1) / NATIVE_THREADS, f.n.out_h), block(NATIVE_THREADS);
    void (*const kernels[8])(NativeFilterArgs) = {
        native_filter<false, false, false>, native_filter<false, false, true>, native_filter<false, true, false>, native_filter<false, true, true>,
        native_filter<true, false, false>,  native_filter<true, false, true>,  native_filter<true, true, false>,  native_filter<true, true, true>,
    };
    hipLaunchKernelGGL(kernels[(planar ? 4 : 0) | (bilinear ? 2 : 0) | (blend ? 1 : 0)], grid, block, 0, stream, f);
    return hipGetLastError();
}

} // namespace lfi
