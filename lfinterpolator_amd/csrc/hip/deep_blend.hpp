// deep_blend.hpp — deep views (LFI_FLAG_DEEP_VIEWS, include/lfi.h): a fixed-focus render that keeps TEN bits per channel straight from the
// accumulator, beside the 8-bit views, from ONE gather and ONE accumulation per pixel and view.
//
// A view is a weighted mean of 64–225 input bytes accumulated in fp32; the 8-bit kernels cut that mean to a byte (blend_p3: floor of the
// fp16-rounded sum; the STD kernels: RN-even of the fp32 chain).  This kernel writes the byte planes exactly as those kernels define them
// AND, per (view, channel), a plane of little-endian u16 with the 10-bit code in bits 9..0 (upper six bits 0):
//      STD     s = the reference's ordered fmaf chain (src/kernels.cu:292-299), D10 = min(1023, rn_even(4·s)) — 4·s is exact in fp32
//      TEN_WM  s = the fp32-accumulated matrix-core sum,                          D10 = min(1023, floor(4·fp16_RN(s)))
// For TEN_WM D10 >> 2 IS the byte floor(min(fp16_RN(s), 255)) of blend_p3, so the byte plane is written from the code.
//
// The skeleton — the tile, the LDS image, the fetch by LDS-DMA, the unit walk, the two accumulate loops and the byte-plane store — is
// blend_tile16.hpp's, shared with blend_inframe.  This file adds the deep planes: a lane that ends with 8 consecutive pixels of a view and
// channel stores ONE 16-byte piece into the deep plane beside its 8-byte piece of the byte plane (16 lanes: 256 B of a deep-plane row).  The
// kernel writes 3× the bytes of blend_p3 per pixel and is paced by its stores.
#pragma once

#include "blend_tile16.hpp"

namespace lfi {

// deep planes: plane (view, channel) at ((view·3 + channel)·out_rows)·deep_pitch, pixel x of row y at y·deep_pitch + 2x; view = the
// ABSOLUTE view index.  deep_pitch = 2·W rounded up to 128: a multiple of 16 ≥ 2·round8(W), so a lane's 16-byte piece at 2·(x0 + 8n)
// lies inside its row wherever it starts inside it.
template <bool STD>
__global__ void __launch_bounds__(256, 2) deep_blend(const KernelArgs a, uint8_t *__restrict__ deep, const int deep_pitch, const int tiles_x, const int n_tiles,
                                                     const int view_passes, const int nch)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[T16_BUFS * P3_BUF_B + LFI_MAX_IMAGES * 8];

    const T16Lane L = t16_lane(lds);
    int2 *off_table = reinterpret_cast<int2 *>(lds + T16_BUFS * P3_BUF_B);
    t16_fill_offsets<false>(a, off_table, nullptr);
    if(int(blockIdx.x) >= n_tiles)
        return;

    f32x4 acc[8][3]; // [block = pixel 8n + blk][channel]: views 4kg + i of this wave's 16

    // quantise both ways, pack eight pixels per (view, channel), store
    auto epilogue = [&](const int t, const int vw, const int nvalid) {
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int x = tx * P3_TPX + 8 * L.n; // this lane's first pixel
        const bool x16 = 2 * x < deep_pitch; // the pitch ≥ twice the next multiple of 8 pixels: whole pieces stay inside the row
#pragma unroll
        for(int i = 0; i < 4; i++)
        {
            if(4 * L.kg + i >= nvalid)
                continue;
            const size_t plane0 = (size_t)(vw + 4 * L.kg + i) * 3;
#pragma unroll
            for(int ch = 0; ch < 3; ch++)
            {
                __builtin_amdgcn_sched_barrier(0); // one (view, channel) at a time
                uint32_t code[8], byte[8];
#pragma unroll
                for(int p = 0; p < 4; p++)
                {
                    if constexpr(STD)
                    {
#pragma unroll
                        for(int e = 0; e < 2; e++)
                        {
                            const float s = acc[2 * p + e][ch][i];
                            code[2 * p + e] = uint32_t(min(1023, max(0, __float2int_rn(4.0f * s)))); // 4·s is exact
                            byte[2 * p + e] = quant_rn(s);
                        }
                    }
                    else
                    {
                        // floor(4·S) = floor(acc·2^11) of the fp16-rounded sum
                        const float2_t r = t16_ten_round(float2_t{acc[2 * p][ch][i], acc[2 * p + 1][ch][i]});
#pragma unroll
                        for(int e = 0; e < 2; e++)
                        {
                            code[2 * p + e] = uint32_t(min(1023, int(r[e] * 2048.0f))); // sums are ≥ 0 (weights in [0, 2)): the cast is the floor
                            byte[2 * p + e] = code[2 * p + e] >> 2;
                        }
                    }
                }
                const size_t row = (plane0 + ch) * (size_t)a.out_rows + ty;
                t16_store_bytes(a, row, x, byte);
                if(x16)
                    *reinterpret_cast<u32x4 *>(deep + row * deep_pitch + 2 * x) =
                        u32x4{code[0] | (code[1] << 16), code[2] | (code[3] << 16), code[4] | (code[5] << 16), code[6] | (code[7] << 16)};
            }
        }
    };

    int buf = 0;
    auto fetch = [&](const int t, const int chunk, const int buf) { t16_fetch(a, L, off_table, tiles_x, a.out_y0, a.in_y0, a.in_rows, t, chunk, buf); };
    fetch(blockIdx.x, 0, 0);
    for(int t = blockIdx.x; t < n_tiles; t += gridDim.x)
        t16_tile(
            a, L, t, n_tiles, view_passes, nch, buf, fetch, [&] { t16_clear(acc); },
            [&](const int vw, const int chunk, const int buf) {
                if constexpr(STD)
                    t16_std_chunk<false>(a, L, lds + buf * P3_BUF_B, vw, chunk, acc, T16Unmasked{});
                else
                    t16_ten_chunk<false>(a, L, lds + buf * P3_BUF_B, vw, chunk, acc, T16Unmasked{});
            },
            [&](const int vw, const int nvalid) { epilogue(t, vw, nvalid); });
}

} // namespace lfi
