// blend_linear.hpp — linear-light blending (LFI_FLAG_LINEAR_LIGHT, include/lfi.h): a fixed-focus render that DECODES every input byte from its
// sRGB encoding to linear light before the weighted sum, and ENCODES the sum afterwards.
//
// For view v, channel c, pixel (x, y), images g ascending, px_g,c the byte of image g at pixel + focused_offsets[g] clamped to the frame (the
// samples of a flag-free fixed-focus render), D, T and E of ../linear_light.h:
//      s_c    = STD:    the ordered fp32 chain s ← fmaf(float(D[px_g,c]), w_g, s) — an fp16 times an fp16 is exact in fp32, so each link is one
//                       fp32 addition of an exact product
//               TEN_WM: the fp32-accumulated matrix-core sum of D[px_g,c] · w_g, the weights as given (a.w16, not the ×2^15 copy)
//      byte_c = E(s_c) = #{ b in 1 … 255 : T[b] ≤ s_c },   alpha 255
// E is the same under both methods; they differ only in how s is accumulated.
//
// The skeleton — the tile, the LDS image, the fetch by LDS-DMA (window 0, 0, H: no row window under the flag, flagged_refused), the unit walk,
// the ownership (a wave = 128 pixels × 16 views), the weight walk and the byte-plane store — is blend_tile16.hpp's, shared with deep_blend and
// blend_inframe.  What this file adds:
//   - the tables in LDS, filled once per workgroup before the offset-table barrier: the thresholds T[0 … 256] (fp32), the first-guess table G
//     of linear_light.h (one byte per sixteenth of [0, 256), built from T by each thread for 16 cells), and D — widened to fp32 for STD (it
//     saves the conversion), as fp16 bit patterns for TEN_WM;
//   - the decode, PER WAVE: every byte a lane takes out of the two dwords it read from a pixel buffer goes through D in LDS before it is an
//     operand — STD in place of the byte-to-float conversion, TEN_WM in place of the v_perm that makes fp16 subnormals (two 16-bit reads
//     packed into one operand dword).  The other way — decoding a whole unit once, cooperatively, into an fp16 operand buffer — needs
//     48 KB more LDS per buffer (or a channel at a time with two more barriers per unit) and was not built;
//   - TEN_WM: v_mfma_f32_16x16x32_f16 with A = the unscaled fp16 weights: the accumulator IS s;
//   - the epilogue E: linear_encode — one byte read of G, one read of T, one comparison.
#pragma once

#include "../linear_light.h"
#include "blend_tile16.hpp"

namespace lfi {

constexpr int LIN_THR_B = 260 * 4;                                  // T[0 … 256], padded to 16 bytes
constexpr int LIN_TABLES_B = LIN_THR_B + LINEAR_CELLS + 256 * 4; // T, G, D (fp32; TEN_WM uses the first half as fp16)

template <bool STD>
__global__ void __launch_bounds__(256, 2) blend_linear(const KernelArgs a, const int tiles_x, const int n_tiles, const int view_passes, const int nch)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[T16_BUFS * P3_BUF_B + LFI_MAX_IMAGES * 8 + LIN_TABLES_B];

    const T16Lane L = t16_lane(lds);
    const int H = a.height;
    int2 *off_table = reinterpret_cast<int2 *>(lds + T16_BUFS * P3_BUF_B);
    float *thr = reinterpret_cast<float *>(lds + T16_BUFS * P3_BUF_B + LFI_MAX_IMAGES * 8);
    uint8_t *guess = reinterpret_cast<uint8_t *>(thr) + LIN_THR_B;
    float *d32 = reinterpret_cast<float *>(guess + LINEAR_CELLS);
    uint16_t *d16 = reinterpret_cast<uint16_t *>(d32);

    // the tables: T and D by thread b, then (T complete) G by 16 cells per thread; t16_fill_offsets' barrier completes them all
    thr[threadIdx.x] = linear_threshold(threadIdx.x);
    if(threadIdx.x == 0)
        thr[256] = linear_threshold(256);
    if constexpr(STD)
        d32[threadIdx.x] = float(__builtin_bit_cast(_Float16, LINEAR_D16_BITS[threadIdx.x]));
    else
        d16[threadIdx.x] = LINEAR_D16_BITS[threadIdx.x];
    __syncthreads();
    for(int cell = threadIdx.x; cell < LINEAR_CELLS; cell += 256)
        guess[cell] = linear_guess(thr, cell);
    t16_fill_offsets<false>(a, off_table, nullptr);
    if(int(blockIdx.x) >= n_tiles)
        return;

    f32x4 acc[8][3]; // [block = pixel 8n + blk][channel]: views 4kg + i of this wave's 16

    // STD, one chunk of images from the buffer at pb into acc: t16_std_chunk with D[byte] (fp32 in LDS) in place of float(byte)
    auto std_chunk = [&](const uint8_t *pb, const int vw, const int chunk) {
        t16_weights(a, L, vw, chunk, [&](const int gl, const float (&wv)[4]) {
            const uint8_t *row = pb + p3_octet_off(gl >> 3) + 128 * (gl & 7) + 8 * L.n;
#pragma unroll
            for(int ch = 0; ch < 3; ch++)
            {
                __builtin_amdgcn_sched_barrier(0); // one channel's pixels at a time
                const u32x2 p = *reinterpret_cast<const u32x2 *>(row + ch * P3_CH_B);
#pragma unroll
                for(int b = 0; b < 8; b++)
                {
                    const float px = d32[((b < 4 ? p.x : p.y) >> (8 * (b & 3))) & 0xffu];
#pragma unroll
                    for(int i = 0; i < 4; i++)
                        acc[b][ch][i] = __builtin_fmaf(px, wv[i], acc[b][ch][i]);
                }
            }
        });
    };

    // TEN_WM, one chunk of images from the buffer at pb into acc: t16_ten_chunk's fragments with A = the unscaled weights and B = D[byte]
    // (fp16 in LDS).  Octets of a short chunk that were not fetched hold stale bytes: every byte decodes to a finite value, their weights are 0
    auto ten_chunk = [&](const uint8_t *pb, const int vw, const int chunk) {
        const int kc = min(P3_KC, a.k_pad - P3_KC * chunk);
        const int n_ks = kc > 32 ? 2 : 1; // wave-uniform: a chunk of ≤ 32 images has one k-step
#pragma unroll
        for(int ks = 0; ks < 2; ks++)
        {
            if(ks >= n_ks)
                break;
            // A fragment: lane l: view l & 15, images 32ks + 8kg + j of the chunk
            const int k = P3_KC * chunk + 32 * ks + 8 * L.kg;
            u32x4 w = {0u, 0u, 0u, 0u};
            if(k < a.k_pad) // rows are k_pad halves long (a multiple of 16): nothing is read across a row's end
                w = *reinterpret_cast<const u32x4 *>(a.w16 + (size_t)(vw + L.n) * a.k_pad + k);
            const half8 wk = __builtin_bit_cast(half8, w);
            const uint8_t *po = pb + p3_octet_off(4 * ks + L.kg) + 8 * L.n;
#pragma unroll
            for(int ch = 0; ch < 3; ch++)
            {
                __builtin_amdgcn_sched_barrier(0); // one group's reads at a time: the accumulators leave few registers to hoist into
                u32x2 d[8]; // the lane's eight pixels of images 8(4ks + kg) + j
#pragma unroll
                for(int j = 0; j < 8; j++)
                    d[j] = *reinterpret_cast<const u32x2 *>(po + ch * P3_CH_B + 128 * j);
#pragma unroll
                for(int b = 0; b < 8; b++)
                {
                    u32x4 bf;
#pragma unroll
                    for(int q = 0; q < 4; q++)
                    {
                        const uint32_t lo = b < 4 ? d[2 * q].x : d[2 * q].y, hi = b < 4 ? d[2 * q + 1].x : d[2 * q + 1].y;
                        // [15:0] = D[byte (b & 3) of image 2q], [31:16] = D[the same byte of image 2q + 1]
                        bf[q] = uint32_t(d16[(lo >> (8 * (b & 3))) & 0xffu]) | (uint32_t(d16[(hi >> (8 * (b & 3))) & 0xffu]) << 16);
                    }
                    acc[b][ch] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wk, __builtin_bit_cast(half8, bf), acc[b][ch], 0, 0, 0);
                }
            }
        }
    };

    // encode, pack eight pixels per (view, channel), store
    auto epilogue = [&](const int t, const int vw, const int nvalid) {
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int x = tx * P3_TPX + 8 * L.n; // this lane's first pixel
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
                uint32_t byte[8];
#pragma unroll
                for(int b = 0; b < 8; b++)
                    byte[b] = linear_encode(acc[b][ch][i], guess, thr);
                t16_store_bytes(a, (plane0 + ch) * (size_t)H + ty, x, byte);
            }
        }
    };

    int buf = 0;
    auto fetch = [&](const int t, const int chunk, const int buf) { t16_fetch(a, L, off_table, tiles_x, 0, 0, H, t, chunk, buf); };
    fetch(blockIdx.x, 0, 0);
    for(int t = blockIdx.x; t < n_tiles; t += gridDim.x)
        t16_tile(
            a, L, t, n_tiles, view_passes, nch, buf, fetch, [&] { t16_clear(acc); },
            [&](const int vw, const int chunk, const int buf) {
                if constexpr(STD)
                    std_chunk(lds + buf * P3_BUF_B, vw, chunk);
                else
                    ten_chunk(lds + buf * P3_BUF_B, vw, chunk);
            },
            [&](const int vw, const int nvalid) { epilogue(t, vw, nvalid); });
}

} // namespace lfi
