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
// A sibling of blend_p3 (blend_p3.hpp), whose tile, LDS image and operand maps it shares:
//   - the planar, alpha-free copy of the inputs comes in through LDS by LDS-DMA (global_load_lds_dwordx4: 16 bytes per lane, eight lanes
//     per image row of the 128-pixel tile), into the image of a blend_p3 buffer: [channel][octet of images][8 images × 128 B], octets
//     padded by p3_octet_off so that the four octets one ds_read_b64 instruction touches fall into different banks;
//   - persistent workgroups walk the tiles t, t + G, …; a unit is (tile, chunk of 64 images); two buffers: the next unit's fetch is
//     issued before the current unit is computed, ONE barrier per unit.  The wait in front of the barrier is s_waitcnt vmcnt(0) — no
//     hand-counted waits: the kernel writes 3× the bytes of blend_p3 per pixel and is paced by its stores, which the wait also drains;
//   - TEN_WM: a wave = 128 pixels × 16 views on v_mfma_f32_16x16x32_f16, A = weights × 2^15 (lane l: view l & 15, images 8(l >> 4) + j),
//     B = pixels as fp16 subnormals (one v_perm per image pair), D: lane (n, kg) ends with pixels 8n … 8n + 7 of views 4kg + i;
//   - STD: the same ownership (lane (n, kg): pixels 8n … 8n + 7 of views 4kg + i of its wave's 16) on the vector pipe: per image one
//     ds_read_b64 per channel (the four kg groups read the same address: a broadcast) and 96 IEEE fused multiply-adds (the compiler pairs them
//     as 48 v_pk_fma_f32: two fmas each, as blend_std_vfma's), images in ascending order — the chain's value itself, not the band method's decision;
//   - a lane that ends with 8 consecutive pixels of a view and channel stores ONE 8-byte piece into the byte plane and ONE 16-byte piece
//     into the deep plane: 16 lanes write 128 B of a byte-plane row and 256 B of a deep-plane row.
// One chunk of images (up to 64): every 64-view pass of a tile reads the same LDS-resident pixels (any number of views in one launch).
// Several chunks: the host launches once per 64 views.
#pragma once

#include "blend_p3.hpp"
#include "blend_std.hpp"

namespace lfi {

constexpr int DEEP_BUFS = 2;

// deep planes: plane (view, channel) at ((view·3 + channel)·out_rows)·deep_pitch, pixel x of row y at y·deep_pitch + 2x; view = the
// ABSOLUTE view index.  deep_pitch = 2·W rounded up to 128: a multiple of 16 ≥ 2·round8(W), so a lane's 16-byte piece at 2·(x0 + 8n)
// lies inside its row wherever it starts inside it.
template <bool STD>
__global__ void __launch_bounds__(256, 2) deep_blend(const KernelArgs a, uint8_t *__restrict__ deep, const int deep_pitch, const int tiles_x, const int n_tiles,
                                                     const int view_passes, const int nch)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[DEEP_BUFS * P3_BUF_B + LFI_MAX_IMAGES * 8];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lane & 15, kg = lane >> 4;
    const int H = a.height;
    const uint32_t lds_base = __builtin_amdgcn_readfirstlane(uint32_t(uintptr_t((lds_ptr_t)lds)));
    const size_t shift_stride = (size_t)a.in_rows * a.planar_pitch; // one byte plane of the planar inputs
    int2 *off_table = reinterpret_cast<int2 *>(lds + DEEP_BUFS * P3_BUF_B);
    for(int g = threadIdx.x; g < a.n_images; g += 256)
    {
        const lfi_int2 o = a.focused[g];
        off_table[g] = make_int2(o.x + a.planar_phase[g], o.y); // the image's phase inside the planar copy folded into its x offset
    }
    __syncthreads(); // the offset table is complete
    const int G = gridDim.x;
    if(int(blockIdx.x) >= n_tiles)
        return;

    // the fetch of unit (tile t, chunk): wave w moves octets w and w + 4 of every channel; lane l the 16 bytes at 16·(l & 7) of the
    // 128-byte run of image (l >> 3) of the octet.  Addressing is blend_p3's issue_piece: the run starts at pixel x0 + ox (+ the image's
    // phase), the copy's padding exceeds every offset (ensure_planar), rows are clamped in the full image.
    auto issue = [&](const int t, const int chunk, const int buf) {
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int y = a.out_y0 + ty, x0 = tx * P3_TPX;
        const int kc = min(P3_KC, a.k_pad - P3_KC * chunk);
        const uint32_t dst = lds_base + uint32_t(buf) * P3_BUF_B;
#pragma unroll
        for(int o2 = 0; o2 < 2; o2++)
        {
            const int octet = wave + 4 * o2;
            if(8 * octet >= kc)
                continue; // wave-uniform: the chunk is shorter (its length is a multiple of 16)
            const int g_base = min(P3_KC * chunk + 8 * octet, a.n_images - 1);
            const int g = g_base + min(lane >> 3, a.n_images - 1 - g_base); // padded images (zero weights) re-read the last one
            const int2 o = off_table[g];
            const int sy = clampi(y + o.y, 0, H - 1) - a.in_y0; // clamp in the full image, then index the held rows
            const int start = x0 + o.x + a.planar_padx;
            const uint8_t *src = a.planar + (size_t)g * 3 * shift_stride + (size_t)sy * a.planar_pitch + start + 16 * (lane & 7);
#pragma unroll
            for(int ch = 0; ch < 3; ch++)
                dma16(src + (size_t)ch * shift_stride, dst + uint32_t(ch * P3_CH_B + p3_octet_off(octet)));
        }
    };

    f32x4 acc[8][3]; // [block = pixel 8n + blk][channel]: views 4kg + i of this wave's 16
    auto clear_acc = [&] {
#pragma unroll
        for(int b = 0; b < 8; b++)
#pragma unroll
            for(int ch = 0; ch < 3; ch++)
                acc[b][ch] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    };

    // one chunk of images from buffer `buf` into acc, for the 16 views from vw on
    auto accumulate = [&](const int vw, const int chunk, const int buf) {
        const uint8_t *pb = lds + buf * P3_BUF_B;
        if constexpr(STD)
        {
            // acc = fmaf(px_g, w_g, acc), g ascending (chunks ascend too): src/kernels.cu:292-299, :328
            const int g_end = min(P3_KC, a.n_images - P3_KC * chunk);
            const float *wrow = a.w32 + (size_t)(vw + 4 * kg) * a.k_pad + P3_KC * chunk;
            for(int g4 = 0; g4 < g_end; g4 += 4) // rows are k_pad floats long (a multiple of 16): whole float4s, zero beyond the images
            {
                float4 w[4];
#pragma unroll
                for(int i = 0; i < 4; i++)
                    w[i] = *reinterpret_cast<const float4 *>(wrow + (size_t)i * a.k_pad + g4);
#pragma unroll
                for(int e = 0; e < 4; e++)
                {
                    const int gl = g4 + e;
                    if(gl >= g_end) // wave-uniform
                        break;
                    const uint8_t *row = pb + p3_octet_off(gl >> 3) + 128 * (gl & 7) + 8 * n;
#pragma unroll
                    for(int ch = 0; ch < 3; ch++)
                    {
                        __builtin_amdgcn_sched_barrier(0); // one channel's pixels at a time
                        const u32x2 p = *reinterpret_cast<const u32x2 *>(row + ch * P3_CH_B);
#pragma unroll
                        for(int b = 0; b < 8; b++)
                        {
                            const float px = float(((b < 4 ? p.x : p.y) >> (8 * (b & 3))) & 0xffu);
#pragma unroll
                            for(int i = 0; i < 4; i++)
                            {
                                const float wv = e == 0 ? w[i].x : e == 1 ? w[i].y : e == 2 ? w[i].z : w[i].w;
                                acc[b][ch][i] = __builtin_fmaf(px, wv, acc[b][ch][i]);
                            }
                        }
                    }
                }
            }
        }
        else
        {
            const int kc = min(P3_KC, a.k_pad - P3_KC * chunk);
            const int n_ks = kc > 32 ? 2 : 1; // wave-uniform: a chunk of ≤ 32 images has one k-step
#pragma unroll
            for(int ks = 0; ks < 2; ks++)
            {
                if(ks >= n_ks)
                    break;
                // A fragment: lane l: view l & 15, images 32ks + 8kg + j of the chunk
                const int k = P3_KC * chunk + 32 * ks + 8 * kg;
                u32x4 w = {0u, 0u, 0u, 0u};
                if(k < a.k_pad) // rows are k_pad halves long (a multiple of 16): nothing is read across a row's end
                    w = *reinterpret_cast<const u32x4 *>(a.w16s + (size_t)(vw + n) * a.k_pad + k);
                const half8 wk = __builtin_bit_cast(half8, w);
                const uint8_t *po = pb + p3_octet_off(4 * ks + kg) + 8 * n;
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
                            // [15:0] = byte (b & 3) of image 2q, [31:16] = the same byte of image 2q + 1: two fp16 subnormals
                            bf[q] = __builtin_amdgcn_perm(hi, lo, 0x0c000c00u | uint32_t(b & 3) | (uint32_t(4 + (b & 3)) << 16));
                        }
                        acc[b][ch] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wk, __builtin_bit_cast(half8, bf), acc[b][ch], 0, 0, 0);
                    }
                }
            }
        }
    };

    // quantise both ways, pack eight pixels per (view, channel), store
    auto epilogue = [&](const int t, const int vw, const int nvalid) {
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int x = tx * P3_TPX + 8 * n; // this lane's first pixel
        const bool x8 = x < a.views_pitch, x16 = 2 * x < deep_pitch; // both pitches ≥ the next multiple of 8 pixels: whole pieces stay inside the row
#pragma unroll
        for(int i = 0; i < 4; i++)
        {
            if(4 * kg + i >= nvalid)
                continue;
            const size_t plane0 = (size_t)(vw + 4 * kg + i) * 3;
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
                        // acc = S·2^-9 (weights × 2^15, pixels × 2^-24); RN-even to fp16 as blend_p3 rounds it, then floor(4·S) = floor(acc·2^11)
                        const float2_t f = {acc[2 * p][ch][i], acc[2 * p + 1][ch][i]};
                        const float2_t r = __builtin_convertvector(__builtin_convertvector(f, half2_t), float2_t); // v_cvt_pk_f16_f32, and back: exact
#pragma unroll
                        for(int e = 0; e < 2; e++)
                        {
                            code[2 * p + e] = uint32_t(min(1023, int(r[e] * 2048.0f))); // sums are ≥ 0 (weights in [0, 2)): the cast is the floor
                            byte[2 * p + e] = code[2 * p + e] >> 2;
                        }
                    }
                }
                const size_t row = (plane0 + ch) * (size_t)a.out_rows + ty;
                if(x8)
                    *reinterpret_cast<u32x2 *>(a.views + row * a.views_pitch + x) =
                        u32x2{byte[0] | (byte[1] << 8) | (byte[2] << 16) | (byte[3] << 24), byte[4] | (byte[5] << 8) | (byte[6] << 16) | (byte[7] << 24)};
                if(x16)
                    *reinterpret_cast<u32x4 *>(deep + row * deep_pitch + 2 * x) =
                        u32x4{code[0] | (code[1] << 16), code[2] | (code[3] << 16), code[4] | (code[5] << 16), code[6] | (code[7] << 16)};
            }
        }
    };

    // ---- the unit sequence of this workgroup: tiles t, t + G, …; chunks 0 … nch − 1 of each ----------------------------------------
    int t = blockIdx.x, chunk = 0, buf = 0;
    issue(t, 0, 0);
    for(;;)
    {
        int nt = t, nc = chunk + 1; // the next unit
        if(nc == nch)
            nc = 0, nt = t + G;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's pieces of the current unit have landed
        __syncthreads();                                 // everybody's have; everybody is done with the other buffer
        if(nt < n_tiles)
            issue(nt, nc, buf ^ 1);
        // one chunk of images: every view pass of the tile from the same LDS buffer (chunk is 0 throughout); several: view_passes is 1
        for(int pass = 0; pass < view_passes; pass++)
        {
            const int vw = a.v0 + 64 * pass + 16 * wave;
            const int nvalid = __builtin_amdgcn_readfirstlane(min(a.v1 - vw, 16));
            if(nvalid <= 0) // wave-uniform: this wave only helps with the fetch
                continue;
            if(chunk == 0)
                clear_acc();
            accumulate(vw, chunk, buf);
            if(chunk == nch - 1)
                epilogue(t, vw, nvalid);
        }
        if(nt >= n_tiles)
            break;
        t = nt, chunk = nc, buf ^= 1;
    }
}

} // namespace lfi
