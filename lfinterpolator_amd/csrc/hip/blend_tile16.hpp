// blend_tile16.hpp — the skeleton the flagged fixed-focus kernels share (deep_blend.hpp, blend_inframe.hpp): device pieces, no kernel.
//
// A sibling of blend_p3 (blend_p3.hpp), whose tile, LDS image and operand maps it keeps:
//   - the planar, alpha-free copy of the inputs comes in through LDS by LDS-DMA (global_load_lds_dwordx4: 16 bytes per lane, eight lanes
//     per image row of the 128-pixel tile), into the image of a blend_p3 buffer: [channel][octet of images][8 images × 128 B], octets
//     padded by p3_octet_off so that the four octets one ds_read_b64 instruction touches fall into different banks;
//   - persistent workgroups walk the tiles t, t + G, …; a unit is (tile, chunk of 64 images); two buffers: the next unit's fetch is
//     issued before the current unit is computed, ONE barrier per unit.  The wait in front of the barrier is s_waitcnt vmcnt(0) — no
//     hand-counted waits: these kernels are paced by their stores and their arithmetic, and the wait drains the stores too;
//   - a wave = 128 pixels × 16 views; lane (n, kg) ends with pixels 8n … 8n + 7 of views 4kg + i of its wave's 16 in acc[pixel][channel][i];
//   - TEN_WM: v_mfma_f32_16x16x32_f16, A = weights × 2^15 (lane l: view l & 15, images 8(l >> 4) + j), B = pixels as fp16 subnormals (one
//     v_perm per image pair);
//   - STD: the same ownership on the vector pipe: per image one ds_read_b64 per channel (the four kg groups read the same address: a
//     broadcast) and 96 IEEE fused multiply-adds (the compiler pairs them as 48 v_pk_fma_f32: two fmas each, as blend_std_vfma's), images
//     in ascending order — the chain's value itself, not the band method's decision;
//   - a lane that ends with 8 consecutive pixels of a view and channel stores ONE 8-byte piece into the byte plane: 16 lanes write 128 B of a row.
// One chunk of images (up to 64): every 64-view pass of a tile reads the same LDS-resident pixels (any number of views in one launch).
// Several chunks: the host launches once per 64 views.
//
// A kernel's LDS: T16_BUFS buffers, then its offset table(s) of LFI_MAX_IMAGES int2 each.
#pragma once

#include "blend_p3.hpp"
#include "blend_std.hpp"

namespace lfi {

constexpr int T16_BUFS = 2;

// where a lane stands: pixels 8n … 8n + 7 of views 4kg + i of wave `wave`'s 16; lds_base = the workgroup's LDS as the DMA addresses it
struct T16Lane
{
    int lane, wave, n, kg;
    uint32_t lds_base;
};

__device__ __forceinline__ T16Lane t16_lane(const uint8_t *lds)
{
    const int lane = threadIdx.x & 63;
    return {lane, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane & 15, lane >> 4,
            uint32_t(__builtin_amdgcn_readfirstlane(uint32_t(uintptr_t((lds_ptr_t)lds))))};
}

// off_table[g] = (ox + phase, oy): where image g's fetch starts — its phase inside the planar copy folded into its x offset; raw_table[g]
// (where wanted) = (ox, oy).  Ends with the barrier that completes the tables: a workgroup without tiles returns AFTER it
template <bool RAW>
__device__ __forceinline__ void t16_fill_offsets(const KernelArgs &a, int2 *off_table, int2 *raw_table)
{
    for(int g = threadIdx.x; g < a.n_images; g += 256)
    {
        const lfi_int2 o = a.focused[g];
        off_table[g] = make_int2(o.x + a.planar_phase[g], o.y);
        if constexpr(RAW)
            raw_table[g] = make_int2(o.x, o.y);
    }
    __syncthreads();
}

// the fetch of unit (tile t, chunk) into buffer buf: wave w moves octets w and w + 4 of every channel; lane l the 16 bytes at 16·(l & 7) of
// the 128-byte run of image (l >> 3) of the octet.  Addressing is blend_p3's issue_piece: the run starts at pixel x0 + ox (+ the image's
// phase), the copy's padding exceeds every offset (ensure_planar), rows are clamped in the full image.  The row window — output row
// out_y0 + ty, rows [in_y0, in_y0 + in_rows) of the inputs held — comes in as values: a kernel without one passes 0, 0, H
__device__ __forceinline__ void t16_fetch(const KernelArgs &a, const T16Lane &L, const int2 *off_table, const int tiles_x, const int out_y0, const int in_y0,
                                          const int in_rows, const int t, const int chunk, const int buf)
{
    const size_t shift_stride = (size_t)in_rows * a.planar_pitch; // one byte plane of the planar inputs
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int y = out_y0 + ty, x0 = tx * P3_TPX;
    const int kc = min(P3_KC, a.k_pad - P3_KC * chunk);
    const uint32_t dst = L.lds_base + uint32_t(buf) * P3_BUF_B;
#pragma unroll
    for(int o2 = 0; o2 < 2; o2++)
    {
        const int octet = L.wave + 4 * o2;
        if(8 * octet >= kc)
            continue; // wave-uniform: the chunk is shorter (its length is a multiple of 16)
        const int g_base = min(P3_KC * chunk + 8 * octet, a.n_images - 1);
        const int g = g_base + min(L.lane >> 3, a.n_images - 1 - g_base); // padded images (zero weights) re-read the last one
        const int2 o = off_table[g];
        const int sy = clampi(y + o.y, 0, a.height - 1) - in_y0; // clamp in the full image, then index the held rows
        const int start = x0 + o.x + a.planar_padx;
        const uint8_t *src = a.planar + (size_t)g * 3 * shift_stride + (size_t)sy * a.planar_pitch + start + 16 * (L.lane & 7);
#pragma unroll
        for(int ch = 0; ch < 3; ch++)
            dma16(src + (size_t)ch * shift_stride, dst + uint32_t(ch * P3_CH_B + p3_octet_off(octet)));
    }
}

__device__ __forceinline__ void t16_clear(f32x4 (&acc)[8][3])
{
#pragma unroll
    for(int b = 0; b < 8; b++)
#pragma unroll
        for(int ch = 0; ch < 3; ch++)
            acc[b][ch] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}

// the images of a chunk in ascending order with their fp32 weights: per_image(gl, wv) with gl the image's index inside the chunk and wv[i]
// its weight for view vw + 4kg + i.  Rows are k_pad floats long (a multiple of 16): whole float4s, zero beyond the images
template <class PerImage>
__device__ __forceinline__ void t16_weights(const KernelArgs &a, const T16Lane &L, const int vw, const int chunk, PerImage per_image)
{
    const int g_end = min(P3_KC, a.n_images - P3_KC * chunk);
    const float *wrow = a.w32 + (size_t)(vw + 4 * L.kg) * a.k_pad + P3_KC * chunk;
    for(int g4 = 0; g4 < g_end; g4 += 4)
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
            float wv[4];
#pragma unroll
            for(int i = 0; i < 4; i++)
                wv[i] = e == 0 ? w[i].x : e == 1 ? w[i].y : e == 2 ? w[i].z : w[i].w;
            per_image(gl, wv);
        }
    }
}

// what a kernel without a mask passes for the callables below
struct T16Unmasked
{
    __device__ __forceinline__ bool operator()(int, const float (&)[4], u32x2 &) const { return true; }
    __device__ __forceinline__ u32x2 operator()(int) const { return u32x2{~0u, ~0u}; }
};

// STD, one chunk of images from the buffer at pb into acc, for the 16 views from vw on: acc = fmaf(px_g, w_g, acc), g ascending (chunks
// ascend too): src/kernels.cu:292-299, :328.  per_image(gl, wv, mask) comes first for every image: false skips the image (wave-uniform);
// MASKED: the byte mask it sets is ANDed onto the two dwords the lane read — a left-out sample is a zero operand
template <bool MASKED, class PerImage>
__device__ __forceinline__ void t16_std_chunk(const KernelArgs &a, const T16Lane &L, const uint8_t *pb, const int vw, const int chunk, f32x4 (&acc)[8][3],
                                              PerImage per_image)
{
    t16_weights(a, L, vw, chunk, [&](const int gl, const float (&wv)[4]) {
        u32x2 mask = {~0u, ~0u};
        if(!per_image(gl, wv, mask))
            return;
        const uint8_t *row = pb + p3_octet_off(gl >> 3) + 128 * (gl & 7) + 8 * L.n;
#pragma unroll
        for(int ch = 0; ch < 3; ch++)
        {
            __builtin_amdgcn_sched_barrier(0); // one channel's pixels at a time
            u32x2 p = *reinterpret_cast<const u32x2 *>(row + ch * P3_CH_B);
            if constexpr(MASKED)
                p &= mask;
#pragma unroll
            for(int b = 0; b < 8; b++)
            {
                const float px = float(((b < 4 ? p.x : p.y) >> (8 * (b & 3))) & 0xffu);
#pragma unroll
                for(int i = 0; i < 4; i++)
                    acc[b][ch][i] = __builtin_fmaf(px, wv[i], acc[b][ch][i]);
            }
        }
    });
}

// TEN_WM, one chunk of images from the buffer at pb into acc, for the 16 views from vw on.  MASKED: mask_of(g) is ANDed onto the lane's
// two dwords of image g before the v_perm (padded images: the last one's g, their weights are zero)
template <bool MASKED, class MaskOf>
__device__ __forceinline__ void t16_ten_chunk(const KernelArgs &a, const T16Lane &L, const uint8_t *pb, const int vw, const int chunk, f32x4 (&acc)[8][3],
                                              MaskOf mask_of)
{
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
            w = *reinterpret_cast<const u32x4 *>(a.w16s + (size_t)(vw + L.n) * a.k_pad + k);
        const half8 wk = __builtin_bit_cast(half8, w);
        const uint8_t *po = pb + p3_octet_off(4 * ks + L.kg) + 8 * L.n;
        u32x2 mask[8];
        if constexpr(MASKED)
        {
#pragma unroll
            for(int j = 0; j < 8; j++)
                mask[j] = mask_of(min(k + j, a.n_images - 1));
        }
#pragma unroll
        for(int ch = 0; ch < 3; ch++)
        {
            __builtin_amdgcn_sched_barrier(0); // one group's reads at a time: the accumulators leave few registers to hoist into
            u32x2 d[8]; // the lane's eight pixels of images 8(4ks + kg) + j
#pragma unroll
            for(int j = 0; j < 8; j++)
            {
                d[j] = *reinterpret_cast<const u32x2 *>(po + ch * P3_CH_B + 128 * j);
                if constexpr(MASKED)
                    d[j] &= mask[j];
            }
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

// TEN_WM's accumulator is S·2^-9 (weights × 2^15, pixels × 2^-24): RN-even to fp16 as blend_p3 rounds it (v_cvt_pk_f16_f32), and back: exact
__device__ __forceinline__ float2_t t16_ten_round(const float2_t f)
{
    return __builtin_convertvector(__builtin_convertvector(f, half2_t), float2_t);
}

// … and its byte floor(min(S, 255)) from the rounded value: sums are ≥ 0 (weights in [0, 2)), so the cast is the floor.  (STD's byte: quant_rn)
__device__ __forceinline__ uint32_t t16_ten_byte(const float h)
{
    return uint32_t(fminf(h * 512.0f, 255.0f));
}

// the lane's 8 pixels from x on of byte-plane row `row` (a row index over all planes) as ONE 8-byte piece.  views_pitch ≥ the next multiple
// of 8 pixels: whole pieces stay inside the row
__device__ __forceinline__ void t16_store_bytes(const KernelArgs &a, const size_t row, const int x, const uint32_t (&byte)[8])
{
    if(x < a.views_pitch)
        *reinterpret_cast<u32x2 *>(a.views + row * a.views_pitch + x) =
            u32x2{byte[0] | (byte[1] << 8) | (byte[2] << 16) | (byte[3] << 24), byte[4] | (byte[5] << 8) | (byte[6] << 16) | (byte[7] << 24)};
}

// The unit sequence of a workgroup is tiles t, t + G, …, chunks 0 … nch − 1 of each: the kernel issues fetch(blockIdx.x, 0, 0), then calls this
// for its tiles in turn with the same buf (0 at first) — on whichever of its code paths the tile takes, a scalar choice.  (That loop stays in the
// kernel: with it here, behind one more closure, blend_inframe compiled to 82–257 spilled VGPRs — profiles/r30_tile16_notes.md.)  Here: tile
// t's units from buffer buf on.  fetch(t, chunk, buf) issues a unit's DMA; per view pass, for the 16 views from vw on of which nvalid exist:
// clear() at the first chunk, accumulate(vw, chunk, buf) per chunk, epilogue(vw, nvalid) after the last.  One chunk of images: every view
// pass of the tile from the same LDS buffer; several: view_passes is 1
template <class Fetch, class Clear, class Accumulate, class Epilogue>
__device__ __forceinline__ void t16_tile(const KernelArgs &a, const T16Lane &L, const int t, const int n_tiles, const int view_passes, const int nch, int &buf,
                                         Fetch fetch, Clear clear, Accumulate accumulate, Epilogue epilogue)
{
    const int G = gridDim.x;
    for(int chunk = 0; chunk < nch; chunk++)
    {
        int nt = t, nc = chunk + 1; // the next unit
        if(nc == nch)
            nc = 0, nt = t + G;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's pieces of the current unit have landed
        __syncthreads();                                 // everybody's have; everybody is done with the other buffer
        if(nt < n_tiles)
            fetch(nt, nc, buf ^ 1);
        for(int pass = 0; pass < view_passes; pass++)
        {
            const int vw = a.v0 + 64 * pass + 16 * L.wave;
            const int nvalid = __builtin_amdgcn_readfirstlane(min(a.v1 - vw, 16));
            if(nvalid <= 0) // wave-uniform: this wave only helps with the fetch
                continue;
            if(chunk == 0)
                clear();
            accumulate(vw, chunk, buf);
            if(chunk == nch - 1)
                epilogue(vw, nvalid);
        }
        buf ^= 1;
    }
}

} // namespace lfi
