// blend_inframe.hpp — in-frame blending (LFI_FLAG_IN_FRAME, include/lfi.h): a fixed-focus render that LEAVES OUT the samples that fall outside
// their image instead of clamping them to its edge, and scales the rest back to the full weight.
//
// For view v, channel c, pixel (x, y), images g ascending, w_g the fp16 weight widened to fp32, (ox_g, oy_g) = focused_offsets[g]:
//      in_g  = 0 ≤ x + ox_g < W  and  0 ≤ y + oy_g < H
//      wall  = fp32 chain of w_g over all g;   den = fp32 chain of w_g over the g with in_g
//      num_c = STD: the reference's ordered chain num ← fmaf(px, w_g, num) (src/kernels.cu:292-299) over the g with in_g
//              TEN_WM: the fp32-accumulated matrix-core sum with the left-out samples as zeros
//      den == 0: s_c = 0;   otherwise r = wall / den (IEEE, RN), s_c = num_c · r (one fp32 multiplication, RN)
//      byte_c = STD: quant_rn(s_c)    TEN_WM: floor(min(fp16_RN(s_c), 255))
// den, wall and r are formed on the vector pipe, in ascending g, under BOTH methods: they are the same bits under both, and only num carries
// the matrix core's accumulation error.
//
// A sibling of deep_blend (deep_blend.hpp), whose skeleton it keeps: the planar copy by LDS-DMA into blend_p3's buffer image, persistent
// workgroups over 128-pixel tiles, units (tile, chunk of 64 images) in two buffers with ONE barrier per unit, a wave = 16 views, lane (n, kg)
// = pixels 8n … 8n + 7 of views 4kg + i, one 8-byte piece per (view, channel) into the byte plane.  No deep planes.  What it adds:
//   - the offset table in LDS keeps the raw (ox, oy) beside the phase-folded x offset;
//   - a tile is INTERIOR when every image has every pixel of the tile that lies in the frame in frame — decided per tile from the bounds of the
//     offsets (KernelArgs::fo_min / fo_max), scalar and workgroup-uniform.  A tile the bounds call a border tile although every image covers
//     it only takes the longer path to the same bytes.  Interior tiles run deep_blend's loops: no mask, no den; r = 1 there, so their bytes
//     ARE the definition's;
//   - border tiles, per image and lane: the row test (wave-uniform) and the x interval [−ox − x_lane, W − ox − x_lane) cut to the lane's 8
//     pixels become a 64-bit byte mask that is ANDed onto the two dwords the lane read from LDS — before the STD conversions, before the
//     TEN_WM v_perm.  A left-out sample is a zero operand: with weights in [0, 2) and accumulators that start at +0, adding zero is skipping.
//     The clamped rows and the copy's padding are still FETCHED (the same addresses as deep_blend's), only never used;
//   - den[8][4] and wall[4]: fp32 accumulators carried across chunks; den by one fused multiply-add per (pixel, view) and image with the
//     multiplier 1.0f or 0.0f — fmaf(w, 1, den) is the rounded sum w + den, fmaf(w, 0, den) is den — for the images whose edge crosses the tile;
//     an image that has the whole tile in frame, or nothing of it (a scalar test per image), is a plain addition, or nothing;
//   - the border epilogue: one division per (pixel, view), one multiplication per channel, then the method's quantisation.
// One chunk of images (up to 64): every 64-view pass of a tile reads the same LDS-resident pixels.  Several chunks: the host launches once per
// 64 views.
#pragma once

#include <type_traits>

#include "blend_p3.hpp"
#include "blend_std.hpp"

namespace lfi {

constexpr int INFRAME_BUFS = 2;

template <bool STD>
__global__ void __launch_bounds__(256, 2) blend_inframe(const KernelArgs a, const int tiles_x, const int n_tiles, const int view_passes, const int nch)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[INFRAME_BUFS * P3_BUF_B + 2 * LFI_MAX_IMAGES * 8];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lane & 15, kg = lane >> 4;
    const int W = a.width, H = a.height;
    const uint32_t lds_base = __builtin_amdgcn_readfirstlane(uint32_t(uintptr_t((lds_ptr_t)lds)));
    // (no row window under the flag — inframe_refused: the context holds rows [0, H) of the inputs and renders rows [0, H))
    const size_t shift_stride = (size_t)H * a.planar_pitch; // one byte plane of the planar inputs
    int2 *off_table = reinterpret_cast<int2 *>(lds + INFRAME_BUFS * P3_BUF_B); // (ox + phase, oy): where the fetch starts
    int2 *raw_table = off_table + LFI_MAX_IMAGES;                              // (ox, oy): what is in frame
    for(int g = threadIdx.x; g < a.n_images; g += 256)
    {
        const lfi_int2 o = a.focused[g];
        off_table[g] = make_int2(o.x + a.planar_phase[g], o.y); // the image's phase inside the planar copy folded into its x offset
        raw_table[g] = make_int2(o.x, o.y);
    }
    __syncthreads(); // the offset tables are complete
    const int G = gridDim.x;
    if(int(blockIdx.x) >= n_tiles)
        return;

    // the fetch of unit (tile t, chunk): deep_blend's, address for address (rows clamped in the full image, the run starts in the copy's
    // padding where the offset leads out of the image — those bytes are masked away below, not avoided)
    auto issue = [&](const int t, const int chunk, const int buf) {
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int y = ty, x0 = tx * P3_TPX;
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
            const int sy = clampi(y + o.y, 0, H - 1); // clamped to the image as the fetch of the clamping kernels is; masked below
            const int start = x0 + o.x + a.planar_padx;
            const uint8_t *src = a.planar + (size_t)g * 3 * shift_stride + (size_t)sy * a.planar_pitch + start + 16 * (lane & 7);
#pragma unroll
            for(int ch = 0; ch < 3; ch++)
                dma16(src + (size_t)ch * shift_stride, dst + uint32_t(ch * P3_CH_B + p3_octet_off(octet)));
        }
    };

    // is tile t a border tile?  Scalar: the bounds of the offsets against the tile's pixels that lie in the frame
    auto border_tile = [&](const int t) {
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int y = ty, x0 = tx * P3_TPX, x1 = min(x0 + P3_TPX, W) - 1;
        return !(x0 + a.fo_min_x >= 0 && x1 + a.fo_max_x < W && y + a.fo_min_y >= 0 && y + a.fo_max_y < H);
    };

    // which of this lane's 8 pixels (from x on, row y) image g (raw offsets o) has in frame: [lo, hi), empty where the row is out
    auto in_frame = [&](const int2 o, const int x, const int y, int &lo, int &hi) {
        const bool row_in = uint32_t(y + o.y) < uint32_t(H);
        lo = clampi(-o.x - x, 0, 8);
        hi = row_in ? clampi(W - o.x - x, 0, 8) : 0;
    };
    auto byte_mask = [](const int lo, const int hi) {
        const uint64_t m = hi > lo ? (~0ull >> (8 * (8 - (hi - lo)))) << (8 * lo) : 0ull;
        return u32x2{uint32_t(m), uint32_t(m >> 32)};
    };

    f32x4 acc[8][3]; // [block = pixel 8n + blk][channel]: views 4kg + i of this wave's 16
    f32x4 den[8];    // [pixel]: the in-frame weight of views 4kg + i (border tiles)
    f32x4 wall;      // the whole weight of views 4kg + i (border tiles)
    auto clear_den = [&] {
#pragma unroll
        for(int b = 0; b < 8; b++)
            den[b] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        wall = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    };
    auto clear_acc = [&] {
#pragma unroll
        for(int b = 0; b < 8; b++)
#pragma unroll
            for(int ch = 0; ch < 3; ch++)
                acc[b][ch] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    };

    // image g's weights wv[i] of views 4kg + i into wall and, for the pixels in [lo, hi), into den.  Most images of a border tile have the
    // whole tile in frame or none of it — a scalar test on the image's raw offsets o (the same in every lane): the one adds w to every den,
    // the other nothing, and only an image whose edge crosses the tile pays for the per-pixel multipliers.  false: the image has no pixel of the tile
    auto weigh = [&](const float (&wv)[4], const int2 o, const int tx, const int y, const int lo, const int hi) {
#pragma unroll
        for(int i = 0; i < 4; i++)
            wall[i] += wv[i];
        const int ox = __builtin_amdgcn_readfirstlane(o.x), oy = __builtin_amdgcn_readfirstlane(o.y);
        const int x0 = tx * P3_TPX + ox, x1 = min(tx * P3_TPX + P3_TPX, W) - 1 + ox; // where the tile's pixels that lie in the frame land in the image
        if(uint32_t(y + oy) >= uint32_t(H) || x1 < 0 || x0 >= W)
            return false;
        if(x0 >= 0 && x1 < W)
        {
#pragma unroll
            for(int b = 0; b < 8; b++)
#pragma unroll
                for(int i = 0; i < 4; i++)
                    den[b][i] += wv[i]; // (a ragged tile's pixels beyond W count it too: they are never shown)
            return true;
        }
#pragma unroll
        for(int b = 0; b < 8; b++)
        {
            const float m = (b >= lo && b < hi) ? 1.0f : 0.0f;
#pragma unroll
            for(int i = 0; i < 4; i++)
                den[b][i] = __builtin_fmaf(wv[i], m, den[b][i]); // w + den rounded once, or den
        }
        return true;
    };

    // one chunk of images from buffer `buf` into acc (border tiles: masked, and into den and wall), for the 16 views from vw on
    auto accumulate = [&](const int ty, const int tx, const int vw, const int chunk, const int buf, auto border_c) {
        constexpr bool BORDER = decltype(border_c)::value;
        const uint8_t *pb = lds + buf * P3_BUF_B;
        const int y = ty, x = tx * P3_TPX + 8 * n; // this lane's first pixel
        const int g_end = min(P3_KC, a.n_images - P3_KC * chunk);
        const float *wrow = a.w32 + (size_t)(vw + 4 * kg) * a.k_pad + P3_KC * chunk;
        if constexpr(STD)
        {
            // acc = fmaf(px_g, w_g, acc), g ascending (chunks ascend too): src/kernels.cu:292-299, :328
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
                    float wv[4];
#pragma unroll
                    for(int i = 0; i < 4; i++)
                        wv[i] = e == 0 ? w[i].x : e == 1 ? w[i].y : e == 2 ? w[i].z : w[i].w;
                    u32x2 mask = {~0u, ~0u};
                    if constexpr(BORDER)
                    {
                        int lo, hi;
                        const int2 o = raw_table[P3_KC * chunk + gl];
                        in_frame(o, x, y, lo, hi);
                        mask = byte_mask(lo, hi);
                        if(!weigh(wv, o, tx, y, lo, hi)) // wave-uniform: every sample of the image is left out — 96 additions of zero
                            continue;
                    }
                    const uint8_t *row = pb + p3_octet_off(gl >> 3) + 128 * (gl & 7) + 8 * n;
#pragma unroll
                    for(int ch = 0; ch < 3; ch++)
                    {
                        __builtin_amdgcn_sched_barrier(0); // one channel's pixels at a time
                        u32x2 p = *reinterpret_cast<const u32x2 *>(row + ch * P3_CH_B);
                        if constexpr(BORDER)
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
                }
            }
        }
        else
        {
            if constexpr(BORDER)
            {
                // den and wall: the vector pipe's chain over the chunk's images in ascending order, from the fp32 rows the STD chain reads
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
                        int lo, hi;
                        const int2 o = raw_table[P3_KC * chunk + gl];
                        in_frame(o, x, y, lo, hi);
                        weigh(wv, o, tx, y, lo, hi);
                    }
                }
            }
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
                u32x2 mask[8]; // of images k + j (padded images: the last one's, their weights are zero)
                if constexpr(BORDER)
                {
#pragma unroll
                    for(int j = 0; j < 8; j++)
                    {
                        int lo, hi;
                        in_frame(raw_table[min(k + j, a.n_images - 1)], x, y, lo, hi);
                        mask[j] = byte_mask(lo, hi);
                    }
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
                        if constexpr(BORDER)
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
    };

    // (border tiles: scale by wall / den,) quantise, pack eight pixels per (view, channel), store
    auto epilogue = [&](const int ty, const int tx, const int vw, const int nvalid, auto border_c) {
        constexpr bool BORDER = decltype(border_c)::value;
        const int x = tx * P3_TPX + 8 * n; // this lane's first pixel
        const bool x8 = x < a.views_pitch; // the pitch ≥ the next multiple of 8 pixels: whole pieces stay inside the row
#pragma unroll
        for(int i = 0; i < 4; i++)
        {
            if(4 * kg + i >= nvalid)
                continue;
            const size_t plane0 = (size_t)(vw + 4 * kg + i) * 3;
            if constexpr(BORDER)
            {
                // r = wall / den takes den's place (den is cleared before its next use); no image in frame (or only zero weights): the pixel is 0
#pragma unroll
                for(int b = 0; b < 8; b++)
                {
                    if((b & 1) == 0)
                        __builtin_amdgcn_sched_barrier(0); // two divisions at a time: each holds half a dozen temporaries
                    den[b][i] = den[b][i] == 0.0f ? 0.0f : __fdiv_rn(wall[i], den[b][i]);
                }
            }
#pragma unroll
            for(int ch = 0; ch < 3; ch++)
            {
                __builtin_amdgcn_sched_barrier(0); // one (view, channel) at a time
                uint32_t byte[8];
#pragma unroll
                for(int p = 0; p < 4; p++)
                {
                    float2_t f = {acc[2 * p][ch][i], acc[2 * p + 1][ch][i]};
                    if constexpr(BORDER)
                        f = float2_t{__fmul_rn(f[0], den[2 * p][i]), __fmul_rn(f[1], den[2 * p + 1][i])};
                    if constexpr(STD)
                    {
                        byte[2 * p] = quant_rn(f[0]);
                        byte[2 * p + 1] = quant_rn(f[1]);
                    }
                    else
                    {
                        // acc = S·2^-9 (weights × 2^15, pixels × 2^-24) and so is acc·r: RN-even to fp16 as blend_p3 rounds it, then floor(min(S, 255))
                        const float2_t h = __builtin_convertvector(__builtin_convertvector(f, half2_t), float2_t); // v_cvt_pk_f16_f32, and back: exact
#pragma unroll
                        for(int e = 0; e < 2; e++)
                            byte[2 * p + e] = uint32_t(fminf(h[e] * 512.0f, 255.0f)); // sums are ≥ 0 (weights in [0, 2)): the cast is the floor
                    }
                }
                const size_t row = (plane0 + ch) * (size_t)H + ty;
                if(x8)
                    *reinterpret_cast<u32x2 *>(a.views + row * a.views_pitch + x) =
                        u32x2{byte[0] | (byte[1] << 8) | (byte[2] << 16) | (byte[3] << 24), byte[4] | (byte[5] << 8) | (byte[6] << 16) | (byte[7] << 24)};
            }
        }
    };

    // ---- the unit sequence of this workgroup: tiles t, t + G, …; chunks 0 … nch − 1 of each ----------------------------------------
    // One tile's units, on one of the two code paths.  den and wall are written and read on the border path only and cleared where it begins:
    // they hold no registers while an interior tile runs.
    int buf = 0;
    auto run_tile = [&](const int t, auto border_c) {
        constexpr bool BORDER = decltype(border_c)::value;
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        if constexpr(BORDER)
            clear_den();
        for(int chunk = 0; chunk < nch; chunk++)
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
                {
                    clear_acc();
                    if constexpr(BORDER)
                        clear_den();
                }
                accumulate(ty, tx, vw, chunk, buf, border_c);
                if(chunk == nch - 1)
                    epilogue(ty, tx, vw, nvalid, border_c);
            }
            buf ^= 1;
        }
    };
    issue(blockIdx.x, 0, 0);
    for(int t = blockIdx.x; t < n_tiles; t += G)
    {
        if(border_tile(t)) // scalar: the same for every chunk and pass of the tile
            run_tile(t, std::true_type{});
        else
            run_tile(t, std::false_type{});
    }
}

} // namespace lfi
