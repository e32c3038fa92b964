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
// The skeleton — the tile, the LDS image, the fetch by LDS-DMA, the unit walk, the two accumulate loops, the weight walk and the byte-plane
// store — is blend_tile16.hpp's, shared with deep_blend.  No row window under the flag (flagged_refused): the context holds rows [0, H) of
// the inputs and renders rows [0, H), and the kernel reads none of KernelArgs' window fields.  What this file adds:
//   - the offset table in LDS keeps the raw (ox, oy) beside the phase-folded x offset;
//   - a tile is INTERIOR when every image has every pixel of the tile that lies in the frame in frame — decided per tile from the bounds of the
//     offsets (KernelArgs::fo_min / fo_max), scalar and workgroup-uniform.  A tile the bounds call a border tile although every image covers
//     it only takes the longer path to the same bytes.  Interior tiles run the shared loops unmasked, as deep_blend does: no mask, no den;
//     r = 1 there, so their bytes ARE the definition's;
//   - border tiles, per image and lane: the row test (wave-uniform) and the x interval [−ox − x_lane, W − ox − x_lane) cut to the lane's 8
//     pixels become a 64-bit byte mask that is ANDed onto the two dwords the lane read from LDS — before the STD conversions, before the
//     TEN_WM v_perm.  A left-out sample is a zero operand: with weights in [0, 2) and accumulators that start at +0, adding zero is skipping.
//     The clamped rows and the copy's padding are still FETCHED (the same addresses as deep_blend's), only never used;
//   - den[8][4] and wall[4]: fp32 accumulators carried across chunks; den by one fused multiply-add per (pixel, view) and image with the
//     multiplier 1.0f or 0.0f — fmaf(w, 1, den) is the rounded sum w + den, fmaf(w, 0, den) is den — for the images whose edge crosses the tile;
//     an image that has the whole tile in frame, or nothing of it (a scalar test per image), is a plain addition, or nothing;
//   - the border epilogue: one division per (pixel, view), one multiplication per channel, then the method's quantisation.
#pragma once

#include <type_traits>

#include "blend_tile16.hpp"

namespace lfi {

template <bool STD>
__global__ void __launch_bounds__(256, 2) blend_inframe(const KernelArgs a, const int tiles_x, const int n_tiles, const int view_passes, const int nch)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[T16_BUFS * P3_BUF_B + 2 * LFI_MAX_IMAGES * 8];

    const T16Lane L = t16_lane(lds);
    const int W = a.width, H = a.height;
    int2 *off_table = reinterpret_cast<int2 *>(lds + T16_BUFS * P3_BUF_B); // (ox + phase, oy): where the fetch starts
    int2 *raw_table = off_table + LFI_MAX_IMAGES;                          // (ox, oy): what is in frame
    t16_fill_offsets<true>(a, off_table, raw_table);
    if(int(blockIdx.x) >= n_tiles)
        return;

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
        const int y = ty, x = tx * P3_TPX + 8 * L.n; // this lane's first pixel
        // a border tile's image gl of the chunk: its mask, and its weights into den and wall
        auto border_image = [&](const int gl, const float (&wv)[4], u32x2 &mask) {
            int lo, hi;
            const int2 o = raw_table[P3_KC * chunk + gl];
            in_frame(o, x, y, lo, hi);
            mask = byte_mask(lo, hi);
            return weigh(wv, o, tx, y, lo, hi);
        };
        if constexpr(!BORDER)
        {
            if constexpr(STD)
                t16_std_chunk<false>(a, L, pb, vw, chunk, acc, T16Unmasked{});
            else
                t16_ten_chunk<false>(a, L, pb, vw, chunk, acc, T16Unmasked{});
        }
        else if constexpr(STD)
            t16_std_chunk<true>(a, L, pb, vw, chunk, acc, border_image); // false: every sample of the image is left out — 96 additions of zero
        else
        {
            // den and wall: the vector pipe's chain over the chunk's images in ascending order, from the fp32 rows the STD chain reads
            t16_weights(a, L, vw, chunk, [&](const int gl, const float (&wv)[4]) {
                u32x2 mask;
                border_image(gl, wv, mask);
            });
            t16_ten_chunk<true>(a, L, pb, vw, chunk, acc, [&](const int g) {
                int lo, hi;
                in_frame(raw_table[g], x, y, lo, hi);
                return byte_mask(lo, hi);
            });
        }
    };

    // (border tiles: scale by wall / den,) quantise, pack eight pixels per (view, channel), store
    auto epilogue = [&](const int ty, const int tx, const int vw, const int nvalid, auto border_c) {
        constexpr bool BORDER = decltype(border_c)::value;
        const int x = tx * P3_TPX + 8 * L.n; // this lane's first pixel
#pragma unroll
        for(int i = 0; i < 4; i++)
        {
            if(4 * L.kg + i >= nvalid)
                continue;
            const size_t plane0 = (size_t)(vw + 4 * L.kg + i) * 3;
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
                        const float2_t h = t16_ten_round(f); // acc·r is S·2^-9 as acc is
                        byte[2 * p] = t16_ten_byte(h[0]);
                        byte[2 * p + 1] = t16_ten_byte(h[1]);
                    }
                }
                t16_store_bytes(a, (plane0 + ch) * (size_t)H + ty, x, byte);
            }
        }
    };

    // One tile's units, on one of the two code paths.  den and wall are written and read on the border path only and cleared where it begins:
    // they hold no registers while an interior tile runs.
    int buf = 0;
    auto fetch = [&](const int t, const int chunk, const int buf) { t16_fetch(a, L, off_table, tiles_x, 0, 0, H, t, chunk, buf); };
    auto run_tile = [&](const int t, auto border_c) {
        constexpr bool BORDER = decltype(border_c)::value;
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        if constexpr(BORDER)
            clear_den();
        t16_tile(
            a, L, t, n_tiles, view_passes, nch, buf, fetch,
            [&] {
                t16_clear(acc);
                if constexpr(BORDER)
                    clear_den();
            },
            [&](const int vw, const int chunk, const int buf) { accumulate(ty, tx, vw, chunk, buf, border_c); },
            [&](const int vw, const int nvalid) { epilogue(ty, tx, vw, nvalid, border_c); });
    };
    fetch(blockIdx.x, 0, 0);
    for(int t = blockIdx.x; t < n_tiles; t += gridDim.x)
    {
        if(border_tile(t)) // scalar: the same for every chunk and pass of the tile
            run_tile(t, std::true_type{});
        else
            run_tile(t, std::false_type{});
    }
}

} // namespace lfi
