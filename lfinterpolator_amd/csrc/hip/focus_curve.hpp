// focus_curve.hpp — the focus curve of a region (lfi_focus_curve): cost[i] = Σ over the region's pixels of the integer dispersion S_i of
// focus candidate f_i = fma(range / (steps − 1), i, focus), and the first candidate with the strictly smallest cost.
//
// S_i(x, y) is FocusMap::focusDispersion (reference src/kernels.cu:196-217, ElementRange :173-194) in the integer formulation of
// focus_estimate_packed (focus_map.hpp: its exactness argument holds here unchanged): over the n_focus_ids sampled images, per tap of the
// 3 × 3 block the largest channel's max − min, summed over the nine taps.  The estimate keeps the per-pixel argmin of it (MinDispersion,
// :219-237) and throws the cost away; here the cost is kept and summed over the region instead.  One departure from the float code: the
// reference's FLT_MIN start value (:178) makes an all-zero tap contribute 1.2e-38 instead of 0 — those terms cannot be added meaningfully
// over a region and are dropped (S_i is the plain integer sum).
//
// Three kernels, no atomics, every sum an integer (exact, order-independent):
//   focus_curve_partial   region × candidates.  Sampled as focus_estimate_packed samples (focus_map.hpp; the candidate's value and a tap's dispersion by
//                         its helpers focus_sweep_value and focus_tap_range, the tap loads written out again here): a lane owns PPL consecutive
//                         pixels of a row, a tap is one wide load where the per-lane exactness check allows it (else per-pixel clamped
//                         fetches), min / max over the images on v_pk_min_u16 / v_pk_max_u16.  Per candidate the lane's S of the pixels
//                         INSIDE the region (the ragged right edge is masked out of the sum, not out of the sampling) is reduced over the
//                         wave (u32: 64 lanes × 4 pixels × 9 × 255 < 2^20) and added to the workgroup's u64 accumulator in LDS; a workgroup
//                         (one wave) walks the region's rows blockIdx.y, blockIdx.y + gridDim.y, … and stores its accumulators once, as
//                         partial[candidate][workgroup].  A region too small to fill the GPU with one wave per 128 pixels of a row is also
//                         split along the candidates (blockIdx.z): a wave's life is its candidates × images × 9 dependent taps.
//   (focus_curve_sum and focus_curve_pick also finish lfi_focus_tiles' curves, focus_tiles.hpp: one more grid dimension, the tile)
//   focus_curve_sum       one workgroup per candidate sums that candidate's partials in a fixed order → cost[candidate].
//   focus_curve_pick      the first strict minimum of cost[] (MinDispersion's rule) → {best_index, best_focus, pixels}.
// The candidates are a run-time loop (2 ≤ steps ≤ 256), not the estimate's unrolled 32.
#pragma once

#include "focus_map.hpp"

namespace lfi {

constexpr int FOCUS_CURVE_MAX_STEPS = 256;

struct FocusCurveArgs
{
    int32_t x0, y0, x1, y1; // the region [x0, x1) × [y0, y1), inside the image
    int32_t steps;
    int32_t steps_per_wg;   // candidates per workgroup: blockIdx.z takes candidates [z · steps_per_wg, (z + 1) · steps_per_wg) (small regions)
    uint32_t n_wg;          // gridDim.x · gridDim.y of focus_curve_partial: the pitch of partial[]
    uint64_t pixels;
    uint64_t *partial;      // [steps][n_wg]
    uint64_t *cost;         // [steps], followed by the result (lfi_focus_curve_result's layout: i32, f32, u64)
    int32_t tiled;          // lfi_focus_tiles: focus_curve_sum / focus_curve_pick run once per tile of a gridDim tiles_x × tiles_y grid — tile t's
                            // partials are partial[t][gridDim.x][n_wg], its curve and result lie at cost + t · (steps + 2), its pixels are its rectangle's
    int32_t sum_at;         // focus_curve_sum: its gridDim.x candidates are sum_at … sum_at + gridDim.x − 1 of the curve's steps (0 and all of them
                            // everywhere but lfi_focus_tiles_steps, whose partials hold one pass of 32 candidates at a time)
};

// focus_curve_sum's grid is (candidates summed: steps, or one pass's 32) × tiles_x × tiles_y, focus_curve_pick's tiles_x × tiles_y; lfi_focus_curve launches them with one tile (tile 0)
constexpr int FOCUS_CURVE_RESULT_WORDS = 2;
static_assert(sizeof(lfi_focus_curve_result) == sizeof(uint64_t) * FOCUS_CURVE_RESULT_WORDS, "the result follows the curve in u64 words");

// v + the values of the lanes whose number differs from this one's in the lowest STEPS bits (STEPS ≤ 5): a butterfly of ds_swizzle steps with
// an immediate lane pattern (bit-mask mode: lane' = (lane & 0x1f) ^ m) — no address register, unlike ds_bpermute
template <int STEPS>
__device__ __forceinline__ uint32_t swizzle_sum_u32(uint32_t v)
{
    static_assert(STEPS >= 1 && STEPS <= 5, "ds_swizzle's bit-mask mode reaches 32 lanes");
    v += (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (1 << 10) | 0x1f);
    if constexpr(STEPS > 1)
        v += (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (2 << 10) | 0x1f);
    if constexpr(STEPS > 2)
        v += (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (4 << 10) | 0x1f);
    if constexpr(STEPS > 3)
        v += (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (8 << 10) | 0x1f);
    if constexpr(STEPS > 4)
        v += (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (16 << 10) | 0x1f);
    return v;
}

// the sum of v over the wave's 64 lanes, wave-uniform: each half's sum by the butterfly (focus_curve_partial lives at the edge of five waves
// per SIMD), then the two halves' sums by v_readlane
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
    v = swizzle_sum_u32<5>(v);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 32);
}

template <int PPL, int WPE>
__global__ void __launch_bounds__(64, WPE) focus_curve_partial(const KernelArgs a, const FocusCurveArgs q)
{
    __shared__ uint64_t acc[FOCUS_CURVE_MAX_STEPS];
    constexpr int NP = PPL / 2; // pixel pairs per lane
    const int lane = threadIdx.x & 63;
    const int W = a.width, H = a.height;
    const int x0 = q.x0 + (blockIdx.x * 64 + lane) * PPL; // first of this lane's pixels: the region's left edge needs no alignment
    const bool lane_active = x0 < q.x1;
    const int steps = q.steps;
    const float div = static_cast<float>(steps - 1);
    const int rx = a.radius_x, ry = a.radius_y;
    const uint32_t *grid32 = reinterpret_cast<const uint32_t *>(a.grid);
    const size_t plane_px = (size_t)W * (size_t)H; // no row window (the host refuses it)
    typedef const __attribute__((address_space(4))) float *const_float_ptr;
    typedef const __attribute__((address_space(4))) int32_t *const_int_ptr;
    const const_float_ptr c_offsets = (const_float_ptr)(uintptr_t)a.offsets;
    const const_int_ptr c_ids = (const_int_ptr)(uintptr_t)a.focus_ids;
    // which of the lane's pixels lie inside the region, as a mask over the u16 pairs
    uint32_t in_mask[NP];
#pragma unroll
    for(int p = 0; p < NP; p++)
        in_mask[p] = (x0 + 2 * p < q.x1 ? 0x0000ffffu : 0u) | (x0 + 2 * p + 1 < q.x1 ? 0xffff0000u : 0u);

    const int i_begin = (int)blockIdx.z * q.steps_per_wg, i_end = min(steps, i_begin + q.steps_per_wg); // wave-uniform
    for(int i = i_begin + lane; i < i_end; i += 64)
        acc[i] = 0;
    __syncthreads();

    for(int y = q.y0 + (int)blockIdx.y; y < q.y1; y += (int)gridDim.y) // wave-uniform
        for(int i = i_begin; i < i_end; i++)
        {
            const float f = focus_sweep_value(a.focus, a.range, div, i);
            // running min / max per tap (9), pixel pair and channel (3), as u16 pairs
            u16x2 lo[9][NP][3], hi[9][NP][3];
#pragma unroll
            for(int t = 0; t < 9; t++)
#pragma unroll
                for(int p = 0; p < NP; p++)
#pragma unroll
                    for(int c = 0; c < 3; c++)
                    {
                        lo[t][p][c] = as_u16x2(0x00ff00ffu);
                        hi[t][p][c] = as_u16x2(0u);
                    }
            for(int k = 0; k < a.n_focus_ids; k++)
            {
                const int g = c_ids[k];
                const float offx = c_offsets[2 * g], offy = c_offsets[2 * g + 1];
                const uint32_t *plane = grid32 + (size_t)g * plane_px;
                int cx[PPL];
#pragma unroll
                for(int j = 0; j < PPL; j++)
                    cx[j] = warp_float(x0 + j, f, offx);
                const int cy = warp_float(y, f, offy);
                bool consecutive = true;
#pragma unroll
                for(int j = 1; j < PPL; j++)
                    consecutive = consecutive && (cx[j] == cx[0] + j);
                // per lane: one wide load per tap is valid when the sample columns are consecutive and no x-clamp can touch them
                const bool vec_ok = consecutive && (cx[0] - rx >= 0) && (cx[PPL - 1] + rx <= W - 1) && (x0 + PPL - 1 < W);
                if(lane_active)
                {
#pragma unroll
                    for(int ty = 0; ty < 3; ty++)
                    {
                        const uint32_t *row = plane + (size_t)clampi(cy + (ty - 1) * ry, 0, H - 1) * W;
#pragma unroll
                        for(int tx = 0; tx < 3; tx++)
                        {
                            uint32_t px[PPL];
                            if(vec_ok)
                            {
                                if constexpr(PPL == 4)
                                {
                                    const u32x4_a4 v = *reinterpret_cast<const u32x4_a4 *>(row + cx[0] + (tx - 1) * rx);
                                    px[0] = v.x;
                                    px[1] = v.y;
                                    px[2] = v.z;
                                    px[3] = v.w;
                                }
                                else
                                {
                                    const u32x2_a4 v = *reinterpret_cast<const u32x2_a4 *>(row + cx[0] + (tx - 1) * rx);
                                    px[0] = v.x;
                                    px[1] = v.y;
                                }
                            }
                            else
                            {
#pragma unroll
                                for(int j = 0; j < PPL; j++)
                                    px[j] = row[clampi(cx[j] + (tx - 1) * rx, 0, W - 1)];
                            }
                            const int t = tx * 3 + ty;
#pragma unroll
                            for(int p = 0; p < NP; p++)
                            {
                                const u16x2 cr = channel_pair<0>(px[2 * p], px[2 * p + 1]);
                                const u16x2 cg = channel_pair<1>(px[2 * p], px[2 * p + 1]);
                                const u16x2 cb = channel_pair<2>(px[2 * p], px[2 * p + 1]);
                                lo[t][p][0] = __builtin_elementwise_min(lo[t][p][0], cr);
                                hi[t][p][0] = __builtin_elementwise_max(hi[t][p][0], cr);
                                lo[t][p][1] = __builtin_elementwise_min(lo[t][p][1], cg);
                                hi[t][p][1] = __builtin_elementwise_max(hi[t][p][1], cg);
                                lo[t][p][2] = __builtin_elementwise_min(lo[t][p][2], cb);
                                hi[t][p][2] = __builtin_elementwise_max(hi[t][p][2], cb);
                            }
                        }
                    }
                }
            }
            // dispersion of this candidate: the integer sum S per pixel (at most 9 · 255: a u16), the pixels inside the region added up
            uint32_t s_lane = 0;
#pragma unroll
            for(int p = 0; p < NP; p++)
            {
                u16x2 sum = as_u16x2(0u);
#pragma unroll
                for(int t = 0; t < 9; t++)
                    sum += focus_tap_range(lo[t][p], hi[t][p]);
                const uint32_t s = as_u32(sum) & in_mask[p];
                s_lane += (s & 0xffffu) + (s >> 16);
            }
            if(!lane_active)
                s_lane = 0; // (its min / max never left their start values)
            const uint32_t s_wave = wave_sum_u32(s_lane);
            if(lane == 0)
                acc[i] += s_wave;
        }
    __syncthreads();
    const uint32_t wg = blockIdx.y * gridDim.x + blockIdx.x;
    for(int i = i_begin + lane; i < i_end; i += 64)
        q.partial[(size_t)i * q.n_wg + wg] = acc[i];
}

// cost[sum_at + candidate] = Σ of the candidate's partials: thread t takes partials t, t + 256, …, then the 256 thread sums are added in a tree of
// fixed shape — integer sums, so the order could not matter anyway
__global__ void __launch_bounds__(256) focus_curve_sum(const FocusCurveArgs q)
{
    __shared__ uint64_t part[256];
    const size_t tile = (size_t)blockIdx.z * gridDim.y + blockIdx.y;
    const uint64_t *src = q.partial + (tile * gridDim.x + blockIdx.x) * q.n_wg;
    uint64_t s = 0;
    for(uint32_t w = threadIdx.x; w < q.n_wg; w += 256)
        s += src[w];
    part[threadIdx.x] = s;
    __syncthreads();
    for(int m = 128; m >= 1; m >>= 1)
    {
        if((int)threadIdx.x < m)
            part[threadIdx.x] += part[threadIdx.x + m];
        __syncthreads();
    }
    if(threadIdx.x == 0)
        q.cost[tile * (q.steps + FOCUS_CURVE_RESULT_WORDS) + q.sum_at + blockIdx.x] = part[0];
}

// the first candidate with the strictly smallest cost (MinDispersion::add, src/kernels.cu:225-231: strict <, candidates in ascending order)
__global__ void __launch_bounds__(256) focus_curve_pick(const KernelArgs a, const FocusCurveArgs q)
{
    __shared__ uint64_t best_cost[256];
    __shared__ int32_t best_at[256];
    const int t = threadIdx.x;
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    uint64_t *cost = q.cost + tile * (q.steps + FOCUS_CURVE_RESULT_WORDS);
    best_cost[t] = t < q.steps ? cost[t] : ~0ull;
    best_at[t] = t < q.steps ? t : 0x7fffffff;
    __syncthreads();
    for(int m = 128; m >= 1; m >>= 1)
    {
        if(t < m)
        {
            const uint64_t c = best_cost[t + m];
            const int32_t at = best_at[t + m];
            if(c < best_cost[t] || (c == best_cost[t] && at < best_at[t]))
            {
                best_cost[t] = c;
                best_at[t] = at;
            }
        }
        __syncthreads();
    }
    if(t == 0)
    {
        lfi_focus_curve_result r;
        r.best_index = best_at[0];
        r.best_focus = focus_sweep_value(a.focus, a.range, static_cast<float>(q.steps - 1), best_at[0]);
        r.pixels = q.pixels;
        if(q.tiled) // tile (blockIdx.x, blockIdx.y) begins at floor(t · size / tiles) on either axis (lfi.h)
        {
            const int64_t bx = blockIdx.x, by = blockIdx.y, nx = gridDim.x, ny = gridDim.y;
            r.pixels = uint64_t((bx + 1) * a.width / nx - bx * a.width / nx) * uint64_t((by + 1) * a.height / ny - by * a.height / ny);
        }
        *reinterpret_cast<lfi_focus_curve_result *>(cost + q.steps) = r;
    }
}

} // namespace lfi
