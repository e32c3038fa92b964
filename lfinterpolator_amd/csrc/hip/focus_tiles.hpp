// focus_tiles.hpp — the focus curves of all tiles of a grid over the frame (lfi_focus_tiles), from ONE factored estimate.
//
// By definition tile (tx, ty)'s curve is what lfi_focus_curve gives for the tile's rectangle with 32 steps (focus_curve.hpp): cost[i] = Σ over
// the rectangle's pixels of the integer dispersion S_i.  The factored estimate (focus_factored.hpp) holds S_i for every pixel after
// focus_line_keys: the nine-sample sum of E_i (16·range + the FLT_MIN bit per tap) where the uniform shift is proven, the exact key K_i where
// the pair is flagged.  Both carry S in the same place: a nine-tap sum is 16·S + n with n ≤ 9 FLT_MIN taps, focus_key_encode keeps 16·S (or n
// alone when S = 0), so S = sum >> 4 = K >> 4 — the FLT_MIN bits are dropped, as lfi_focus_curve documents.  focus_pick keeps the argmin of the
// key per pixel and throws the cost away; focus_tile_costs, enqueued in its place, keeps the cost and adds it up per tile.
//
//   focus_tile_costs<PPL>  one workgroup (four waves) per (tile, band of 4·rows_per_wave rows, chunk of 64·PPL columns); a lane owns PPL ∈ {1, 2}
//                          adjacent columns, wave v the band's rows v, v + 4, …  PPL = 2 reads both pixels' samples of E with one dword load
//                          and needs an even radius_x and an even first column: the chunk starts at the tile's left edge rounded DOWN to even,
//                          and the columns outside [x0, x1) are masked out of the sum, not out of the loads (as focus_pick<2>'s lanes past the
//                          right edge, every load stays inside the workspace).  Per candidate a lane adds up S over its rows in a register and
//                          leaves it in LDS; then eight threads per candidate add the 256 lane sums (u32: 256 lanes × 2 pixels × 64 rows ×
//                          9 × 255 < 2^27) → partial[tile][candidate][workgroup] (u64).  No wave reduction inside the candidate loop, no atomics.
//   focus_curve_sum / focus_curve_pick (focus_curve.hpp) with the tile in blockIdx.y finish: cost[tile][32] and the first strict minimum.
// lfi_focus_tiles_steps (more than 32 candidates, a multiple of 32): the estimate runs one pass per 32 candidates (a.focus_i0 = 32g) and this
// kernel, unchanged, once per pass on the pass's E, K and flag bits 0 … 31 — the pass's first index only enters upstream, through
// focus_candidate; focus_curve_sum then writes the pass's slice cost[tile][32g … 32g + 31] (FocusCurveArgs::sum_at) and the partials are
// overwritten by the next pass; focus_curve_pick runs once over all the steps.  The u32 bound below is per pass.
// Every sum is an integer: exact in any order.
#pragma once

#include "focus_factored.hpp"
#include "focus_curve.hpp"

namespace lfi {

constexpr int FOCUS_TILE_MAX_ROWS_PER_WAVE = 64;

struct FocusTileArgs
{
    int32_t tiles_x, tiles_y;
    int32_t chunks;        // column chunks of 64·PPL pixels per tile (enough for the widest tile from an even first column)
    int32_t bands;         // row bands per tile (enough for the tallest tile)
    int32_t rows_per_wave; // a band = 4 waves × rows_per_wave rows
    uint32_t n_wg;         // chunks · bands: the pitch of partial[]
    uint64_t *partial;     // [tiles][32][n_wg]
};

// tile t of n over an axis of `size` pixels begins at floor(t · size / n) (lfi.h, lfi_host_focus_tile_rect)
__host__ __device__ __forceinline__ int focus_tile_edge(const int t, const int size, const int n)
{
    return static_cast<int>(static_cast<int64_t>(t) * size / n);
}

template <int PPL>
__global__ void __launch_bounds__(256) focus_tile_costs(const KernelArgs a, const FocusWork w, const FocusTileArgs q)
{
    __shared__ uint32_t lane_sum[FOCUS_STEPS][256];
    const int W = a.width, H = a.height, rx = a.radius_x, ry = a.radius_y;
    uint32_t b = blockIdx.x; // wave-uniform from here to the rows
    const uint32_t chunk = b % uint32_t(q.chunks);
    b /= uint32_t(q.chunks);
    const uint32_t band = b % uint32_t(q.bands), tile = b / uint32_t(q.bands);
    const int tx = int(tile % uint32_t(q.tiles_x)), ty = int(tile / uint32_t(q.tiles_x));
    const int x0 = focus_tile_edge(tx, W, q.tiles_x), x1 = focus_tile_edge(tx + 1, W, q.tiles_x);
    const int y0 = focus_tile_edge(ty, H, q.tiles_y), y1 = focus_tile_edge(ty + 1, H, q.tiles_y);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = (PPL == 2 ? (x0 & ~1) : x0) + (int(chunk) * 64 + lane) * PPL;
    // lanes past the right edge of the image sample pixel 0 and count nothing; the second pixel of a lane at x = W − 1 (odd W) reads one
    // element past a row of badx / E / K, inside the workspace (focus_pick<2> does the same), and is not counted either
    const int xs = x < W ? x : 0;
    bool inside[PPL];
    uint32_t flagged_x[PPL];
    bool any_inside = false;
#pragma unroll
    for(int j = 0; j < PPL; j++)
    {
        inside[j] = x + j >= x0 && x + j < x1;
        any_inside = any_inside || inside[j];
        flagged_x[j] = w.badx[xs + j];
    }
    const bool wave_inside = __builtin_amdgcn_ballot_w64(any_inside) != 0ull;
    const int y_first = y0 + int(band) * 4 * q.rows_per_wave + wave; // this wave's rows: y_first, y_first + 4, …
    const size_t plane_bytes = (size_t)w.He_p * w.We_p * 2;
    const uint8_t *plane = reinterpret_cast<const uint8_t *>(w.E);
    const uint16_t *exact = w.K + xs;

#pragma unroll 2
    for(int i = 0; i < FOCUS_STEPS; i++)
    {
        uint32_t s = 0;
        if(wave_inside)
            for(int r = 0, y = y_first; r < q.rows_per_wave && y < y1; r++, y += 4)
            {
                const uint32_t flagged_y = __builtin_amdgcn_readfirstlane(w.bady[y]);
                const uint8_t *e = plane + (size_t(y) * w.We_p + xs) * 2;
                uint32_t sum[PPL];
                focus_e_sum9<PPL>(sum, [&](const int t) { return e + uint32_t((t / 3) * ry * w.We_p + (t % 3) * rx) * 2u; });
                bool flagged[PPL], any = false;
#pragma unroll
                for(int j = 0; j < PPL; j++)
                {
                    flagged[j] = ((flagged_x[j] | flagged_y) >> i) & 1u;
                    any = any || flagged[j];
                }
                if(__builtin_amdgcn_ballot_w64(any) != 0ull) // wave-uniform; then every lane loads (a divergent load costs more than the unused values)
                {
                    const uint16_t *k = exact + ((size_t)i * H + y) * W;
#pragma unroll
                    for(int j = 0; j < PPL; j++)
                    {
                        const uint32_t key = k[j];
                        sum[j] = flagged[j] ? key : sum[j];
                    }
                }
#pragma unroll
                for(int j = 0; j < PPL; j++)
                    s += inside[j] ? sum[j] >> 4 : 0u; // S = key >> 4, for the nine-tap sum and for the encoded key alike
            }
        lane_sum[i][threadIdx.x] = s;
        plane += plane_bytes;
    }
    __syncthreads();
    // candidate c's 256 lane sums by threads 8c … 8c + 7 (thread p of them takes sums p, p + 8, …: neighbouring threads, neighbouring banks)
    const int c = threadIdx.x >> 3, p = threadIdx.x & 7;
    uint32_t s = 0;
#pragma unroll 8
    for(int k = 0; k < 32; k++)
        s += lane_sum[c][k * 8 + p];
    s = swizzle_sum_u32<3>(s); // the eight threads of a candidate are neighbours
    if(p == 0)
        q.partial[((size_t)tile * FOCUS_STEPS + c) * q.n_wg + band * uint32_t(q.chunks) + chunk] = s;
}

} // namespace lfi
