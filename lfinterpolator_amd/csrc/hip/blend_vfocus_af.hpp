// blend_vfocus_af.hpp — all-focus renders with float offsets PER VIEW (lfi_set_view_float_offsets): every view shifted about its own camera.
//
// Every other all-focus kernel here samples image g of every view at (int)fma(f(x,y), offsets[g], x) with one row of float offsets, computed
// for the trajectory's centre (reference src/interpolator.cu:226-246, loadGPUOffsets → trajectoryCenter).  Here view v samples at
// (int)fma(f(x,y), O[v][g], x): the sample depends on the view, the image and the pixel's focus, so neither a shared pixel operand (no MFMA
// formulation) nor a shared sample across views exists.  A vector-pipe gather-blend, on the skeleton of blend_vfocus.hpp:
//
//   workgroup   4 waves, one output row each, 256 pixels per wave (4 consecutive pixels per lane), VIEWS views (VF_VIEWS)
//   focus       each lane decodes its 4 pixels' focus once, before the image loop (loadFocusFromMap, src/kernels.cu:134-137): the map the
//               method reads (map 1 for STD, map 0 for TEN_WM, map 1 for both with LFI_FLAG_UNIFIED_FOCUS_MAP), at the view's own pixel.
//               VIEW_MAPS (lfi_view_focus_maps): each view of the chunk has its own map pair, f[VIEWS][4] decoded once before the loop
//               (+(VIEWS − 1)·4 VGPRs; the chunk size of that variant is chosen so that it does not spill: DESIGN.md §4.8)
//   loop        g outermost (ascending: the chain order of the reference's STD kernel, src/kernels.cu:328-338), the chunk's views inner;
//               O[v][g] and the weight are wave-uniform scalar loads ([g][view] layouts: one run of VF_VIEWS float2 / floats per g)
//   sources     the RGBA planes only, one dword gather per (view, image, pixel) with clamp-to-edge (surf2Dread's cudaBoundaryModeClamp,
//               src/kernels.cu:119-126), through a buffer resource per image plane (32-bit offsets; a stray index reads 0, not memory)
//   outputs     RGBA views (one 16-byte store per lane) or the planar view layout (one dword per lane and channel)
//   order       the view chunk varies fastest over the block index: the chunks of one tile run side by side and share its input rows
//
// Numerics, both methods: acc = fmaf(float(px), w32[v][g], acc) over ascending g from 0 — blend_vfocus's chain at the all-focus sample.
//   STD     the reference's Standard::process chain (src/kernels.cu:289-343) itself, then (unsigned char)__float2int_rn: bit-exact.
//   TEN_WM  the fp32-accumulated sum of the exact byte × fp16-weight products, rounded once to fp16 (RN-even) and truncated with saturation
//           like __half2uchar_rz (src/kernels.cu:393).  The matrix cores are not used.
#pragma once

#include "blend_vfocus.hpp"

namespace lfi {

// views per workgroup of the per-view-map variant (VIEW_MAPS): its focus of VM_VIEWS views stays in registers beside the accumulators
constexpr int VM_VIEWS = 8;

// grid: n_chunks × tiles_x × ceil(out_rows / VF_ROWS) blocks of 256 threads.
// vo: [n_images][vo_pitch] float offsets of views [0, vo_pitch), views contiguous; w32t: a.w32t ([k_pad][v_pad]).  Both are zero for the
// padding views, so a chunk that runs past a.v1 reads defined values; it stores views < a.v1 only.
// rows: the dispatcher has checked that every row the band samples is held (row windows); the clamp below only keeps a stray index inside
// the planes.
template <bool TEN, bool PLANAR_OUT, int VIEWS = VF_VIEWS, bool VIEW_MAPS = false>
__global__ void __launch_bounds__(256) blend_vfocus_af(const KernelArgs a, const lfi_float2 *__restrict__ vo, const int vo_pitch, const int n_chunks,
                                                       const int tiles_x)
{
    const int chunk = blockIdx.x % n_chunks, tile = blockIdx.x / n_chunks;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int yl = ty * VF_ROWS + wave; // row inside the output window
    if(yl >= a.out_rows)
        return; // wave-uniform
    const int W = a.width, H = a.height;
    const int y = a.out_y0 + yl;
    const int x0 = tx * VF_TILE_W + lane * VF_PX;
    const int vbase = a.v0 + chunk * VIEWS;

    // maps are whole-image planes; decode_focus clamps the pixels past the right edge (their results are not stored).
    // VIEW_MAPS: a.maps is [views][2][H][W] (lfi_view_focus_maps) and every view of the chunk decodes its own pair's map; the padding views
    // past a.v1 (not stored) read the last view's, so no read leaves the views' maps
    constexpr int NF = VIEW_MAPS ? VIEWS : 1;
    float f[NF][VF_PX];
#pragma unroll
    for(int j = 0; j < NF; j++)
    {
        const size_t pair = VIEW_MAPS ? (size_t)min(vbase + j, a.v1 - 1) * 2 : 0;
        const uint8_t *map_plane = a.maps + (pair + (size_t)a.map_index) * (size_t)W * H * 4;
#pragma unroll
        for(int i = 0; i < VF_PX; i++)
            f[j][i] = decode_focus(map_plane, W, H, x0 + i, y, a.focus, a.range);
    }

    float acc[VIEWS][3][VF_PX];
#pragma unroll
    for(int j = 0; j < VIEWS; j++)
#pragma unroll
        for(int c = 0; c < 3; c++)
#pragma unroll
            for(int i = 0; i < VF_PX; i++)
                acc[j][c][i] = 0.0f;

    const int plane_bytes = a.in_rows * W * 4; // ≤ 2^28 (lfi_set_grid)
    for(int g = 0; g < a.n_images; g++)
    {
        const lfi_float2 *o = vo + (size_t)g * vo_pitch + vbase;
        const float *w = a.w32t + (size_t)g * a.v_pad + vbase;
        const __amdgpu_buffer_rsrc_t plane =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(a.grid) + (size_t)g * plane_bytes, 0, plane_bytes, 0x00020000);
#pragma unroll
        for(int j = 0; j < VIEWS; j++)
        {
            const lfi_float2 oj = o[j];
            const float wj = w[j];
            uint32_t px[VF_PX];
#pragma unroll
            for(int i = 0; i < VF_PX; i++)
            {
                const float fi = f[VIEW_MAPS ? j : 0][i];
                const int sx = clampi(warp_float(x0 + i, fi, oj.x), 0, W - 1);
                const int sy = clampi(clampi(warp_float(y, fi, oj.y), 0, H - 1) - a.in_y0, 0, a.in_rows - 1);
                px[i] = __builtin_amdgcn_raw_buffer_load_b32(plane, (sy * W + sx) * 4, 0, 0);
            }
#pragma unroll
            for(int c = 0; c < 3; c++)
#pragma unroll
                for(int i = 0; i < VF_PX; i++)
                    acc[j][c][i] = __builtin_fmaf(vf_byte(px[i], c), wj, acc[j][c][i]);
        }
    }

    if(x0 >= W)
        return;
    const bool full = x0 + VF_PX <= W;
#pragma unroll
    for(int j = 0; j < VIEWS; j++)
    {
        const int v = vbase + j;
        if(v >= a.v1) // wave-uniform
            break;
        uint32_t q[3][VF_PX];
#pragma unroll
        for(int c = 0; c < 3; c++)
#pragma unroll
            for(int i = 0; i < VF_PX; i++)
            {
                if constexpr(TEN)
                {
                    float rounded;
                    q[c][i] = quant_trunc_f16(acc[j][c][i], rounded);
                }
                else
                    q[c][i] = quant_rn(acc[j][c][i]);
            }
        if constexpr(PLANAR_OUT)
        {
            // [view][R,G,B][out_rows][views_pitch]: the pitch is a multiple of 128 ≥ W, so the 4 bytes of a lane with x0 < W stay in its row
#pragma unroll
            for(int c = 0; c < 3; c++)
            {
                uint8_t *out = a.views + ((size_t)(3 * v + c) * a.out_rows + yl) * a.views_pitch + x0;
                *reinterpret_cast<uint32_t *>(out) = q[c][0] | (q[c][1] << 8) | (q[c][2] << 16) | (q[c][3] << 24);
            }
        }
        else
        {
            uint32_t *out = reinterpret_cast<uint32_t *>(a.views) + ((size_t)v * a.out_rows + yl) * W + x0;
            uint32_t rgba[VF_PX];
#pragma unroll
            for(int i = 0; i < VF_PX; i++)
                rgba[i] = q[0][i] | (q[1][i] << 8) | (q[2][i] << 16) | 0xff000000u;
            if(full)
                *reinterpret_cast<u32x4_a4 *>(out) = u32x4{rgba[0], rgba[1], rgba[2], rgba[3]};
            else
#pragma unroll
                for(int i = 0; i < VF_PX; i++)
                    if(x0 + i < W)
                        out[i] = rgba[i];
        }
    }
}

} // namespace lfi
