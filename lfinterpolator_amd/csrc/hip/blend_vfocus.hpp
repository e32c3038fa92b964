// blend_vfocus.hpp — fixed-focus renders with one focus PER VIEW (lfi_set_view_offsets): focal stacks and focus pulls in one launch.
//
// View v samples image g at pixel + D[v][g] instead of pixel + focused_offsets[g] (reference src/interpolator.cu:226-246 computes the one
// shift per image that every other kernel here applies to all views).  The sample of (v, g) depends on v, so the contraction over images is
// no longer one matrix product with a shared pixel operand: there is no MFMA formulation, and this is a vector-pipe gather-blend.
//
//   workgroup   4 waves, one output row each, 256 pixels per wave (4 consecutive pixels per lane), VF_VIEWS views
//   accumulators VF_VIEWS views × 3 channels × 4 pixels = 96 fp32 VGPRs per lane, held for the whole image loop
//   loop        g outermost (ascending: the chain order of the reference's STD kernel, src/kernels.cu:328-338), the chunk's views inner;
//               D[v][g] and the weight are wave-uniform scalar loads ([g][view] layouts: one run of VF_VIEWS values per g)
//   sources     the derived planar copy of the inputs (3 byte planes per image, edges replicated into its padding — blend_planar.hpp):
//               a lane's 4 bytes of one channel come from one dword-aligned 8-byte load and a shift; or, where the copy cannot serve
//               the offsets (attached / handed-out grids not marked with lfi_grid_modified, shifts beyond what a copy may be padded
//               for), the RGBA planes with clamp-to-edge per pixel (surf2Dread's cudaBoundaryModeClamp, src/kernels.cu:119-126)
//   outputs     RGBA views (one 16-byte store per lane) or the planar view layout (one dword per lane and channel)
//   order       the view chunk varies fastest over the block index: the chunks of one tile run side by side and share its input rows
//
// Numerics, both methods: acc = fmaf(float(px), w32[v][g], acc) over ascending g from 0.
//   STD     the reference's Standard::process chain (src/kernels.cu:289-343) itself, then (unsigned char)__float2int_rn: bit-exact.
//   TEN_WM  pixel byte × fp16 weight is exact in fp32 (8 + 11 significant bits), so the chain is an fp32-accumulated sum of the exact
//           products — what the matrix-core kernels form, in a fixed order — rounded once to fp16 (RN-even) and truncated with saturation
//           like __half2uchar_rz (src/kernels.cu:393).  The matrix cores are not used.
#pragma once

#include "blend_std.hpp"
#include "blend_ten.hpp"

namespace lfi {

constexpr int VF_VIEWS = 8;               // views per workgroup
constexpr int VF_PX = 4;                  // pixels per lane
constexpr int VF_TILE_W = 64 * VF_PX;     // pixels per wave row
constexpr int VF_ROWS = 4;                // waves (= rows) per workgroup

__device__ __forceinline__ float vf_byte(uint32_t v, int k)
{
    return static_cast<float>((v >> (8 * k)) & 0xffu); // v_cvt_f32_ubyte{k}
}

// grid: n_chunks × tiles_x × ceil(out_rows / VF_ROWS) blocks of 256 threads.
// vo: [n_images][vo_pitch] integer offsets of views [0, vo_pitch), views contiguous; w32t: a.w32t ([k_pad][v_pad]).  Both are zero for the
// padding views, so a chunk that runs past a.v1 reads defined values; it stores views < a.v1 only.
// PLANAR_SRC: a.planar is valid and padded for every |D.x| (the dispatcher checks it against the copy's reach); rows: the dispatcher has
// checked that every sampled row is held (row windows), the clamp below only keeps a stray index inside the planes.
template <bool TEN, bool PLANAR_SRC, bool PLANAR_OUT>
__global__ void __launch_bounds__(256) blend_vfocus(const KernelArgs a, const lfi_int2 *__restrict__ vo, const int vo_pitch, const int n_chunks,
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
    const int vbase = a.v0 + chunk * VF_VIEWS;

    float acc[VF_VIEWS][3][VF_PX];
#pragma unroll
    for(int j = 0; j < VF_VIEWS; j++)
#pragma unroll
        for(int c = 0; c < 3; c++)
#pragma unroll
            for(int i = 0; i < VF_PX; i++)
                acc[j][c][i] = 0.0f;

    const size_t plane_b = (size_t)a.in_rows * a.planar_pitch; // PLANAR_SRC: bytes of one channel plane
    for(int g = 0; g < a.n_images; g++)
    {
        const lfi_int2 *d = vo + (size_t)g * vo_pitch + vbase;
        const float *w = a.w32t + (size_t)g * a.v_pad + vbase;
        int first = 0; // PLANAR_SRC: byte of pixel 0 in a row of image g
        if constexpr(PLANAR_SRC)
            first = a.planar_padx + a.planar_phase[g];
#pragma unroll
        for(int j = 0; j < VF_VIEWS; j++)
        {
            const int dx = d[j].x;
            const int sy = clampi(clampi(y + d[j].y, 0, H - 1) - a.in_y0, 0, a.in_rows - 1);
            const float wj = w[j];
            uint32_t px[3]; // PLANAR_SRC: channel c of the lane's 4 pixels; else RGBA of pixel c (and px4)
            uint32_t px4 = 0;
            if constexpr(PLANAR_SRC)
            {
                const uint8_t *row = a.planar + ((size_t)g * 3 * a.in_rows + sy) * a.planar_pitch;
                // the lane's 4 bytes start at byte b; read the dword-aligned 8 bytes that hold them, kept inside the row.  Every pixel
                // x < W lies at a byte < pitch, so where the start is pulled back to pitch − 8 the bytes shifted out of the window belong
                // to pixels past the right edge, whose results are not stored.
                const int b = x0 + dx + first;
                const int base = max(min(b & ~3, a.planar_pitch - 8), 0);
                const uint32_t sh = 8u * uint32_t(clampi(b - base, 0, 7));
#pragma unroll
                for(int c = 0; c < 3; c++)
                {
                    const u32x2 q = *reinterpret_cast<const u32x2_a4 *>(row + c * plane_b + base);
                    px[c] = uint32_t(((uint64_t(q[1]) << 32) | q[0]) >> sh);
                }
            }
            else
            {
                const uint32_t *row = reinterpret_cast<const uint32_t *>(a.grid) + ((size_t)g * a.in_rows + sy) * W;
#pragma unroll
                for(int i = 0; i < 3; i++)
                    px[i] = row[clampi(x0 + i + dx, 0, W - 1)];
                px4 = row[clampi(x0 + 3 + dx, 0, W - 1)];
            }
#pragma unroll
            for(int c = 0; c < 3; c++)
#pragma unroll
                for(int i = 0; i < VF_PX; i++)
                {
                    float s;
                    if constexpr(PLANAR_SRC)
                        s = vf_byte(px[c], i);
                    else
                        s = vf_byte(i < 3 ? px[i] : px4, c);
                    acc[j][c][i] = __builtin_fmaf(s, wj, acc[j][c][i]);
                }
        }
    }

    if(x0 >= W)
        return;
    const bool full = x0 + VF_PX <= W;
#pragma unroll
    for(int j = 0; j < VF_VIEWS; j++)
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
