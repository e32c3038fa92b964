// deep_yuv.hpp — 10-bit YUV 4:2:0 frames (I010, P010) from the DEEP planes (deep_blend.hpp): lfi_download_views_yuv with a format that
// carries LFI_YUV_DEEP.  Where yuvs_convert10 (yuv10.hpp) scales 8-bit codes by 876/255, these kernels convert the render's own 10-bit
// codes: the frame holds the accumulator's ten bits, no first quantisation to bytes.  The definition is in include/lfi.h.
//
// Arithmetic, integers only (DEEP_COEFFS: round(c · scale · 2¹⁶), scale 876/1023 limited luma, 896/1023 limited chroma, 1 full; G adjusted
// so that Y sums to 56120 (limited) / 65536 (full) and Cb, Cr to 0; the full rows ARE the 8-bit full rows):
//     Y10 = y_off10 + ((yR·R + yG·G + yB·B + 2¹⁵) >> 16)                       y_off10 = 64 (limited), 0 (full)
//     centre  C10 = min(1023, (2²⁷ + 2¹⁷ + uR·ΣR + uG·ΣG + uB·ΣB) >> 18)          Σ over the 2 × 2 block (≤ 4092)
//     left    C10 = min(1023, (2²⁸ + 2¹⁸ + …) >> 19)                           Σ the [1 2 1] × box sums of weight 8 (≤ 8184)
//   u32 throughout (the negative coefficients wrap, the brackets do not): the luma bracket is at most 65536·1023 + 2¹⁵ < 2²⁶; the chroma
//   brackets lie in (0, 2²⁸] (centre) and (0, 2²⁹] (left) — the upper ends are reached by full-range Cb of pure blue (32768 · 4092 + 2²⁷ + 2¹⁷
//   = 2²⁸ exactly), which the min then takes to 1023.  One rounding.
//
// Decomposition, alignment contract and stores are yuvs_convert10's (yuv10.hpp): a lane owns 8 columns × 2 rows, a wave 64 neighbouring
// blocks of ONE block row, a workgroup four block rows, the view is grid.z; no LDS, no atomics, no scratch.  A lane's row of a deep plane is
// ONE 16-byte load at 16·bx: deep_pitch is 2·W rounded up to 128, so 16·bx + 16 ≤ 2·round8(W) ≤ deep_pitch; columns beyond W (the planes'
// padding holds whatever the blend's last lanes wrote) are replaced by the last column's, an odd last row by the row above: the
// definition's clamp.  The codes are taken & 1023.
//   deep_convert10<FORMAT>        centre siting
//   deep_convert10_left<FORMAT>   the left neighbour lane's column 7 crosses with DPP moves (wave_shr:1) as in yuvs_convert10_left — TWO of
//     them: the three two-row sums of 10-bit codes are 11 bits each, 33 bits in all, one more than a dword holds.  Lane 0 of a wave with
//     bx > 0 loads pixel column x0 − 1 itself; bx = 0 clamps to its own column 0.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "yuv10.hpp"

namespace lfi {

constexpr YuvCoeffs DEEP_COEFFS[4] = {
    {{11931, 40137, 4052}, {-6576, -22124, 28700}, {28700, -26068, -2632}, 64},  // BT.709 limited
    {{13933, 46871, 4732}, {-7509, -25259, 32768}, {32768, -29763, -3005}, 0},   // BT.709 full
    {{16780, 32942, 6398}, {-9685, -19015, 28700}, {28700, -24033, -4667}, 64},  // BT.601 limited
    {{19595, 38470, 7471}, {-11058, -21710, 32768}, {32768, -27439, -5329}, 0},  // BT.601 full
};

struct DeepOutArgs
{
    const uint8_t *deep; // the R plane of the first view: [view][3: R,G,B][H][pitch] bytes, u16 codes
    size_t view_stride;  // bytes from view to view: 3·H·pitch
    uint32_t pitch;      // bytes per plane row
    uint32_t W, H;
    YuvSurfaces s;       // written
    uint32_t cw, ch;
    uint32_t blocks_x;   // (W + 7) / 8
    YuvCoeffs k;         // DEEP_COEFFS[matrix · 2 + range]
};

__device__ inline uint32_t deep_luma(const YuvCoeffs &k, const uint32_t r, const uint32_t g, const uint32_t b)
{
    return k.y_off + (((uint32_t)k.y[0] * r + (uint32_t)k.y[1] * g + (uint32_t)k.y[2] * b + 0x8000u) >> 16);
}

template <bool LEFT>
__device__ inline uint32_t deep_chroma(const int32_t (&c)[3], const uint32_t sr, const uint32_t sg, const uint32_t sb)
{
    constexpr int S = LEFT ? 1 : 0;
    const uint32_t v = ((1u << (27 + S)) + (1u << (17 + S)) + (uint32_t)c[0] * sr + (uint32_t)c[1] * sg + (uint32_t)c[2] * sb) >> (18 + S);
    return v < 1023u ? v : 1023u;
}

// the eight codes of a lane's row of a plane; columns beyond `last` (the view's last column inside the block, 0 … 7) take column last's
__device__ __forceinline__ void deep_load_row(const uint8_t *row, const uint32_t bx, const uint32_t last, uint32_t (&v)[8])
{
    yuv10_words(*reinterpret_cast<const uint4 *>(row + 16u * bx), v);
#pragma unroll
    for(int i = 0; i < 8; i++)
        v[i] &= 1023u;
#pragma unroll
    for(int i = 1; i < 8; i++)
        v[i] = (uint32_t)i > last ? v[i - 1] : v[i];
}

template <int FORMAT, bool LEFT>
__device__ __forceinline__ void deep_convert10_block(const DeepOutArgs &a)
{
    const uint32_t bx = blockIdx.x * YUV_LANES_X + threadIdx.x;
    const uint32_t by = blockIdx.y * YUV_BLOCK_ROWS + threadIdx.y; // wave-uniform
    if(bx >= a.blocks_x || by >= a.ch)
        return;
    const uint32_t x0 = bx * YUV_BLOCK_W;
    const bool two_rows = by * YUV_BLOCK_H + 1u < a.H;
    const uint32_t ya = by * YUV_BLOCK_H, yb = two_rows ? ya + 1u : ya; // ya < H: by < ch
    const bool whole = x0 + YUV_BLOCK_W <= a.W;                         // all 8 columns inside the view
    const uint32_t last = whole ? 7u : a.W - 1u - x0;
    const uint8_t *view = a.deep + (size_t)blockIdx.z * a.view_stride;
    const size_t plane = (size_t)a.H * a.pitch;
    // LEFT: lane 0 of a wave loads pixel column x0 − 1 itself (bx > 0: inside the view), ahead of the block's own loads
    [[maybe_unused]] uint32_t edge[3] = {0u, 0u, 0u};
    if constexpr(LEFT)
        if(threadIdx.x == 0 && bx)
        {
#pragma unroll
            for(int ch = 0; ch < 3; ch++)
                edge[ch] = (uint32_t)(*reinterpret_cast<const uint16_t *>(view + ch * plane + (size_t)ya * a.pitch + 2u * (x0 - 1u)) & 1023u) +
                           (uint32_t)(*reinterpret_cast<const uint16_t *>(view + ch * plane + (size_t)yb * a.pitch + 2u * (x0 - 1u)) & 1023u);
        }
    uint32_t r[2][8], g[2][8], b[2][8];
    deep_load_row(view + (size_t)ya * a.pitch, bx, last, r[0]);
    deep_load_row(view + (size_t)yb * a.pitch, bx, last, r[1]);
    deep_load_row(view + plane + (size_t)ya * a.pitch, bx, last, g[0]);
    deep_load_row(view + plane + (size_t)yb * a.pitch, bx, last, g[1]);
    deep_load_row(view + 2 * plane + (size_t)ya * a.pitch, bx, last, b[0]);
    deep_load_row(view + 2 * plane + (size_t)yb * a.pitch, bx, last, b[1]);
    uint8_t *frame = a.s.base + (size_t)blockIdx.z * a.s.frame_stride;
    // Y: the row's own samples only, and no row beyond H (the stores are yuvs_convert10's)
#pragma unroll
    for(int j = 0; j < 2; j++)
    {
        uint32_t y[8];
#pragma unroll
        for(int i = 0; i < 8; i++)
            y[i] = yuv10_word<FORMAT>(deep_luma(a.k, r[j][i], g[j][i], b[j][i]));
        uint8_t *row = frame + (size_t)(ya + j) * a.s.y_pitch + 16u * bx;
        if(j && !two_rows)
            continue;
        if(whole)
            *reinterpret_cast<uint4 *>(row) = uint4{y[0] | (y[1] << 16), y[2] | (y[3] << 16), y[4] | (y[5] << 16), y[6] | (y[7] << 16)};
        else
        {
#pragma unroll
            for(int i = 0; i < 7; i++) // a ragged block holds at most 7 columns
                if(x0 + i < a.W)
                    reinterpret_cast<uint16_t *>(row)[i] = (uint16_t)y[i];
        }
    }
    // v(k): the two-row sums of block column k; v(−1) from the left neighbour lane (LEFT)
    [[maybe_unused]] uint32_t lr = 0u, lg = 0u, lb = 0u;
    if constexpr(LEFT)
    {
        // behind the early return: a source lane bx − 1 < bx is always on and always a whole block; lane 0 of a wave keeps `old` and takes
        // the column it loaded above, or its own column 0 (bx = 0)
        const uint32_t rg = (r[0][7] + r[1][7]) | ((g[0][7] + g[1][7]) << 16), bb = b[0][7] + b[1][7];
        const uint32_t nrg = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)rg, 0x138, 0xf, 0xf, false);
        const uint32_t nb = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)bb, 0x138, 0xf, 0xf, false);
        lr = nrg & 0xffffu, lg = nrg >> 16, lb = nb;
        if(threadIdx.x == 0)
        {
            lr = bx ? edge[0] : r[0][0] + r[1][0];
            lg = bx ? edge[1] : g[0][0] + g[1][0];
            lb = bx ? edge[2] : b[0][0] + b[1][0];
        }
    }
    uint32_t cb[4], cr[4];
#pragma unroll
    for(int i = 0; i < 4; i++)
    {
        const int c = 2 * i, n = 2 * i + 1;
        uint32_t sr = r[0][c] + r[1][c], sg = g[0][c] + g[1][c], sb = b[0][c] + b[1][c];
        if constexpr(LEFT)
        {
            const uint32_t pr = i ? r[0][c - 1] + r[1][c - 1] : lr, pg = i ? g[0][c - 1] + g[1][c - 1] : lg, pb = i ? b[0][c - 1] + b[1][c - 1] : lb;
            sr = pr + 2u * sr, sg = pg + 2u * sg, sb = pb + 2u * sb;
        }
        sr += r[0][n] + r[1][n], sg += g[0][n] + g[1][n], sb += b[0][n] + b[1][n];
        cb[i] = yuv10_word<FORMAT>(deep_chroma<LEFT>(a.k.cb, sr, sg, sb));
        cr[i] = yuv10_word<FORMAT>(deep_chroma<LEFT>(a.k.cr, sr, sg, sb));
    }
    const uint32_t c0 = 4u * bx; // < cw: x0 < W
    const bool c_whole = c0 + 4u <= a.cw;
    if constexpr(FORMAT == YUVS_NV12)
    {
        uint8_t *row = frame + a.s.c_offset + (size_t)by * a.s.c_pitch + 16u * bx;
        if(c_whole)
            *reinterpret_cast<uint4 *>(row) = uint4{cb[0] | (cr[0] << 16), cb[1] | (cr[1] << 16), cb[2] | (cr[2] << 16), cb[3] | (cr[3] << 16)};
        else
        {
#pragma unroll
            for(int i = 0; i < 3; i++)
                if(c0 + i < a.cw)
                    reinterpret_cast<uint16_t *>(row)[2 * i] = (uint16_t)cb[i], reinterpret_cast<uint16_t *>(row)[2 * i + 1] = (uint16_t)cr[i];
        }
    }
    else
    {
        uint8_t *u_row = frame + a.s.c_offset + (size_t)by * a.s.c_pitch + 8u * bx, *v_row = frame + a.s.cr_offset + (size_t)by * a.s.c_pitch + 8u * bx;
        if(c_whole)
        {
            *reinterpret_cast<uint2 *>(u_row) = uint2{cb[0] | (cb[1] << 16), cb[2] | (cb[3] << 16)};
            *reinterpret_cast<uint2 *>(v_row) = uint2{cr[0] | (cr[1] << 16), cr[2] | (cr[3] << 16)};
        }
        else
        {
#pragma unroll
            for(int i = 0; i < 3; i++)
                if(c0 + i < a.cw)
                    reinterpret_cast<uint16_t *>(u_row)[i] = (uint16_t)cb[i], reinterpret_cast<uint16_t *>(v_row)[i] = (uint16_t)cr[i];
        }
    }
}

template <int FORMAT>
__global__ void __launch_bounds__(YUV_LANES_X *YUV_BLOCK_ROWS) deep_convert10(const DeepOutArgs a)
{
    deep_convert10_block<FORMAT, false>(a);
}

// left-sited chroma
template <int FORMAT>
__global__ void __launch_bounds__(YUV_LANES_X *YUV_BLOCK_ROWS) deep_convert10_left(const DeepOutArgs a)
{
    deep_convert10_block<FORMAT, true>(a);
}

// Enqueues the ONE deep_convert10 launch for n views; layout: YUVS_I420 (I010) or YUVS_NV12 (P010)
inline hipError_t launch_deep_convert10(hipStream_t stream, const int layout, const bool left, const DeepOutArgs &a, const int n)
{
    const dim3 grid = yuvs_grid(a.blocks_x, a.ch, n), block(YUV_LANES_X, YUV_BLOCK_ROWS);
    if(left)
    {
        if(layout == YUVS_NV12)
            hipLaunchKernelGGL((deep_convert10_left<YUVS_NV12>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((deep_convert10_left<YUVS_I420>), grid, block, 0, stream, a);
    }
    else if(layout == YUVS_NV12)
        hipLaunchKernelGGL((deep_convert10<YUVS_NV12>), grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL((deep_convert10<YUVS_I420>), grid, block, 0, stream, a);
    return hipGetLastError();
}

} // namespace lfi
