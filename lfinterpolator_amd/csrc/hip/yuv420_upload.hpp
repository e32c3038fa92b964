// yuv420_upload.hpp — 8-bit YUV 4:2:0 frames expanded into the RGBA input planes: the definition's arithmetic and its coefficient tables.  The
// kernel that uses them is yuvs_expand (yuv_surfaces.hpp), behind lfi_upload_images_yuv420 and lfi_upload_images_yuv: decoded video goes in as
// it is, 1.5 bytes per pixel cross PCIe instead of the 4 of lfi_upload_image.  The mirror image of yuv420.hpp.
//
// Definition (include/lfi.h), integers only.  A frame of a W × H image is the Y plane [H][W], then Cb and Cr [ch][cw] with cw = (W + 1) >> 1,
// ch = (H + 1) >> 1, chroma centre-sited.  The chroma of pixel (x, y) in sixteenths, cx = x >> 1, cy = y >> 1:
//     NEAREST   SU = 16·U[cy][cx]
//     BILINEAR  SU = 9·U[cy][cx] + 3·U[cy][nx] + 3·U[ny][cx] + U[ny][nx],  nx = clamp(cx + ((x & 1) ? 1 : −1), 0, cw − 1), ny likewise
// and with the coefficient row (matrix, range) of YUV_IN_COEFFS, l = 16·cY·(Y − y_off), u = SU − 2048, v = SV − 2048:
//     R = clamp((l + rV·v + 2¹⁹) >> 20, 0, 255)    G = clamp((l + gU·u + gV·v + 2¹⁹) >> 20, 0, 255)    B = clamp((l + bU·u + 2¹⁹) >> 20, 0, 255)
// A = 255.  The bracket stays within ±573,111,632: int32 with an arithmetic shift, one rounding.
//
// Left siting (lfi_set_yuv_siting, include/lfi.h), BILINEAR: h(r) = 4·U[r][cx] (even x), 2·U[r][cx] + 2·U[r][min(cx + 1, cw − 1)] (odd x) and
// SU = 3·h(cy) + h(ny), again sixteenths; NEAREST is the same under either siting.  yuv_in_columns_left and yuv_in_row_left: the window
// without its left column.
//
// Here: YUV_IN_COEFFS; yuv_in_pixel and yuv_in_clamp, one RGBA dword from a luma code and chroma in sixteenths; yuv_in_bytes; yuv_in_columns
// and yuv_in_row, the bilinear filter's six-column window of a lane with the definition's clamp as byte positions; yuv_in_store, a lane's
// 8 × 2 pixels into its image, 16-byte stores where the block is whole and the rows are aligned, else dwords, none outside the image.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "yuv420.hpp"

namespace lfi {

// 16-bit fixed point: round(c · scale · 2¹⁶), scale = 255/219 (limited luma), 255/224 (limited chroma), 1 (full); with Kr, Kb of the matrix
// and Kg = 1 − Kr − Kb: rV = 2(1 − Kr), bU = 2(1 − Kb), gU = −2Kb(1 − Kb)/Kg, gV = −2Kr(1 − Kr)/Kg.  Row = matrix · 2 + range.
struct YuvInCoeffs
{
    int32_t cY, rV, gU, gV, bU, y_off;
};

constexpr YuvInCoeffs YUV_IN_COEFFS[4] = {
    {76309, 117489, -13975, -34925, 138438, 16}, // BT.709 limited
    {65536, 103206, -12276, -30679, 121609, 0},  // BT.709 full
    {76309, 104597, -25675, -53279, 132201, 16}, // BT.601 limited
    {65536, 91881, -22553, -46802, 116130, 0},   // BT.601 full
};

// clamp(floor(v / 2²⁰), 0, 255) of a bracket with its rounding term: clamped BEFORE the shift, so that the shift is a logical one of a value
// below 2²⁸.  (Written as clamp(v >> 20, 0, 255) the compiler pairs two channels into one v_ashr_pk_u8_i32 and ORs the third beside it as
// if the instruction cleared bits 16-31 of its result; on the MI355X the blue channel then came out with stray bits set.)
__device__ inline uint32_t yuv_in_clamp(const int32_t v)
{
    return (uint32_t)(v < 0 ? 0 : v > (1 << 28) - 1 ? (1 << 28) - 1 : v) >> 20;
}

// su, sv: the chroma in sixteenths; y: the luma code.  One RGBA dword
__device__ inline uint32_t yuv_in_pixel(const YuvInCoeffs &k, const int32_t y, const int32_t su, const int32_t sv)
{
    const int32_t l = 16 * k.cY * (y - k.y_off) + (1 << 19), u = su - 2048, v = sv - 2048;
    const uint32_t r = yuv_in_clamp(l + k.rV * v);
    const uint32_t g = yuv_in_clamp(l + k.gU * u + k.gV * v);
    const uint32_t b = yuv_in_clamp(l + k.bU * u);
    return r | (g << 8) | (b << 16) | 0xff000000u;
}

// the bytes of an 8-byte piece
__device__ __forceinline__ void yuv_in_bytes(const uint2 p, uint32_t (&b)[8])
{
#pragma unroll
    for(int i = 0; i < 8; i++)
        b[i] = ((i < 4 ? p.x : p.y) >> (8 * (i & 3))) & 0xffu;
}

// BILINEAR: the six chroma columns 4bx − 1 … 4bx + 4 of a lane, clamped to [0, cw − 1], as bit positions in its window of six bytes
// [column 4bx − 1 | the lane's own four | column 4bx + 4]: cw − 1 ≥ 4bx (x0 < W), so every clamped column lies in the window and a clamped
// one is a byte of the lane's own four
__device__ __forceinline__ void yuv_in_columns(const uint32_t bx, const uint32_t cw, uint32_t (&sh)[6])
{
    const int32_t c0 = 4 * (int32_t)bx - 1;
#pragma unroll
    for(int i = 0; i < 6; i++)
    {
        const int32_t c = c0 + i;
        sh[i] = 8u * (uint32_t)((c < 0 ? 0 : c > (int32_t)cw - 1 ? (int32_t)cw - 1 : c) - c0);
    }
}

// h[i] = 3·(centre column of pixel column i) + (its neighbour column) of one chroma row's window
__device__ __forceinline__ void yuv_in_row(const uint64_t win, const uint32_t (&sh)[6], int32_t (&h)[8])
{
    int32_t c[6];
#pragma unroll
    for(int i = 0; i < 6; i++)
        c[i] = (int32_t)((uint32_t)(win >> sh[i]) & 0xffu);
#pragma unroll
    for(int i = 0; i < 8; i++)
        h[i] = 3 * c[1 + (i >> 1)] + c[(i & 1) ? 2 + (i >> 1) : (i >> 1)];
}

// Left siting: the five chroma columns 4bx … 4bx + 4 of a lane, clamped to cw − 1, as bit positions in its window of five bytes [the lane's
// own four | column 4bx + 4]: a clamped column is a byte of the lane's own four (cw − 1 ≥ 4bx)
__device__ __forceinline__ void yuv_in_columns_left(const uint32_t bx, const uint32_t cw, uint32_t (&sh)[5])
{
    const uint32_t c0 = 4u * bx;
#pragma unroll
    for(int i = 0; i < 5; i++)
        sh[i] = 8u * ((c0 + i > cw - 1u ? cw - 1u : c0 + i) - c0);
}

// h[i] of pixel column i of one chroma row's window, in quarters: 4·(its own column) where i is even, else 2·(its own) + 2·(the next one)
__device__ __forceinline__ void yuv_in_row_left(const uint64_t win, const uint32_t (&sh)[5], int32_t (&h)[8])
{
    int32_t c[5];
#pragma unroll
    for(int i = 0; i < 5; i++)
        c[i] = (int32_t)((uint32_t)(win >> sh[i]) & 0xffu);
#pragma unroll
    for(int i = 0; i < 8; i++)
        h[i] = (i & 1) ? 2 * c[i >> 1] + 2 * c[(i >> 1) + 1] : 4 * c[i >> 1];
}

// a block's pixels into its image: out addresses pixel (x0, ya) of rows of W pixels.  Whole blocks of 16-byte aligned rows leave as 16-byte
// stores, ragged ones and unaligned rows pixel by pixel; two_rows: row ya + 1 exists
__device__ __forceinline__ void yuv_in_store(uint32_t *out, const uint32_t W, const uint32_t x0, const bool two_rows, const uint32_t rows16,
                                             const uint32_t (&px)[2][8])
{
    if(x0 + YUV_BLOCK_W <= W && rows16)
    {
        uint4 *row = reinterpret_cast<uint4 *>(out);
        row[0] = uint4{px[0][0], px[0][1], px[0][2], px[0][3]};
        row[1] = uint4{px[0][4], px[0][5], px[0][6], px[0][7]};
        if(two_rows)
        {
            row = reinterpret_cast<uint4 *>(out + W);
            row[0] = uint4{px[1][0], px[1][1], px[1][2], px[1][3]};
            row[1] = uint4{px[1][4], px[1][5], px[1][6], px[1][7]};
        }
    }
    else
    {
#pragma unroll
        for(int i = 0; i < 8; i++)
            if(x0 + i < W)
            {
                out[i] = px[0][i];
                if(two_rows)
                    out[W + i] = px[1][i];
            }
    }
}

} // namespace lfi
