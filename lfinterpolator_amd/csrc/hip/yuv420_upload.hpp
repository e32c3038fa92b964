// yuv420_upload.hpp — 8-bit YUV 4:2:0 frames (I420) expanded into the RGBA input planes on the device (lfi_upload_images_yuv420): decoded
// video goes in as it is, 1.5 bytes per pixel cross PCIe instead of the 4 of lfi_upload_image.  The mirror image of yuv420.hpp.
//
// Definition (include/lfi.h), integers only.  A frame of a W × H image is the Y plane [H][W], then Cb and Cr [ch][cw] with cw = (W + 1) >> 1,
// ch = (H + 1) >> 1, chroma centre-sited.  The chroma of pixel (x, y) in sixteenths, cx = x >> 1, cy = y >> 1:
//     NEAREST   SU = 16·U[cy][cx]
//     BILINEAR  SU = 9·U[cy][cx] + 3·U[cy][nx] + 3·U[ny][cx] + U[ny][nx],  nx = clamp(cx + ((x & 1) ? 1 : −1), 0, cw − 1), ny likewise
// and with the coefficient row (matrix, range) of YUV_IN_COEFFS, l = 16·cY·(Y − y_off), u = SU − 2048, v = SV − 2048:
//     R = clamp((l + rV·v + 2¹⁹) >> 20, 0, 255)    G = clamp((l + gU·u + gV·v + 2¹⁹) >> 20, 0, 255)    B = clamp((l + bU·u + 2¹⁹) >> 20, 0, 255)
// A = 255.  The bracket stays within ±573,111,632: int32 with an arithmetic shift, one rounding.
//
//   yuv420_expand<NEAREST>  one launch per chunk of frames (the frame is grid.z).  A lane owns a block of 8 columns × 2 rows of one image: it
//     reads two 8-byte pieces of Y and, per chroma plane, the dword at 4·bx (its four chroma columns) of chroma row by — BILINEAR: also of
//     rows by − 1 and by + 1 (clamped) and in each of them the dwords left and right of it, of which it uses one byte each — and writes two
//     runs of 32 bytes as 16-byte stores.  A wave is 64 neighbouring blocks of ONE block row: its Y loads are two runs of 512 bytes, its
//     chroma loads runs of 256 bytes that neighbouring lanes share (the repeats hit in cache), its stores two runs of 2 KiB; the row's
//     offsets are wave-uniform.  A workgroup is four waves = four block rows.
//     The frames lie in the padded staging planes of yuv_geometry (Y pitch a multiple of 8, chroma pitch of 4, an even number of Y rows):
//     every load is whole and inside its own row.  The host copies only the frames' own bytes there, so NO value the kernel uses may come
//     from padding: the chroma neighbours are clamped to [0, cw − 1] × [0, ch − 1] as the definition says (a clamped neighbour is a byte
//     of the lane's own dword or row), and the Y bytes beyond the image belong to pixels that are not stored.
//     Ragged blocks, an odd last row, and images whose rows are not 16-byte aligned (W no multiple of 4) store pixel by pixel as dwords;
//     no lane stores outside the image.  No LDS, no atomics, no byte stores, no scratch.
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

struct YuvInArgs
{
    const uint8_t *src;  // staged frame 0 of the chunk: [frame][Y: y_rows × y_pitch | Cb: ch × c_pitch | Cr: ch × c_pitch]
    uint8_t *dst;        // RGBA plane [H][W] of the chunk's first image
    size_t frame_stride; // bytes from staged frame to staged frame
    size_t image_stride; // bytes from image to image
    uint32_t W, H, cw, ch;
    uint32_t y_pitch, c_pitch;
    uint32_t blocks_x; // y_pitch / 8
    uint32_t rows16;   // every pixel row of an image starts on a 16-byte boundary (W a multiple of 4)
    YuvInCoeffs k;
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

template <bool NEAREST>
__global__ void __launch_bounds__(YUV_LANES_X *YUV_BLOCK_ROWS) yuv420_expand(const YuvInArgs a)
{
    const uint32_t bx = blockIdx.x * YUV_LANES_X + threadIdx.x;
    const uint32_t by = blockIdx.y * YUV_BLOCK_ROWS + threadIdx.y; // wave-uniform
    if(bx >= a.blocks_x || by >= a.ch)
        return;
    const uint32_t x0 = bx * YUV_BLOCK_W, ya = by * YUV_BLOCK_H; // x0 < W (x0 < y_pitch < W + 8), ya < H (by < ch)
    const uint8_t *frame = a.src + (size_t)blockIdx.z * a.frame_stride;
    const uint8_t *cb_plane = frame + (size_t)a.y_pitch * (2u * a.ch), *cr_plane = cb_plane + (size_t)a.c_pitch * a.ch;
    // Y: rows ya and ya + 1 < y_rows = 2·ch, columns x0 … x0 + 7 < y_pitch
    uint32_t y[2][8];
#pragma unroll
    for(int j = 0; j < 2; j++)
        yuv_in_bytes(*reinterpret_cast<const uint2 *>(frame + (size_t)(ya + j) * a.y_pitch + x0), y[j]);
    // chroma in sixteenths of the 16 pixels
    int32_t su[2][8], sv[2][8];
    if constexpr(NEAREST)
    {
        const uint32_t u = *reinterpret_cast<const uint32_t *>(cb_plane + (size_t)by * a.c_pitch + 4u * bx);
        const uint32_t v = *reinterpret_cast<const uint32_t *>(cr_plane + (size_t)by * a.c_pitch + 4u * bx);
#pragma unroll
        for(int i = 0; i < 8; i++)
            su[0][i] = su[1][i] = 16 * (int32_t)((u >> (8 * (i >> 1))) & 0xffu), sv[0][i] = sv[1][i] = 16 * (int32_t)((v >> (8 * (i >> 1))) & 0xffu);
    }
    else
    {
        uint32_t sh[6];
        yuv_in_columns(bx, a.cw, sh);
        const bool has_l = bx > 0, has_r = bx + 1u < a.blocks_x;
        // rows by − 1, by, by + 1, clamped to [0, ch − 1]
        const uint32_t rows[3] = {by > 0 ? by - 1u : 0u, by, by + 1u < a.ch ? by + 1u : a.ch - 1u};
        // h[r][i] = 3·(centre column of pixel column i) + (its neighbour column) on row r
        int32_t hu[3][8], hv[3][8];
#pragma unroll
        for(int r = 0; r < 3; r++)
        {
#pragma unroll
            for(int p = 0; p < 2; p++)
            {
                const uint32_t *row = reinterpret_cast<const uint32_t *>((p ? cr_plane : cb_plane) + (size_t)rows[r] * a.c_pitch) + bx;
                const uint32_t own = row[0], left = has_l ? row[-1] : 0u, right = has_r ? row[1] : 0u;
                const uint64_t win = (uint64_t)(left >> 24) | ((uint64_t)own << 8) | ((uint64_t)(right & 0xffu) << 40);
                yuv_in_row(win, sh, p ? hv[r] : hu[r]);
            }
        }
        // 9·a + 3·b + 3·c + d = 3·(3a + b) + (3c + d): an even row's neighbour row is the one above, an odd row's the one below
#pragma unroll
        for(int j = 0; j < 2; j++)
#pragma unroll
            for(int i = 0; i < 8; i++)
                su[j][i] = 3 * hu[1][i] + hu[j ? 2 : 0][i], sv[j][i] = 3 * hv[1][i] + hv[j ? 2 : 0][i];
    }
    uint32_t px[2][8];
#pragma unroll
    for(int j = 0; j < 2; j++)
#pragma unroll
        for(int i = 0; i < 8; i++)
            px[j][i] = yuv_in_pixel(a.k, (int32_t)y[j][i], su[j][i], sv[j][i]);
    uint32_t *out = reinterpret_cast<uint32_t *>(a.dst + (size_t)blockIdx.z * a.image_stride) + (size_t)ya * a.W + x0;
    const bool two_rows = ya + 1u < a.H; // an odd H's last block row has one pixel row
    yuv_in_store(out, a.W, x0, two_rows, a.rows16, px);
}

// Enqueues the ONE yuv420_expand launch for n staged frames.  The caller has checked the sizes: n ≥ 1, a.src holds n staged frames, a.dst n images.
inline hipError_t launch_yuv420_expand(hipStream_t stream, const bool nearest, const YuvInArgs &a, const int n)
{
    const dim3 grid((a.blocks_x + YUV_LANES_X - 1) / YUV_LANES_X, (a.ch + YUV_BLOCK_ROWS - 1) / YUV_BLOCK_ROWS, n), block(YUV_LANES_X, YUV_BLOCK_ROWS);
    if(nearest)
        hipLaunchKernelGGL(yuv420_expand<true>, grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL(yuv420_expand<false>, grid, block, 0, stream, a);
    return hipGetLastError();
}

} // namespace lfi
