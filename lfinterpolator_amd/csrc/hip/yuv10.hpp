// yuv10.hpp — the 10-bit YUV 4:2:0 kernels: I010 (planar, the code in bits 9..0 of a little-endian u16: yuv420p10le, Y4M's C420p10) and P010
// (semi-planar, the code in bits 15..6: p010le) surfaces in and out, behind lfi_upload_images_yuv, lfi_download_views_yuv and
// lfi_download_quilt_yuv when the descriptor's format carries LFI_YUV_10BIT.  The definition is in include/lfi.h; the geometry is that of
// yuv_surfaces.hpp with two bytes per sample (pitches, offsets and strides stay in bytes), the decomposition is the same (a lane owns
// 8 columns × 2 rows, a wave 64 neighbouring blocks of ONE block row, a workgroup four block rows, the frame or view is grid.z; no LDS, no
// atomics, no scratch), and so are the rules about what is read and what is stored.  Kernels of their own names — tests pin the number of
// yuvs_expand and yuvs_convert bodies —, which share with the 8-bit ones what does not depend on the depth: loading the views
// (yuv_load_block, yuv_load_column), the packed column sums and the one DPP move of the left-sited exchange, the store of a block's RGBA
// pixels (yuv_in_store), the final clamp (yuv_in_clamp), the launch grid.
//
// Arithmetic, integers only.
//   views → frames (YUV10_COEFFS, 14 fractional bits: round(c · scale · 2¹⁴), scale 876/255 limited luma, 896/255 limited chroma, 1023/255
//   full; the limited rows ARE the 8-bit rows: 876/255 · 2¹⁴ = 219/255 · 2¹⁶):
//     Y10 = y_off10 + ((yR·R + yG·G + yB·B + 2¹³) >> 14)                  y_off10 = 64 (limited), 0 (full)
//     centre  C10 = min(1023, (2²⁵ + 2¹⁵ + uR·ΣR + uG·ΣG + uB·ΣB) >> 16)     Σ over the 2 × 2 block
//     left    C10 = min(1023, (2²⁶ + 2¹⁶ + …) >> 17)                      Σ the [1 2 1] × box sums of weight 8
//   u32 throughout (the negative coefficients wrap, the brackets — below 2²⁷ and at most 2²⁸ as in the 8-bit definition, the coefficients
//   being of the same size — do not), one rounding.
//   frames → images (YUV10_IN_COEFFS, round(c · scale · 2¹⁶), scale 255/876, 255/896, 255/1023): chroma in sixteenths exactly as in
//   yuv420_upload.hpp, of 10-bit codes (SU ≤ 16368),
//     l = 16·cY·(Y10 − y_off),  u = SU − 8192,  v = SV − 8192,  R = clamp((l + rV·v + 2¹⁹) >> 20, 0, 255), G and B likewise, A = 255.
//   The bracket with its rounding term stays within ±576,213,136 over all 10-bit code triples (709 limited, blue, Y = 1023, U = 1023): int32.
//
// What the launches rely on (the entry points see to it): the Y plane's base and the frame stride are multiples of 16 and so is y_pitch;
// I010: the chroma planes' bases and c_pitch are multiples of 8; P010: the chroma plane's base and c_pitch are multiples of 16 — in-place
// surfaces have multiples of 16 throughout, the staged planes are those of yuv_geometry with two bytes per sample (y_pitch 2·round8(W);
// I010 chroma rows of y_pitch / 2 bytes, P010 of y_pitch).  Every pitch is at least its format's minimum (2W; 2cw, 4cw).  Then every load
// and every word store is aligned and lies inside its own row:
//   Y      16 bytes at 16·bx:   16·bx + 16 ≤ 2·round8(W) ≤ y_pitch
//   I010   8 bytes at 8·bx:     8·bx + 8 ≤ round8(2·cw) ≤ c_pitch
//   P010   16 bytes at 16·bx:   16·bx + 16 ≤ round16(4·cw) ≤ c_pitch
// and rows are clamped to the plane's own.  The bilinear filter's two columns from outside a lane's four are read as SAMPLES, only where they
// exist: column 4bx − 1 where bx > 0 (I010 the u16 at 8·bx − 2, P010 the pair at 16·bx − 4), column 4bx + 4 only where bx + 1 < blocks_x
// (then 4bx + 4 ≤ cw − 1: I010 the u16 at 8·bx + 8, P010 the pair at 16·bx + 16).  No value comes from padding or from outside the plane.
//
//   yuvs_expand10<FORMAT, NEAREST>      frames → RGBA images.  The six columns of a lane's window go, as 10-bit codes, into one u64 of ten
//     bits apiece, and the definition's clamp is a set of bit positions computed once (yuv_in_columns with 10 for 8).  P010's low six bits
//     and I010's upper six are dropped when the codes are taken.
//   yuvs_expand10_left<FORMAT>          left-sited BILINEAR (NEAREST is yuvs_expand10<FORMAT, true> under either siting): the window
//     without its left column.
//   yuvs_convert10<PLANAR, FORMAT>      views → frames.  A whole block stores words — a Y row one 16-byte piece, four P010 pairs one 16-byte
//     piece, four I010 samples per plane one 8-byte piece —, a ragged last block of a row stores its valid samples one u16 at a time, a row
//     beyond H is not stored; unused bits are written as 0; pitch padding keeps its value.
//   yuvs_convert10_left<PLANAR, FORMAT> the left neighbour lane's column 7 crosses with ONE DPP move, as in yuvs_convert_left.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "yuv_surfaces.hpp"

namespace lfi {

// 14 fractional bits; G adjusted so that Y sums to 56284 (limited: 876/255 · 2¹⁴) / 65729 (full: round(1023/255 · 2¹⁴)) and Cb, Cr to 0
constexpr YuvCoeffs YUV10_COEFFS[4] = {
    {{11966, 40254, 4064}, {-6596, -22188, 28784}, {28784, -26145, -2639}, 64},  // BT.709 limited
    {{13974, 47009, 4746}, {-7531, -25333, 32864}, {32864, -29851, -3013}, 0},   // BT.709 full
    {{16829, 33039, 6416}, {-9714, -19070, 28784}, {28784, -24103, -4681}, 64},  // BT.601 limited
    {{19653, 38583, 7493}, {-11091, -21773, 32864}, {32864, -27519, -5345}, 0},  // BT.601 full
};

constexpr YuvInCoeffs YUV10_IN_COEFFS[4] = {
    {19077, 29372, -3494, -8731, 34610, 64}, // BT.709 limited
    {16336, 25726, -3060, -7647, 30313, 0},  // BT.709 full
    {19077, 26149, -6419, -13320, 33050, 64}, // BT.601 limited
    {16336, 22903, -5622, -11666, 28947, 0},  // BT.601 full
};

// the word of a 10-bit code and the code of a word: I010 bits 9..0, P010 bits 15..6; the other six bits are written 0 and ignored
template <int FORMAT>
__device__ __forceinline__ uint32_t yuv10_word(const uint32_t code)
{
    return FORMAT == YUVS_NV12 ? code << 6 : code;
}

template <int FORMAT>
__device__ __forceinline__ uint32_t yuv10_code(const uint32_t word16)
{
    return FORMAT == YUVS_NV12 ? (word16 & 0xffffu) >> 6 : word16 & 1023u;
}

__device__ inline uint32_t yuv10_luma(const YuvCoeffs &k, const uint32_t r, const uint32_t g, const uint32_t b)
{
    return k.y_off + (((uint32_t)k.y[0] * r + (uint32_t)k.y[1] * g + (uint32_t)k.y[2] * b + 0x2000u) >> 14);
}

template <bool LEFT>
__device__ inline uint32_t yuv10_chroma(const int32_t (&c)[3], const uint32_t sr, const uint32_t sg, const uint32_t sb)
{
    constexpr int S = LEFT ? 1 : 0;
    const uint32_t v = ((1u << (25 + S)) + (1u << (15 + S)) + (uint32_t)c[0] * sr + (uint32_t)c[1] * sg + (uint32_t)c[2] * sb) >> (16 + S);
    return v < 1023u ? v : 1023u;
}

// Cb and Cr of the block's chroma column i.  left (LEFT only): v(−1) as yuv_pack_sums packs it
template <bool LEFT>
__device__ __forceinline__ void yuv10_block_chroma(const YuvCoeffs &k, const uint32_t (&r)[2][8], const uint32_t (&g)[2][8], const uint32_t (&b)[2][8],
                                                   const uint32_t left, const int i, uint32_t &cb, uint32_t &cr)
{
    const int c = 2 * i, n = 2 * i + 1;
    uint32_t sr = r[0][c] + r[1][c], sg = g[0][c] + g[1][c], sb = b[0][c] + b[1][c];
    if constexpr(LEFT)
    {
        uint32_t lr, lg, lb;
        if(i == 0)
            lr = left & 0x3ffu, lg = (left >> 10) & 0x3ffu, lb = left >> 20;
        else
            lr = r[0][c - 1] + r[1][c - 1], lg = g[0][c - 1] + g[1][c - 1], lb = b[0][c - 1] + b[1][c - 1];
        sr = lr + 2u * sr, sg = lg + 2u * sg, sb = lb + 2u * sb;
    }
    sr += r[0][n] + r[1][n], sg += g[0][n] + g[1][n], sb += b[0][n] + b[1][n];
    cb = yuv10_chroma<LEFT>(k.cb, sr, sg, sb);
    cr = yuv10_chroma<LEFT>(k.cr, sr, sg, sb);
}

// su, sv: the chroma in sixteenths of 10-bit codes; y: the luma code.  One RGBA dword
__device__ inline uint32_t yuv10_in_pixel(const YuvInCoeffs &k, const int32_t y, const int32_t su, const int32_t sv)
{
    const int32_t l = 16 * k.cY * (y - k.y_off) + (1 << 19), u = su - 8192, v = sv - 8192;
    const uint32_t r = yuv_in_clamp(l + k.rV * v);
    const uint32_t g = yuv_in_clamp(l + k.gU * u + k.gV * v);
    const uint32_t b = yuv_in_clamp(l + k.bU * u);
    return r | (g << 8) | (b << 16) | 0xff000000u;
}

// the eight 16-bit words of a 16-byte piece
__device__ __forceinline__ void yuv10_words(const uint4 p, uint32_t (&w)[8])
{
    w[0] = p.x & 0xffffu, w[1] = p.x >> 16, w[2] = p.y & 0xffffu, w[3] = p.y >> 16;
    w[4] = p.z & 0xffffu, w[5] = p.z >> 16, w[6] = p.w & 0xffffu, w[7] = p.w >> 16;
}

// The bilinear window of a lane as bit positions, ten bits a column: N = 6 [column 4bx − 1 | own four | column 4bx + 4] (centre), N = 5 [own
// four | column 4bx + 4] (left siting); every column clamped to [0, cw − 1] — cw − 1 ≥ 4bx, so a clamped one is one of the lane's own four
template <int N>
__device__ __forceinline__ void yuv10_in_columns(const uint32_t bx, const uint32_t cw, uint32_t (&sh)[N])
{
    const int32_t c0 = 4 * (int32_t)bx - (N == 6 ? 1 : 0);
#pragma unroll
    for(int i = 0; i < N; i++)
    {
        const int32_t c = c0 + i;
        sh[i] = 10u * (uint32_t)((c < 0 ? 0 : c > (int32_t)cw - 1 ? (int32_t)cw - 1 : c) - c0);
    }
}

// h[i] of pixel column i of one chroma row's window: centre 3·(its column) + (its neighbour), left siting quarters as in yuv_in_row_left
template <int N>
__device__ __forceinline__ void yuv10_in_row(const uint64_t win, const uint32_t (&sh)[N], int32_t (&h)[8])
{
    int32_t c[N];
#pragma unroll
    for(int i = 0; i < N; i++)
        c[i] = (int32_t)((uint32_t)(win >> sh[i]) & 1023u);
#pragma unroll
    for(int i = 0; i < 8; i++)
    {
        if constexpr(N == 6)
            h[i] = 3 * c[1 + (i >> 1)] + c[(i & 1) ? 2 + (i >> 1) : (i >> 1)];
        else
            h[i] = (i & 1) ? 2 * c[i >> 1] + 2 * c[(i >> 1) + 1] : 4 * c[i >> 1];
    }
}

// The codes of a lane's own four chroma columns of chroma row `row` (a row of the Cb or CbCr plane; v_row: the same row of I010's Cr plane)
template <int FORMAT>
__device__ __forceinline__ void yuv10_own_chroma(const uint8_t *row, const uint8_t *v_row, const uint32_t bx, uint32_t (&u)[4], uint32_t (&v)[4])
{
    if constexpr(FORMAT == YUVS_NV12)
    {
        uint32_t w[8];
        yuv10_words(*reinterpret_cast<const uint4 *>(row + 16u * bx), w);
#pragma unroll
        for(int i = 0; i < 4; i++)
            u[i] = w[2 * i] >> 6, v[i] = w[2 * i + 1] >> 6;
    }
    else
    {
        const uint2 pu = *reinterpret_cast<const uint2 *>(row + 8u * bx), pv = *reinterpret_cast<const uint2 *>(v_row + 8u * bx);
        u[0] = pu.x & 1023u, u[1] = (pu.x >> 16) & 1023u, u[2] = pu.y & 1023u, u[3] = (pu.y >> 16) & 1023u;
        v[0] = pv.x & 1023u, v[1] = (pv.x >> 16) & 1023u, v[2] = pv.y & 1023u, v[3] = (pv.y >> 16) & 1023u;
    }
}

// chroma column c (it exists: 0 ≤ c < cw) of a chroma row, as codes
template <int FORMAT>
__device__ __forceinline__ void yuv10_chroma_sample(const uint8_t *row, const uint8_t *v_row, const uint32_t c, uint32_t &u, uint32_t &v)
{
    if constexpr(FORMAT == YUVS_NV12)
    {
        const uint32_t p = *reinterpret_cast<const uint32_t *>(row + 4u * c);
        u = (p & 0xffffu) >> 6, v = p >> 22;
    }
    else
        u = *reinterpret_cast<const uint16_t *>(row + 2u * c) & 1023u, v = *reinterpret_cast<const uint16_t *>(v_row + 2u * c) & 1023u;
}

template <int FORMAT, bool NEAREST, bool LEFT>
__device__ __forceinline__ void yuvs_expand10_block(const YuvsInArgs &a)
{
    const uint32_t bx = blockIdx.x * YUV_LANES_X + threadIdx.x;
    const uint32_t by = blockIdx.y * YUV_BLOCK_ROWS + threadIdx.y; // wave-uniform
    if(bx >= a.blocks_x || by >= a.ch)
        return;
    const uint32_t x0 = bx * YUV_BLOCK_W, ya = by * YUV_BLOCK_H; // x0 < W, ya < H
    const bool two_rows = ya + 1u < a.H;                         // an odd H's last block row has one pixel row
    const uint8_t *frame = a.s.base + (size_t)blockIdx.z * a.s.frame_stride;
    const uint8_t *u_plane = frame + a.s.c_offset, *v_plane = frame + a.s.cr_offset; // P010: the CbCr plane, v_plane unused
    // Y: row ya and row ya + 1 (clamped to the plane: its pixels are not stored then), columns x0 … x0 + 7
    uint32_t y[2][8];
    yuv10_words(*reinterpret_cast<const uint4 *>(frame + (size_t)ya * a.s.y_pitch + 16u * bx), y[0]);
    yuv10_words(*reinterpret_cast<const uint4 *>(frame + (size_t)(two_rows ? ya + 1u : ya) * a.s.y_pitch + 16u * bx), y[1]);
    // chroma in sixteenths of the 16 pixels
    int32_t su[2][8], sv[2][8];
    if constexpr(NEAREST)
    {
        uint32_t u[4], v[4];
        yuv10_own_chroma<FORMAT>(u_plane + (size_t)by * a.s.c_pitch, v_plane + (size_t)by * a.s.c_pitch, bx, u, v);
#pragma unroll
        for(int i = 0; i < 8; i++)
            su[0][i] = su[1][i] = 16 * (int32_t)u[i >> 1], sv[0][i] = sv[1][i] = 16 * (int32_t)v[i >> 1];
    }
    else
    {
        constexpr int N = LEFT ? 5 : 6;
        constexpr int OWN = LEFT ? 0 : 10; // the bit of the window at which the lane's own four columns begin
        uint32_t sh[N];
        yuv10_in_columns<N>(bx, a.cw, sh);
        const bool has_l = !LEFT && bx > 0, has_r = bx + 1u < a.blocks_x;
        // rows by − 1, by, by + 1, clamped to [0, ch − 1]
        const uint32_t rows[3] = {by > 0 ? by - 1u : 0u, by, by + 1u < a.ch ? by + 1u : a.ch - 1u};
        int32_t hu[3][8], hv[3][8];
#pragma unroll
        for(int r = 0; r < 3; r++)
        {
            const uint8_t *row = u_plane + (size_t)rows[r] * a.s.c_pitch, *v_row = v_plane + (size_t)rows[r] * a.s.c_pitch;
            uint32_t u[4], v[4], lu = 0u, lv = 0u, ru = 0u, rv = 0u; // a column that does not exist is 0 and is never selected
            yuv10_own_chroma<FORMAT>(row, v_row, bx, u, v);
            if(has_l)
                yuv10_chroma_sample<FORMAT>(row, v_row, 4u * bx - 1u, lu, lv);
            if(has_r)
                yuv10_chroma_sample<FORMAT>(row, v_row, 4u * bx + 4u, ru, rv);
            const uint64_t own_u = (uint64_t)(u[0] | (u[1] << 10) | (u[2] << 20)) | ((uint64_t)u[3] << 30);
            const uint64_t own_v = (uint64_t)(v[0] | (v[1] << 10) | (v[2] << 20)) | ((uint64_t)v[3] << 30);
            const uint64_t win_u = (uint64_t)lu | (own_u << OWN) | ((uint64_t)ru << (40 + OWN));
            const uint64_t win_v = (uint64_t)lv | (own_v << OWN) | ((uint64_t)rv << (40 + OWN));
            yuv10_in_row<N>(win_u, sh, hu[r]), yuv10_in_row<N>(win_v, sh, hv[r]);
        }
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
            px[j][i] = yuv10_in_pixel(a.k, (int32_t)yuv10_code<FORMAT>(y[j][i]), su[j][i], sv[j][i]);
    uint32_t *out = reinterpret_cast<uint32_t *>(a.dst + (size_t)blockIdx.z * a.image_stride) + (size_t)ya * a.W + x0;
    yuv_in_store(out, a.W, x0, two_rows, a.rows16, px);
}

template <int FORMAT, bool NEAREST>
__global__ void __launch_bounds__(YUV_LANES_X *YUV_BLOCK_ROWS) yuvs_expand10(const YuvsInArgs a)
{
    yuvs_expand10_block<FORMAT, NEAREST, false>(a);
}

// left-sited chroma, BILINEAR (NEAREST is yuvs_expand10's under either siting)
template <int FORMAT>
__global__ void __launch_bounds__(YUV_LANES_X *YUV_BLOCK_ROWS) yuvs_expand10_left(const YuvsInArgs a)
{
    yuvs_expand10_block<FORMAT, false, true>(a);
}

template <bool PLANAR, int FORMAT, bool LEFT>
__device__ __forceinline__ void yuvs_convert10_block(const YuvsOutArgs &a)
{
    const uint32_t bx = blockIdx.x * YUV_LANES_X + threadIdx.x;
    const uint32_t by = blockIdx.y * YUV_BLOCK_ROWS + threadIdx.y; // wave-uniform
    if(bx >= a.blocks_x || by >= a.ch)
        return;
    const uint32_t x0 = bx * YUV_BLOCK_W;
    const bool two_rows = by * YUV_BLOCK_H + 1u < a.src.H;
    const uint32_t ya = by * YUV_BLOCK_H, yb = two_rows ? ya + 1u : ya; // ya < H: by < ch
    const bool whole = x0 + YUV_BLOCK_W <= a.src.W;                       // all 8 columns inside the view
    uint32_t r[2][8], g[2][8], b[2][8];
    const uint8_t *view = a.src.base + (size_t)blockIdx.z * a.src.view_stride;
    // LEFT: lane 0 of a wave loads pixel column x0 − 1 itself (bx > 0: inside the view), ahead of the block's own loads (yuvs_convert_block)
    [[maybe_unused]] YuvColumn<PLANAR> edge{};
    if constexpr(LEFT)
        if(threadIdx.x == 0 && bx)
            edge = yuv_load_column<PLANAR>(view, a.src.W, a.src.H, a.src.pitch, x0 - 1u, ya, yb);
    yuv_load_block<PLANAR>(view, a.src.W, a.src.H, a.src.pitch, a.rows16, x0, ya, yb, whole, r, g, b);
    uint8_t *frame = a.s.base + (size_t)blockIdx.z * a.s.frame_stride;
    // Y: the row's own samples only, and no row beyond H
#pragma unroll
    for(int j = 0; j < 2; j++)
    {
        uint32_t y[8];
#pragma unroll
        for(int i = 0; i < 8; i++)
            y[i] = yuv10_word<FORMAT>(yuv10_luma(a.k, r[j][i], g[j][i], b[j][i]));
        uint8_t *row = frame + (size_t)(ya + j) * a.s.y_pitch + 16u * bx;
        if(j && !two_rows)
            continue;
        if(whole)
            *reinterpret_cast<uint4 *>(row) = uint4{y[0] | (y[1] << 16), y[2] | (y[3] << 16), y[4] | (y[5] << 16), y[6] | (y[7] << 16)};
        else
        {
#pragma unroll
            for(int i = 0; i < 7; i++) // a ragged block holds at most 7 columns
                if(x0 + i < a.src.W)
                    reinterpret_cast<uint16_t *>(row)[i] = (uint16_t)y[i];
        }
    }
    uint32_t left = 0u;
    if constexpr(LEFT)
    {
        // the left neighbour lane's column 7 in ONE cross-lane move (DPP wave_shr:1), behind the early return: a source lane bx − 1 < bx is
        // always on and always a whole block; lane 0 of a wave keeps `old` and takes the column it loaded above, or its own column 0 (bx = 0)
        const uint32_t mine = yuv_pack_sums(r[0][7] + r[1][7], g[0][7] + g[1][7], b[0][7] + b[1][7]);
        left = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mine, 0x138, 0xf, 0xf, false);
        if(threadIdx.x == 0)
            left = bx ? yuv_column_sums<PLANAR>(edge)
                      : yuv_pack_sums(r[0][0] + r[1][0], g[0][0] + g[1][0], b[0][0] + b[1][0]);
    }
    uint32_t cb[4], cr[4];
#pragma unroll
    for(int i = 0; i < 4; i++)
    {
        yuv10_block_chroma<LEFT>(a.k, r, g, b, left, i, cb[i], cr[i]);
        cb[i] = yuv10_word<FORMAT>(cb[i]), cr[i] = yuv10_word<FORMAT>(cr[i]);
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

template <bool PLANAR, int FORMAT>
__global__ void __launch_bounds__(YUV_LANES_X *YUV_BLOCK_ROWS) yuvs_convert10(const YuvsOutArgs a)
{
    yuvs_convert10_block<PLANAR, FORMAT, false>(a);
}

// left-sited chroma
template <bool PLANAR, int FORMAT>
__global__ void __launch_bounds__(YUV_LANES_X *YUV_BLOCK_ROWS) yuvs_convert10_left(const YuvsOutArgs a)
{
    yuvs_convert10_block<PLANAR, FORMAT, true>(a);
}

// Enqueues the ONE yuvs_expand10 launch for n frames; layout: YUVS_I420 (I010) or YUVS_NV12 (P010).  The caller has checked sizes, alignment
// and memory as for launch_yuvs_expand
inline hipError_t launch_yuvs_expand10(hipStream_t stream, const int layout, const bool nearest, const bool left, const YuvsInArgs &a, const int n)
{
    const dim3 grid = yuvs_grid(a.blocks_x, a.ch, n), block(YUV_LANES_X, YUV_BLOCK_ROWS);
    if(left && !nearest) // a left-sited nearest upload is the nearest kernel: the same bytes
    {
        if(layout == YUVS_NV12)
            hipLaunchKernelGGL((yuvs_expand10_left<YUVS_NV12>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((yuvs_expand10_left<YUVS_I420>), grid, block, 0, stream, a);
    }
    else if(layout == YUVS_NV12)
    {
        if(nearest)
            hipLaunchKernelGGL((yuvs_expand10<YUVS_NV12, true>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((yuvs_expand10<YUVS_NV12, false>), grid, block, 0, stream, a);
    }
    else
    {
        if(nearest)
            hipLaunchKernelGGL((yuvs_expand10<YUVS_I420, true>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((yuvs_expand10<YUVS_I420, false>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

// Enqueues the ONE yuvs_convert10 launch for n views
inline hipError_t launch_yuvs_convert10(hipStream_t stream, const bool planar, const int layout, const bool left, const YuvsOutArgs &a, const int n)
{
    const dim3 grid = yuvs_grid(a.blocks_x, a.ch, n), block(YUV_LANES_X, YUV_BLOCK_ROWS);
    if(left)
    {
        if(planar)
        {
            if(layout == YUVS_NV12)
                hipLaunchKernelGGL((yuvs_convert10_left<true, YUVS_NV12>), grid, block, 0, stream, a);
            else
                hipLaunchKernelGGL((yuvs_convert10_left<true, YUVS_I420>), grid, block, 0, stream, a);
        }
        else
        {
            if(layout == YUVS_NV12)
                hipLaunchKernelGGL((yuvs_convert10_left<false, YUVS_NV12>), grid, block, 0, stream, a);
            else
                hipLaunchKernelGGL((yuvs_convert10_left<false, YUVS_I420>), grid, block, 0, stream, a);
        }
    }
    else if(planar)
    {
        if(layout == YUVS_NV12)
            hipLaunchKernelGGL((yuvs_convert10<true, YUVS_NV12>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((yuvs_convert10<true, YUVS_I420>), grid, block, 0, stream, a);
    }
    else
    {
        if(layout == YUVS_NV12)
            hipLaunchKernelGGL((yuvs_convert10<false, YUVS_NV12>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((yuvs_convert10<false, YUVS_I420>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

} // namespace lfi
