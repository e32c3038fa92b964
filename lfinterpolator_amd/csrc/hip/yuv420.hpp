// yuv420.hpp — 8-bit YUV 4:2:0 frames of rendered views: the definition's arithmetic, its coefficient tables and the geometry of a frame.  The
// kernel that uses them is yuvs_convert (yuv_surfaces.hpp), behind lfi_download_views_yuv420, lfi_download_views_yuv and
// lfi_render_stream_yuv420: what an encoder or player takes, 1.5 bytes per pixel instead of the 4 of an RGBA download.
//
// Definition (include/lfi.h), integers only.  A frame of a W × H view is the Y plane [H][W], then Cb and Cr [ch][cw] with cw = (W + 1) >> 1,
// ch = (H + 1) >> 1.  With the coefficient row (matrix, range) of YUV_COEFFS:
//     Y[y][x]  = y_off + ((yR·R + yG·G + yB·B + 2¹⁵) >> 16)
//     Cb[cy][cx] = min(255, (2²⁵ + 2¹⁷ + uR·ΣR + uG·ΣG + uB·ΣB) >> 18),   Cr likewise with the Cr coefficients,
// ΣR, ΣG, ΣB summed over the four pixels (min(2cx + i, W − 1), min(2cy + j, H − 1)), i, j ∈ {0, 1} (centre siting, Y4M's C420jpeg; an odd
// last column or row is replicated).  The bracket lies in (0, 2²⁷): it is computed in u32 (the negative coefficients wrap, the sum does
// not), one rounding, no shift of a negative number.
//
// Left siting (lfi_set_yuv_siting, include/lfi.h): the sums become Σ_j [R(xl, y_j) + 2·R(xc, y_j) + R(xr, y_j)] with xl = max(2cx − 1, 0), xc = 2cx,
// xr = min(2cx + 1, W − 1) (total weight 8) and the sample min(255, (2²⁶ + 2¹⁸ + …) >> 19): the bracket lies in (0, 2²⁸], still u32.
// yuv_chroma_left, yuv_block_chroma_left, and yuv_pack_sums / yuv_load_column / yuv_column_sums for the one pixel column a block needs from
// outside itself; the kernel is yuvs_convert_left (yuv_surfaces.hpp).
//
// Here: YUV_COEFFS; the block shape of every YUV kernel (a lane owns 8 columns × 2 rows, a workgroup is 64 lanes × 4 block rows);
// YuvSurfaces, the planes of a batch of frames as a kernel sees them; yuv_geometry, the tight host frame and the padded staged frame a host call's frames pass through on the device (Y pitch a multiple of 8,
// chroma pitch of 4, an even number of Y rows: every word of a row lies inside it); yuv_luma and yuv_chroma; yuv_load_block, a lane's
// 8 × 2 pixels out of RGBA or planar views with the definition's clamp; yuv_block_chroma.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace lfi {

constexpr int YUV_LANES_X = 64;   // lanes (blocks) of a workgroup along x: one wave
constexpr int YUV_BLOCK_ROWS = 4; // block rows of a workgroup: one wave each
constexpr int YUV_BLOCK_W = 8;    // pixel columns of a lane's block
constexpr int YUV_BLOCK_H = 2;    // pixel rows of a lane's block

// 16-bit fixed point: round(c · scale · 2¹⁶), scale = 219/255 (limited luma), 224/255 (limited chroma), 1 (full); G adjusted so that Y sums
// to 56284 (limited) / 65536 (full) and Cb, Cr to 0.  Row = matrix · 2 + range (LFI_YUV_BT709 / _BT601, LFI_YUV_LIMITED / _FULL).
struct YuvCoeffs
{
    int32_t y[3], cb[3], cr[3]; // R, G, B
    uint32_t y_off;
};

constexpr YuvCoeffs YUV_COEFFS[4] = {
    {{11966, 40254, 4064}, {-6596, -22188, 28784}, {28784, -26145, -2639}, 16},  // BT.709 limited
    {{13933, 46871, 4732}, {-7509, -25259, 32768}, {32768, -29763, -3005}, 0},   // BT.709 full
    {{16829, 33039, 6416}, {-9714, -19070, 28784}, {28784, -24103, -4681}, 16},  // BT.601 limited
    {{19595, 38470, 7471}, {-11058, -21710, 32768}, {32768, -27439, -5329}, 0},  // BT.601 full
};

// the padded staged planes of one frame, and the tight host frame
struct YuvGeometry
{
    uint32_t W, H, cw, ch;
    uint32_t y_pitch, c_pitch, y_rows; // device: W rounded up to 8, half of it (= cw rounded up to 4), 2·ch
    size_t frame_bytes;                // host: W·H + 2·cw·ch
    size_t dev_frame_bytes;            // device: y_pitch·y_rows + 2·c_pitch·ch (a multiple of 8)
    bool tight;                        // W a multiple of 8 and H even: the device frame IS the host frame
    uint32_t bps;                      // bytes per sample: 1, or 2 (the 10-bit formats, yuv10.hpp): both pitches and both sizes are bps times the above
};

inline YuvGeometry yuv_geometry(const int width, const int height, const uint32_t bps = 1)
{
    YuvGeometry g{};
    g.W = width, g.H = height, g.bps = bps;
    g.cw = (g.W + 1) >> 1, g.ch = (g.H + 1) >> 1;
    g.y_pitch = (g.W + YUV_BLOCK_W - 1) / YUV_BLOCK_W * YUV_BLOCK_W * bps;
    g.c_pitch = g.y_pitch / 2;
    g.y_rows = g.ch * YUV_BLOCK_H;
    g.frame_bytes = ((size_t)g.W * g.H + 2 * (size_t)g.cw * g.ch) * bps;
    g.dev_frame_bytes = (size_t)g.y_pitch * g.y_rows + 2 * (size_t)g.c_pitch * g.ch;
    g.tight = g.y_pitch == g.W * bps && g.y_rows == g.H;
    return g;
}

constexpr int YUVS_I420 = 0; // LFI_YUV_I420
constexpr int YUVS_NV12 = 1; // LFI_YUV_NV12

// frame 0 of a batch of surfaces as a kernel sees it (yuv_surfaces.hpp, quilt_yuv.hpp)
struct YuvSurfaces
{
    uint8_t *base;                                 // the Y plane of frame 0
    size_t frame_stride, c_offset, cr_offset;      // cr_offset: I420 only
    uint32_t y_pitch, c_pitch;
};

__device__ inline uint32_t yuv_luma(const YuvCoeffs &k, const uint32_t r, const uint32_t g, const uint32_t b)
{
    return k.y_off + (((uint32_t)k.y[0] * r + (uint32_t)k.y[1] * g + (uint32_t)k.y[2] * b + 0x8000u) >> 16);
}

// c: the Cb or the Cr coefficients; sr, sg, sb: the sums over the four pixels.  u32 throughout: the products of the negative coefficients
// wrap, the bracket (true value in (0, 2²⁷)) does not
__device__ inline uint32_t yuv_chroma(const int32_t (&c)[3], const uint32_t sr, const uint32_t sg, const uint32_t sb)
{
    const uint32_t v = ((1u << 25) + (1u << 17) + (uint32_t)c[0] * sr + (uint32_t)c[1] * sg + (uint32_t)c[2] * sb) >> 18;
    return v < 255u ? v : 255u;
}

// left siting: sr, sg, sb are the sums of weight 8; the bracket's true value lies in (0, 2²⁸]
__device__ inline uint32_t yuv_chroma_left(const int32_t (&c)[3], const uint32_t sr, const uint32_t sg, const uint32_t sb)
{
    const uint32_t v = ((1u << 26) + (1u << 18) + (uint32_t)c[0] * sr + (uint32_t)c[1] * sg + (uint32_t)c[2] * sb) >> 19;
    return v < 255u ? v : 255u;
}

// The R, G, B of a lane's block of 8 columns × 2 rows (rows ya and yb, columns x0 … x0 + 7 clamped to W − 1) of one view: RGBA planes
// [H][W], or (PLANAR) byte planes [R,G,B][H][pitch].  whole: all 8 columns lie inside the view
template <bool PLANAR>
__device__ __forceinline__ void yuv_load_block(const uint8_t *view, const uint32_t W, const uint32_t H, const uint32_t pitch, const uint32_t rows16,
                                               const uint32_t x0, const uint32_t ya, const uint32_t yb, const bool whole, uint32_t (&r)[2][8],
                                               uint32_t (&g)[2][8], uint32_t (&b)[2][8])
{
    if constexpr(PLANAR)
    {
        // every row is `pitch` bytes long and pitch ≥ y_pitch: the 8-byte load stays inside it; the bytes beyond the view are replaced
        const uint32_t last = whole ? 7u : W - 1u - x0; // the block's last column inside the view (x0 < W: x0 < y_pitch < W + 8)
        const size_t plane = (size_t)H * pitch;
#pragma unroll
        for(int j = 0; j < 2; j++)
        {
            const uint8_t *row = view + (size_t)(j ? yb : ya) * pitch + x0;
            const uint2 pr = *reinterpret_cast<const uint2 *>(row);
            const uint2 pg = *reinterpret_cast<const uint2 *>(row + plane);
            const uint2 pb = *reinterpret_cast<const uint2 *>(row + 2 * plane);
#pragma unroll
            for(int i = 0; i < 8; i++)
            {
                r[j][i] = ((i < 4 ? pr.x : pr.y) >> (8 * (i & 3))) & 0xffu;
                g[j][i] = ((i < 4 ? pg.x : pg.y) >> (8 * (i & 3))) & 0xffu;
                b[j][i] = ((i < 4 ? pb.x : pb.y) >> (8 * (i & 3))) & 0xffu;
            }
            if(!whole)
            {
                const uint32_t sh = 8u * (last & 3u);
                const uint32_t lr = ((last < 4u ? pr.x : pr.y) >> sh) & 0xffu, lg = ((last < 4u ? pg.x : pg.y) >> sh) & 0xffu,
                               lb = ((last < 4u ? pb.x : pb.y) >> sh) & 0xffu;
#pragma unroll
                for(int i = 1; i < 8; i++)
                    if((uint32_t)i > last)
                        r[j][i] = lr, g[j][i] = lg, b[j][i] = lb;
            }
        }
    }
    else
    {
        const uint32_t *px = reinterpret_cast<const uint32_t *>(view);
#pragma unroll
        for(int j = 0; j < 2; j++)
        {
            const uint32_t *row = px + (size_t)(j ? yb : ya) * W;
            uint32_t p[8];
            if(whole && rows16)
            {
                const uint4 lo = *reinterpret_cast<const uint4 *>(row + x0), hi = *reinterpret_cast<const uint4 *>(row + x0 + 4);
                p[0] = lo.x, p[1] = lo.y, p[2] = lo.z, p[3] = lo.w, p[4] = hi.x, p[5] = hi.y, p[6] = hi.z, p[7] = hi.w;
            }
            else
            {
#pragma unroll
                for(int i = 0; i < 8; i++)
                    p[i] = row[x0 + i < W ? x0 + i : W - 1u];
            }
#pragma unroll
            for(int i = 0; i < 8; i++)
                r[j][i] = p[i] & 0xffu, g[j][i] = (p[i] >> 8) & 0xffu, b[j][i] = (p[i] >> 16) & 0xffu;
        }
    }
}

// left siting: the two-row sums of a pixel column's R, G and B (≤ 510 each), ten bits apiece
__device__ __forceinline__ uint32_t yuv_pack_sums(const uint32_t r, const uint32_t g, const uint32_t b)
{
    return r | (g << 10) | (b << 20);
}

// Pixel column x < W, rows ya and yb, of one view, as loaded: six bytes of PLANAR views (R, G, B of row ya, then of yb), two RGBA dwords.
// The loads only — yuv_column_sums adds them up where the value is needed, so that the loads are in flight beside the block's own
template <bool PLANAR>
struct YuvColumn
{
    uint32_t v[PLANAR ? 6 : 2];
};

template <bool PLANAR>
__device__ __forceinline__ YuvColumn<PLANAR> yuv_load_column(const uint8_t *view, const uint32_t W, const uint32_t H, const uint32_t pitch, const uint32_t x,
                                                             const uint32_t ya, const uint32_t yb)
{
    YuvColumn<PLANAR> c;
    if constexpr(PLANAR)
    {
        const size_t plane = (size_t)H * pitch;
        const uint8_t *pa = view + (size_t)ya * pitch + x, *pb = view + (size_t)yb * pitch + x;
#pragma unroll
        for(int k = 0; k < 3; k++)
            c.v[k] = pa[k * plane], c.v[3 + k] = pb[k * plane];
    }
    else
    {
        const uint32_t *px = reinterpret_cast<const uint32_t *>(view);
        c.v[0] = px[(size_t)ya * W + x], c.v[1] = px[(size_t)yb * W + x];
    }
    return c;
}

template <bool PLANAR>
__device__ __forceinline__ uint32_t yuv_column_sums(const YuvColumn<PLANAR> &c)
{
    if constexpr(PLANAR)
        return yuv_pack_sums(c.v[0] + c.v[3], c.v[1] + c.v[4], c.v[2] + c.v[5]);
    else
    {
        const uint32_t p = c.v[0], q = c.v[1];
        return yuv_pack_sums((p & 0xffu) + (q & 0xffu), ((p >> 8) & 0xffu) + ((q >> 8) & 0xffu), ((p >> 16) & 0xffu) + ((q >> 16) & 0xffu));
    }
}

// Cb and Cr of the block's chroma column i: the sums over its four pixels
__device__ __forceinline__ void yuv_block_chroma(const YuvCoeffs &k, const uint32_t (&r)[2][8], const uint32_t (&g)[2][8], const uint32_t (&b)[2][8], const int i,
                                                 uint32_t &cb, uint32_t &cr)
{
    const uint32_t sr = r[0][2 * i] + r[0][2 * i + 1] + r[1][2 * i] + r[1][2 * i + 1];
    const uint32_t sg = g[0][2 * i] + g[0][2 * i + 1] + g[1][2 * i] + g[1][2 * i + 1];
    const uint32_t sb = b[0][2 * i] + b[0][2 * i + 1] + b[1][2 * i] + b[1][2 * i + 1];
    cb = yuv_chroma(k.cb, sr, sg, sb);
    cr = yuv_chroma(k.cr, sr, sg, sb);
}

// Left siting: Cb and Cr of the block's chroma column i from v(2i − 1) + 2·v(2i) + v(2i + 1), v(k) the two-row sums of block column k.
// left: v(−1) as yuv_pack_sums packs it — the sums of pixel column x0 − 1 (of column 0 where x0 = 0), all a block needs from outside itself
__device__ __forceinline__ void yuv_block_chroma_left(const YuvCoeffs &k, const uint32_t (&r)[2][8], const uint32_t (&g)[2][8], const uint32_t (&b)[2][8],
                                                      const uint32_t left, const int i, uint32_t &cb, uint32_t &cr)
{
    const int c = 2 * i, n = 2 * i + 1;
    uint32_t lr, lg, lb;
    if(i == 0)
        lr = left & 0x3ffu, lg = (left >> 10) & 0x3ffu, lb = left >> 20;
    else
        lr = r[0][c - 1] + r[1][c - 1], lg = g[0][c - 1] + g[1][c - 1], lb = b[0][c - 1] + b[1][c - 1];
    const uint32_t sr = lr + 2u * (r[0][c] + r[1][c]) + r[0][n] + r[1][n];
    const uint32_t sg = lg + 2u * (g[0][c] + g[1][c]) + g[0][n] + g[1][n];
    const uint32_t sb = lb + 2u * (b[0][c] + b[1][c]) + b[0][n] + b[1][n];
    cb = yuv_chroma_left(k.cb, sr, sg, sb);
    cr = yuv_chroma_left(k.cr, sr, sg, sb);
}

} // namespace lfi
