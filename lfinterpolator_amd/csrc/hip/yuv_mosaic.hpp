// yuv_mosaic.hpp — ONE YUV 4:2:0 frame that holds a whole grid of images (a camera-array mosaic, a quilt), split into the RGBA input planes
// where it lies: the kernels behind lfi_upload_mosaic_yuv (include/lfi.h).  No new arithmetic: image g of tile (tx, ty) is what yuvs_expand
// (yuv_surfaces.hpp) makes of the tile taken as a frame of its own — the tables, yuv_in_columns[_left] / yuv_in_row[_left], yuv_in_pixel,
// yuv_in_clamp and yuv_in_store of yuv420_upload.hpp; this header says where a tile's bytes lie in the frame.
//
// The mapping (mosaic_tile, shared with lfi_mosaic_map on the host): tile t = first_tile + k of the frame in ROWS order sits at column
// tx = t % tiles_x of tile row r = t / tiles_x, which is frame row ty = r (BOTTOM_UP: tiles_y − 1 − r); it becomes image g0 + k (ROWS) or
// tx · rows + r (GRID: camera column tx, camera row r).  k, and with it tx, ty and g, are wave-uniform: the tile is grid.z.
//
// Geometry.  The frame is MW × MH = tiles_x·W × tiles_y·H, W and H even (a 2 × 2 block never lies across two tiles), cw = W/2, ch = H/2.
//   the tile's Y origin       ty·H·y_pitch + tx·W            rows of y_pitch
//   the tile's chroma origin  ty·ch·c_pitch + tx·cw          (I420, in each of the Cb and Cr planes)
//                             ty·ch·c_pitch + tx·W           (NV12)
// Decomposition: that of yuvs_expand.  A lane owns 8 × 2 pixels, a wave 64 neighbouring blocks of one block row OF ONE TILE, a workgroup four
// block rows; no LDS, no scratch, no atomics.  What the launches rely on is yuvs_expand's contract for the FRAME: the Y plane's base, y_pitch
// and the chroma planes' bases multiples of 8 (I420 chroma bases: of 4), c_pitch a multiple of 4 (I420) or 8 (NV12) — surfaces read in place
// have multiples of 16 throughout, the staged planes are yuv_geometry's of the copied tile rows.
//
// UNALIGNED = false — W a multiple of 8.  Every tile origin is then as aligned as the frame's: tx·W is a multiple of 8, tx·cw of 4.  The kernel
// calls yuvs_block_pixels UNCHANGED on a per-tile copy of the arguments: the frame pointer moved to the tile's Y origin, c_offset and
// cr_offset patched to reach the tile's chroma origin from there, W, H, cw, ch, blocks_x those of the tile.  Proof that every load lies
// inside the tile, hence inside the pitch of its own plane row: blocks_x = W/8, so
//   Y      8 bytes at tx·W + 8·bx:            8·bx + 8 ≤ W
//   I420   the dword at tx·cw + 4·bx:         4·bx + 4 ≤ cw; the dwords left and right of it only where bx > 0 and bx + 1 < blocks_x
//   NV12   8 bytes at tx·W + 8·bx:            8·bx + 8 ≤ W;  the dwords left and right of it only where bx > 0 and bx + 1 < blocks_x
// and chroma rows are clamped to [0, ch − 1] of the tile.  No byte outside the tile is read at all.
//
// UNALIGNED = true — every other even W (1638, 820, 420, 6).  A tile origin is then any even byte of a Y or NV12 row and any byte of an I420
// chroma row, so the pieces yuvs_block_pixels loads (8 bytes of Y; the own dword or 8 bytes of chroma, the dword left and the dword right of
// them) would be misaligned.  No misaligned pointer is dereferenced: a piece at byte `off` of a plane row is assembled from the naturally
// aligned dwords that cover it, at (off & ~3) + 4·i, shifted by the byte phase off & 3 — one v_alignbyte_b32 per dword of the piece.  The
// phase is wave-uniform (off = the tile's origin + 8·bx or 4·bx).  The assembled pieces feed the same windows as in yuvs_block_pixels, so the
// definition's clamp stays the same set of byte positions.  Rules, with their proof:
//   - A covering dword at byte w of a row is loaded only where w + 4 ≤ the row's pitch (mosaic_word), else it reads as 0.  Rows start on
//     dword boundaries (contract above) and the pitches are multiples of 4, so the dword that holds a byte at position o < pitch lies at
//     (o & ~3) + 4 ≤ pitch: every byte of a plane row CAN be loaded, and no load leaves the pitch of its own plane row — not at the last
//     block of a frame row, and not in the last row of the last plane, behind which the caller's memory may end (a plane occupies
//     rows · pitch bytes, include/lfi.h).  The extra dword a non-zero phase needs falls under the same test.
//   - Every byte that reaches an image is a tile's own: Y bytes at tx·W + x, x < W; chroma bytes of columns clamped to [0, cw − 1] of the
//     tile (yuv_in_columns[_left] with the tile's cw) and rows clamped to [0, ch − 1] of the tile.  All of them lie below MW (cw·tiles_x,
//     2·cw·tiles_x) ≤ the pitch, so the rule above never replaces one of them by 0.
//   - The left and right chroma neighbours are used only where bx > 0 and bx + 1 < blocks_x OF THE TILE; elsewhere they read as 0 and are
//     never selected.  Covering dwords do hold bytes of the neighbouring tile, of tiles outside [first_tile, first_tile + n) or of pitch
//     padding; those bytes are Y of pixels beyond W, which yuv_in_store does not store, or chroma columns beyond cw − 1, which no window
//     position selects.
// Cost against the aligned path: one dword more per piece where the phase is not 0 (Y: 3 dwords for 8 bytes), the shifts, and 4-byte loads
// in place of 8-byte ones.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "yuv_surfaces.hpp"

namespace lfi {

// lfi_mosaic with the context's grid and the call's g0 (include/lfi.h); the entry point has validated it (lfi_mosaic_map)
struct MosaicMap
{
    uint32_t tiles_x, tiles_y, first_tile;
    uint32_t grid;      // LFI_MOSAIC_GRID: g = tx·rows + r; else g = g0 + k
    uint32_t bottom_up; // LFI_MOSAIC_BOTTOM_UP
    uint32_t rows, g0;
};

// tile k of the map: its column tx and row ty in the frame, and the image g it becomes.  The ONE definition: lfi_mosaic_map is this function
// behind its checks, the kernels call it with k = their grid.z
__host__ __device__ inline void mosaic_tile(const MosaicMap &m, const uint32_t k, uint32_t &tx, uint32_t &ty, uint32_t &g)
{
    const uint32_t t = m.first_tile + k, r = t / m.tiles_x;
    tx = t - r * m.tiles_x;
    ty = m.bottom_up ? m.tiles_y - 1u - r : r;
    g = m.grid ? tx * m.rows + r : m.g0 + k;
}

struct YuvsMosaicArgs
{
    YuvsInArgs in;    // s: the FRAME's surfaces (or the staged tile rows); dst: image 0 of the grid; W, H, cw, ch, blocks_x, rows16: a TILE's
    MosaicMap map;
    uint32_t k0;      // the launch's first tile: tile k0 + grid.z
    uint32_t ty_bias; // the frame's tile row that is tile row 0 of s (staged chunks hold some tile rows only; in place: 0)
};

// the aligned dword at byte w (a multiple of 4) of a plane row, 0 where it does not lie inside the row's pitch
__device__ __forceinline__ uint32_t mosaic_word(const uint8_t *row, const uint32_t w, const uint32_t pitch)
{
    return w + 4u <= pitch ? *reinterpret_cast<const uint32_t *>(row + w) : 0u;
}

// bytes [phase, phase + 4) of the eight bytes lo, hi
__device__ __forceinline__ uint32_t mosaic_shift(const uint32_t lo, const uint32_t hi, const uint32_t phase)
{
    return __builtin_amdgcn_alignbyte(hi, lo, phase);
}

// yuvs_block_pixels for block (bx, by) of the tile whose Y origin is column ox of Y row oy of the frame a.s, a.W … a.blocks_x the tile's:
// the same pieces into the same windows, assembled from aligned dwords (the header comment's rules)
template <int FORMAT, bool NEAREST, bool LEFT>
__device__ __forceinline__ void yuvs_mosaic_block_pixels(const YuvsInArgs &a, const uint32_t ox, const uint32_t oy, const uint32_t bx, const uint32_t by,
                                                         uint32_t (&px)[2][8])
{
    const uint32_t ya = by * YUV_BLOCK_H;
    const bool two_rows = ya + 1u < a.H; // H is even: always; kept as in yuvs_block_pixels
    const uint8_t *frame = a.s.base;
    // Y: 8 bytes at ox + 8·bx of rows oy + ya and oy + ya + 1, from three covering dwords each (two where the phase is 0)
    uint32_t y[2][8];
    {
        const uint32_t off = ox + bx * YUV_BLOCK_W, w = off & ~3u, ph = off & 3u;
#pragma unroll
        for(int j = 0; j < 2; j++)
        {
            const uint8_t *row = frame + (size_t)(oy + (j && two_rows ? ya + 1u : ya)) * a.s.y_pitch;
            const uint32_t w0 = mosaic_word(row, w, a.s.y_pitch), w1 = mosaic_word(row, w + 4u, a.s.y_pitch);
            const uint32_t w2 = ph ? mosaic_word(row, w + 8u, a.s.y_pitch) : 0u;
            yuv_in_bytes(uint2{mosaic_shift(w0, w1, ph), mosaic_shift(w1, w2, ph)}, y[j]);
        }
    }
    const uint32_t cy0 = oy >> 1; // the tile's first chroma row
    // byte of a chroma row at which the lane's own columns begin, its covering dword and phase
    const uint32_t c_off = (FORMAT == YUVS_NV12 ? ox + 8u * bx : (ox >> 1) + 4u * bx), cw0 = c_off & ~3u, cph = c_off & 3u;
    int32_t su[2][8], sv[2][8];
    if constexpr(NEAREST)
    {
        uint32_t u, v;
        if constexpr(FORMAT == YUVS_NV12)
        {
            const uint8_t *row = frame + a.s.c_offset + (size_t)(cy0 + by) * a.s.c_pitch;
            const uint32_t w0 = mosaic_word(row, cw0, a.s.c_pitch), w1 = mosaic_word(row, cw0 + 4u, a.s.c_pitch);
            const uint32_t w2 = cph ? mosaic_word(row, cw0 + 8u, a.s.c_pitch) : 0u;
            const uint32_t lo = mosaic_shift(w0, w1, cph), hi = mosaic_shift(w1, w2, cph);
            u = yuvs_component(lo, hi, 0), v = yuvs_component(lo, hi, 1);
        }
        else
        {
            uint32_t c[2];
#pragma unroll
            for(int p = 0; p < 2; p++)
            {
                const uint8_t *row = frame + (p ? a.s.cr_offset : a.s.c_offset) + (size_t)(cy0 + by) * a.s.c_pitch;
                const uint32_t w0 = mosaic_word(row, cw0, a.s.c_pitch), w1 = cph ? mosaic_word(row, cw0 + 4u, a.s.c_pitch) : 0u;
                c[p] = mosaic_shift(w0, w1, cph);
            }
            u = c[0], v = c[1];
        }
#pragma unroll
        for(int i = 0; i < 8; i++)
            su[0][i] = su[1][i] = 16 * (int32_t)((u >> (8 * (i >> 1))) & 0xffu), sv[0][i] = sv[1][i] = 16 * (int32_t)((v >> (8 * (i >> 1))) & 0xffu);
    }
    else
    {
        uint32_t sh[LEFT ? 5 : 6];
        if constexpr(LEFT)
            yuv_in_columns_left(bx, a.cw, sh);
        else
            yuv_in_columns(bx, a.cw, sh);
        constexpr int OWN = LEFT ? 0 : 8;
        const bool has_l = !LEFT && bx > 0, has_r = bx + 1u < a.blocks_x; // of the TILE
        const uint32_t rows[3] = {by > 0 ? by - 1u : 0u, by, by + 1u < a.ch ? by + 1u : a.ch - 1u};
        int32_t hu[3][8], hv[3][8];
#pragma unroll
        for(int r = 0; r < 3; r++)
        {
            uint64_t win[2];
            if constexpr(FORMAT == YUVS_NV12)
            {
                // own: 8 bytes at c_off; left: the dword at c_off − 4 (bx > 0: c_off ≥ 8); right: the dword at c_off + 8
                const uint8_t *row = frame + a.s.c_offset + (size_t)(cy0 + rows[r]) * a.s.c_pitch;
                const uint32_t w0 = mosaic_word(row, cw0, a.s.c_pitch), w1 = mosaic_word(row, cw0 + 4u, a.s.c_pitch);
                const uint32_t w2 = (has_r || cph) ? mosaic_word(row, cw0 + 8u, a.s.c_pitch) : 0u;
                const uint32_t w3 = (has_r && cph) ? mosaic_word(row, cw0 + 12u, a.s.c_pitch) : 0u;
                const uint32_t lo = mosaic_shift(w0, w1, cph), hi = mosaic_shift(w1, w2, cph);
                uint32_t left = 0u;
                if constexpr(!LEFT)
                    left = has_l ? mosaic_shift(mosaic_word(row, cw0 - 4u, a.s.c_pitch), w0, cph) : 0u;
                const uint32_t right = has_r ? mosaic_shift(w2, w3, cph) : 0u;
#pragma unroll
                for(int p = 0; p < 2; p++)
                    win[p] = (uint64_t)((left >> (16 + 8 * p)) & 0xffu) | ((uint64_t)yuvs_component(lo, hi, p) << OWN) |
                             ((uint64_t)((right >> (8 * p)) & 0xffu) << (32 + OWN));
            }
            else
            {
#pragma unroll
                for(int p = 0; p < 2; p++)
                {
                    // own: the dword at c_off; left: the dword at c_off − 4 (bx > 0: c_off ≥ 4); right: the dword at c_off + 4
                    const uint8_t *row = frame + (p ? a.s.cr_offset : a.s.c_offset) + (size_t)(cy0 + rows[r]) * a.s.c_pitch;
                    const uint32_t w0 = mosaic_word(row, cw0, a.s.c_pitch);
                    const uint32_t w1 = (has_r || cph) ? mosaic_word(row, cw0 + 4u, a.s.c_pitch) : 0u;
                    const uint32_t w2 = (has_r && cph) ? mosaic_word(row, cw0 + 8u, a.s.c_pitch) : 0u;
                    uint32_t left = 0u;
                    if constexpr(!LEFT)
                        left = has_l ? mosaic_shift(mosaic_word(row, cw0 - 4u, a.s.c_pitch), w0, cph) : 0u;
                    const uint32_t own = mosaic_shift(w0, w1, cph), right = has_r ? mosaic_shift(w1, w2, cph) : 0u;
                    win[p] = (uint64_t)(left >> 24) | ((uint64_t)own << OWN) | ((uint64_t)(right & 0xffu) << (32 + OWN));
                }
            }
            if constexpr(LEFT)
                yuv_in_row_left(win[0], sh, hu[r]), yuv_in_row_left(win[1], sh, hv[r]);
            else
                yuv_in_row(win[0], sh, hu[r]), yuv_in_row(win[1], sh, hv[r]);
        }
#pragma unroll
        for(int j = 0; j < 2; j++)
#pragma unroll
            for(int i = 0; i < 8; i++)
                su[j][i] = 3 * hu[1][i] + hu[j ? 2 : 0][i], sv[j][i] = 3 * hv[1][i] + hv[j ? 2 : 0][i];
    }
#pragma unroll
    for(int j = 0; j < 2; j++)
#pragma unroll
        for(int i = 0; i < 8; i++)
            px[j][i] = yuv_in_pixel(a.k, (int32_t)y[j][i], su[j][i], sv[j][i]);
}

// The aligned path's tile as a frame of its own (W a multiple of 8): t, the caller's copy of `in`, gets c_offset and cr_offset patched so that
// yuvs_block_pixels, which reads Y at frame + row·y_pitch and chroma at frame + c_offset (cr_offset) + row·c_pitch, reaches the tile whose Y
// origin is column ox of Y row oy of the frame in.s from the pointer returned, the tile's Y origin.  Called by yuv_mosaic_derived.hpp.
// yuvs_mosaic_block below keeps the same six lines in its own body: a function of its own is simplified on its own before it is inlined, and
// in every shape tried that reordered the offset arithmetic of two to six of the twelve yuvs_mosaic_expand[_left] kernels, which must stay
// instruction for instruction what they were (profiles/r26_mosaic_derived_notes.md)
template <int FORMAT>
__device__ __forceinline__ const uint8_t *yuvs_mosaic_tile_frame(const YuvsInArgs &in, const uint32_t ox, const uint32_t oy, YuvsInArgs &t)
{
    const size_t y_origin = (size_t)oy * in.s.y_pitch + ox;
    const size_t c_origin = (size_t)(oy >> 1) * in.s.c_pitch + (FORMAT == YUVS_NV12 ? ox : ox >> 1);
    t.s.c_offset = in.s.c_offset + c_origin - y_origin; // ≥ 0: the chroma planes lie behind the Y plane
    t.s.cr_offset = in.s.cr_offset + c_origin - y_origin;
    return in.s.base + y_origin;
}

template <int FORMAT, bool NEAREST, bool LEFT, bool UNALIGNED>
__device__ __forceinline__ void yuvs_mosaic_block(const YuvsMosaicArgs &a)
{
    const uint32_t bx = blockIdx.x * YUV_LANES_X + threadIdx.x;
    const uint32_t by = blockIdx.y * YUV_BLOCK_ROWS + threadIdx.y; // wave-uniform
    if(bx >= a.in.blocks_x || by >= a.in.ch)
        return;
    uint32_t tx, ty, g; // wave-uniform
    mosaic_tile(a.map, a.k0 + blockIdx.z, tx, ty, g);
    const uint32_t ox = tx * a.in.W, oy = (ty - a.ty_bias) * a.in.H; // the tile's Y origin: column and row of the frame a.in.s
    const uint32_t x0 = bx * YUV_BLOCK_W, ya = by * YUV_BLOCK_H;
    uint32_t px[2][8];
    if constexpr(UNALIGNED)
        yuvs_mosaic_block_pixels<FORMAT, NEAREST, LEFT>(a.in, ox, oy, bx, by, px);
    else
    {
        // the tile as a frame of its own: yuvs_block_pixels reads Y at frame + row·y_pitch, chroma at frame + c_offset (cr_offset) + row·c_pitch
        YuvsInArgs t = a.in;
        const size_t y_origin = (size_t)oy * a.in.s.y_pitch + ox;
        const size_t c_origin = (size_t)(oy >> 1) * a.in.s.c_pitch + (FORMAT == YUVS_NV12 ? ox : ox >> 1);
        t.s.c_offset = a.in.s.c_offset + c_origin - y_origin; // ≥ 0: the chroma planes lie behind the Y plane
        t.s.cr_offset = a.in.s.cr_offset + c_origin - y_origin;
        yuvs_block_pixels<FORMAT, NEAREST, LEFT>(t, a.in.s.base + y_origin, bx, by, px);
    }
    uint32_t *out = reinterpret_cast<uint32_t *>(a.in.dst + (size_t)g * a.in.image_stride) + (size_t)ya * a.in.W + x0;
    yuv_in_store(out, a.in.W, x0, ya + 1u < a.in.H, a.in.rows16, px);
}

template <int FORMAT, bool NEAREST, bool UNALIGNED>
__global__ void __launch_bounds__(YUV_LANES_X *YUV_BLOCK_ROWS) yuvs_mosaic_expand(const YuvsMosaicArgs a)
{
    yuvs_mosaic_block<FORMAT, NEAREST, false, UNALIGNED>(a);
}

// left-sited chroma, BILINEAR (NEAREST is yuvs_mosaic_expand's under either siting)
template <int FORMAT, bool UNALIGNED>
__global__ void __launch_bounds__(YUV_LANES_X *YUV_BLOCK_ROWS) yuvs_mosaic_expand_left(const YuvsMosaicArgs a)
{
    yuvs_mosaic_block<FORMAT, false, true, UNALIGNED>(a);
}

// Enqueues the ONE launch for n tiles from a.k0 on.  The caller has checked the map, sizes, alignment and memory: a.in.s holds the tile rows
// the n tiles lie in, a.in.dst the grid.  unaligned: the tile width is no multiple of 8
inline hipError_t launch_yuvs_mosaic_expand(hipStream_t stream, const int format, const bool nearest, const bool left, const bool unaligned,
                                            const YuvsMosaicArgs &a, const int n)
{
    const dim3 grid = yuvs_grid(a.in.blocks_x, a.in.ch, n), block(YUV_LANES_X, YUV_BLOCK_ROWS);
    // KERNEL<…, UNALIGNED>: the two instantiations of one kernel that differ in the last template argument
#define LFI_MOSAIC_LAUNCH(...)                                                        \
    do                                                                                \
    {                                                                                 \
        if(unaligned)                                                                 \
            hipLaunchKernelGGL((__VA_ARGS__, true >), grid, block, 0, stream, a);     \
        else                                                                          \
            hipLaunchKernelGGL((__VA_ARGS__, false >), grid, block, 0, stream, a);    \
    } while(0)
    if(left && !nearest) // a left-sited nearest upload is the nearest kernel: the same bytes
    {
        if(format == YUVS_NV12)
            LFI_MOSAIC_LAUNCH(yuvs_mosaic_expand_left < YUVS_NV12);
        else
            LFI_MOSAIC_LAUNCH(yuvs_mosaic_expand_left < YUVS_I420);
    }
    else if(format == YUVS_NV12)
    {
        if(nearest)
            LFI_MOSAIC_LAUNCH(yuvs_mosaic_expand < YUVS_NV12, true);
        else
            LFI_MOSAIC_LAUNCH(yuvs_mosaic_expand < YUVS_NV12, false);
    }
    else
    {
        if(nearest)
            LFI_MOSAIC_LAUNCH(yuvs_mosaic_expand < YUVS_I420, true);
        else
            LFI_MOSAIC_LAUNCH(yuvs_mosaic_expand < YUVS_I420, false);
    }
#undef LFI_MOSAIC_LAUNCH
    return hipGetLastError();
}

} // namespace lfi
