// yuv_derived.hpp — YUV 4:2:0 frames expanded straight into the derived planar copy of the inputs, behind
// lfi_upload_images_yuv_derived: a context that holds only that copy (lfi_release_inputs) takes a video's next time step in ONE pass —
// 1.5 bytes read and 3 written per pixel·image, where yuvs_expand and planar_build together move 12.5.  It reads the frames exactly as
// yuvs_expand does (yuv_surfaces.hpp: yuvs_block_pixels, the same loads, clamps and arithmetic, the same alignment contract, no value taken
// from pitch padding) and writes what planar_build (blend_planar.hpp) would have written from yuvs_expand's RGBA image:
//     byte j of a row of plane (g, c) = channel c of pixel clamp(j − padx − phase[g], 0, W − 1)       for every j in [0, pitch)
// the replicated padding on both sides included.
//
// The store side decides the shape.  first = padx + phase[g] is any value mod 128 and of either parity, so the input-aligned 8 × 2 blocks do
// not line up with aligned words of a plane row, and partial-line writes to these planes cost a factor of 2.4 (profiles/r03_plane_skew.txt).
// So a workgroup owns OUTPUT: YUVD_SPAN bytes from a multiple of YUVD_SPAN (of 128: the pitch is one too, every cache line leaves whole) of
// the 2 · YUVD_ROWS plane rows of YUVD_ROWS block rows, of the three planes of one image.
//   1. It computes the blocks that cover the span's pixels clamp(j − first, 0, W − 1): at most YUVD_SPAN / 8 + 1 per block row — the one
//      block that straddles a span boundary is computed by both neighbours; a span that lies in the padding computes the edge block alone.
//      A lane takes one block (lane → (block row, block): 5 · 49 = 245 of 256 lanes at work).
//   2. The lane puts its 8 bytes per (row, channel) into LDS as two dwords, pixel x of the span's first block bx_lo at byte
//      x − 8·bx_lo + off of its LDS row.  off ∈ {0, 4, 8, 12} is chosen per workgroup so that the bytes of every 16-byte-aligned OUTPUT piece
//      begin t = (−s) mod 4 bytes into a 16-byte-aligned LDS piece (s = first + 8·bx_lo − j0, the span-relative output byte of LDS pixel 0).
//   3. After the barrier a lane takes 16-byte output pieces (neighbouring lanes neighbouring pieces of one plane row: 24 lanes store three
//      whole lines): a piece inside the image is one ds_read_b128 and one ds_read_b32 funnelled by t bytes (v_alignbyte_b32); a piece that
//      touches the padding picks its 16 bytes one by one at the clamped pixel.  One 16-byte global store per piece.
// No atomics, no read of the destination, no store outside [0, pitch) of the rows the context holds: pieces at or beyond the pitch (a
// multiple of 16), rows beyond H (an odd H's last block row) and block rows beyond ch are skipped.  W < 8 and ragged last blocks need no
// path of their own: bytes of columns beyond W − 1 are in LDS and never picked (a piece inside the image ends at or before W − 1).
//
// Left-sited chroma (lfi_set_yuv_siting): yuvs_derived_expand_left<FORMAT>, a kernel of its own name (tests pin the four bodies of
// yuvs_derived_expand) with the same body, yuvs_derived_spans — only step 1's pixels differ: yuvs_block_pixels<FORMAT, false, true>, one
// chroma load fewer per row and plane.  NEAREST is the same bytes under either siting and launches yuvs_derived_expand<FORMAT, true>.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../../include/lfi.h"
#include "yuv_surfaces.hpp"

namespace lfi {

constexpr int YUVD_SPAN = 384;                                // output bytes (= pixels) of a plane row per workgroup: LFI_YUV_DERIVED_SPAN
constexpr int YUVD_ROWS = 5;                                  // block rows per workgroup
constexpr int YUVD_NB = YUVD_SPAN / YUV_BLOCK_W + 1;          // blocks that can cover a span
constexpr int YUVD_THREADS = 256;
constexpr int YUVD_LDS_PITCH = (YUVD_NB * YUV_BLOCK_W + 12 + 20 + 15) / 16 * 16; // blocks + the largest off + a funnelled read's reach
constexpr int YUVD_PIECES_X = YUVD_SPAN / 16;
constexpr int YUVD_PIECES = YUVD_ROWS * 2 * 3 * YUVD_PIECES_X;
static_assert(YUVD_SPAN == LFI_YUV_DERIVED_SPAN, "include/lfi.h names the span");
static_assert(YUVD_SPAN % 128 == 0 && YUVD_ROWS * YUVD_NB <= YUVD_THREADS, "a lane per block, whole cache lines per span");

struct YuvsDerivedArgs
{
    YuvsInArgs in;        // the frames, as yuvs_expand takes them (dst, image_stride and rows16 are not used)
    uint8_t *planar;      // the derived copy: [N][3][H][pitch]
    const int32_t *phase; // [N]: the copy's per-image phases (device)
    uint32_t pitch, padx; // bytes per plane row (a multiple of 16), left padding
    uint32_t g0;          // frame z is image g0 + z
};

// The whole kernel, for any source of an image's pixels — a policy whose members inline:
//   src.image()    the index in the copy of the image that grid.z stands for (wave-uniform)
//   Source::ASSEMBLED = false: step 1 is yuvs_block_pixels itself, on src.args() and src.frame(), the image taken as a frame of its own
//   Source::ASSEMBLED = true:  step 1 is src.template block_pixels<FORMAT, NEAREST, LEFT>(bx, by, px), which gives the same pixels by other loads
// a.in.W, H and ch are the image's.  LEFT: left-sited chroma (yuvs_block_pixels' filter).  Steps 2 and 3, the staging and the stores, are the
// same for every source: the frame kernels below and the mosaic kernels of yuv_mosaic_derived.hpp.  The call of yuvs_block_pixels stands here,
// not behind a member of the source, so that the frame kernels keep the instructions they had (profiles/r26_mosaic_derived_notes.md)
template <int FORMAT, bool NEAREST, bool LEFT, class Source>
__device__ __forceinline__ void yuvs_derived_spans(const YuvsDerivedArgs &a, const Source &src)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[YUVD_ROWS][2][3][YUVD_LDS_PITCH];
    const uint32_t tid = threadIdx.x;
    const uint32_t g = src.image();
    const int32_t W = (int32_t)a.in.W;
    const int32_t first = (int32_t)a.padx + a.phase[g]; // byte of pixel 0
    const int32_t j0 = (int32_t)(blockIdx.x * YUVD_SPAN);
    // the span's pixels, and the blocks that hold them
    const int32_t lo = min(max(j0 - first, 0), W - 1), hi = min(max(j0 + YUVD_SPAN - 1 - first, 0), W - 1);
    const uint32_t bx_lo = (uint32_t)lo / YUV_BLOCK_W, nb = (uint32_t)hi / YUV_BLOCK_W - bx_lo + 1u; // nb ≤ YUVD_NB
    const int32_t s = first + (int32_t)(bx_lo * YUV_BLOCK_W) - j0;
    const uint32_t t = (uint32_t)(-s) & 3u, off = (uint32_t)(s + (int32_t)t) & 15u; // off a multiple of 4
    {
        const uint32_t r = tid / YUVD_NB, b = tid % YUVD_NB;
        const uint32_t by = blockIdx.y * YUVD_ROWS + r;
        if(r < (uint32_t)YUVD_ROWS && b < nb && by < a.in.ch)
        {
            uint32_t px[2][8];
            if constexpr(Source::ASSEMBLED)
                src.template block_pixels<FORMAT, NEAREST, LEFT>(bx_lo + b, by, px);
            else
                yuvs_block_pixels<FORMAT, NEAREST, LEFT>(src.args(), src.frame(), bx_lo + b, by, px);
#pragma unroll
            for(int j = 0; j < 2; j++)
#pragma unroll
                for(int c = 0; c < 3; c++)
                {
                    uint32_t *dst = reinterpret_cast<uint32_t *>(&lds[r][j][c][b * YUV_BLOCK_W + off]);
                    const uint32_t sel = 0x0c0c0400u + 0x0101u * uint32_t(c); // [lo.c, hi.c, 0, 0]
                    dst[0] = __builtin_amdgcn_perm(px[j][1], px[j][0], sel) | (__builtin_amdgcn_perm(px[j][3], px[j][2], sel) << 16);
                    dst[1] = __builtin_amdgcn_perm(px[j][5], px[j][4], sel) | (__builtin_amdgcn_perm(px[j][7], px[j][6], sel) << 16);
                }
        }
    }
    __syncthreads();
    for(uint32_t p = tid; p < (uint32_t)YUVD_PIECES; p += YUVD_THREADS)
    {
        const uint32_t k = p % YUVD_PIECES_X, rc = p / YUVD_PIECES_X; // rc = (r · 2 + j) · 3 + c
        const uint32_t c = rc % 3u, j = (rc / 3u) & 1u, r = rc / 6u;
        const uint32_t by = blockIdx.y * YUVD_ROWS + r, y = by * YUV_BLOCK_H + j;
        const int32_t q = (int32_t)(16u * k), jj = j0 + q;
        if(by >= a.in.ch || y >= a.in.H || (uint32_t)jj >= a.pitch)
            continue;
        const uint8_t *row = lds[r][j][c];
        const int32_t x = jj - first; // the pixel of the piece's byte 0, before the clamp
        uint4 out;
        if(x >= 0 && x + 15 <= W - 1)
        {
            const uint32_t al = (uint32_t)(q - s) + off - t; // a multiple of 16, ≥ 0: x ≥ lo ≥ 8·bx_lo
            const uint4 d = *reinterpret_cast<const uint4 *>(row + al);
            const uint32_t e = *reinterpret_cast<const uint32_t *>(row + al + 16u);
            out = uint4{__builtin_amdgcn_alignbyte(d.y, d.x, t), __builtin_amdgcn_alignbyte(d.z, d.y, t), __builtin_amdgcn_alignbyte(d.w, d.z, t),
                        __builtin_amdgcn_alignbyte(e, d.w, t)};
        }
        else
        {
            // the clamped pixels lie in [lo, hi]: inside the span's blocks
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            const int32_t base = (int32_t)off - (int32_t)(bx_lo * YUV_BLOCK_W);
#pragma unroll
            for(int i = 0; i < 16; i++)
                w[i >> 2] |= (uint32_t)row[min(max(x + i, 0), W - 1) + base] << (8 * (i & 3));
            out = uint4{w[0], w[1], w[2], w[3]};
        }
        *reinterpret_cast<uint4 *>(a.planar + (((size_t)g * 3u + c) * a.in.H + y) * a.pitch + (uint32_t)jj) = out;
    }
}

// the pixel source of the frame kernels: frame grid.z of a.in.s is image a.g0 + grid.z
struct YuvsFrameSource
{
    static constexpr bool ASSEMBLED = false;
    const YuvsDerivedArgs &a;
    __device__ __forceinline__ uint32_t image() const { return a.g0 + blockIdx.z; }
    __device__ __forceinline__ const YuvsInArgs &args() const { return a.in; }
    __device__ __forceinline__ const uint8_t *frame() const { return a.in.s.base + (size_t)blockIdx.z * a.in.s.frame_stride; }
};

template <int FORMAT, bool NEAREST>
__global__ void __launch_bounds__(YUVD_THREADS) yuvs_derived_expand(const YuvsDerivedArgs a)
{
    yuvs_derived_spans<FORMAT, NEAREST, false>(a, YuvsFrameSource{a});
}

// left-sited chroma, BILINEAR (NEAREST is yuvs_derived_expand's under either siting)
template <int FORMAT>
__global__ void __launch_bounds__(YUVD_THREADS) yuvs_derived_expand_left(const YuvsDerivedArgs a)
{
    yuvs_derived_spans<FORMAT, false, true>(a, YuvsFrameSource{a});
}

// Enqueues the ONE yuvs_derived_expand launch for n frames.  The caller has checked sizes, alignment and memory as for launch_yuvs_expand;
// a.planar holds images [g0, g0 + n) with a.in.H rows of a.pitch bytes per plane, a.pitch a multiple of 16.
inline hipError_t launch_yuvs_derived_expand(hipStream_t stream, const int format, const bool nearest, const bool left, const YuvsDerivedArgs &a,
                                             const int n)
{
    const dim3 grid((a.pitch + YUVD_SPAN - 1) / YUVD_SPAN, (a.in.ch + YUVD_ROWS - 1) / YUVD_ROWS, n), block(YUVD_THREADS);
    if(left && !nearest)
    {
        if(format == YUVS_NV12)
            hipLaunchKernelGGL((yuvs_derived_expand_left<YUVS_NV12>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((yuvs_derived_expand_left<YUVS_I420>), grid, block, 0, stream, a);
    }
    else if(format == YUVS_NV12)
    {
        if(nearest)
            hipLaunchKernelGGL((yuvs_derived_expand<YUVS_NV12, true>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((yuvs_derived_expand<YUVS_NV12, false>), grid, block, 0, stream, a);
    }
    else
    {
        if(nearest)
            hipLaunchKernelGGL((yuvs_derived_expand<YUVS_I420, true>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((yuvs_derived_expand<YUVS_I420, false>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

} // namespace lfi
