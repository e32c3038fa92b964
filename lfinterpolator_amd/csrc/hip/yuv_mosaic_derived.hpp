// yuv_mosaic_derived.hpp — ONE YUV 4:2:0 frame that holds a whole grid of images, split straight into the derived planar copy of the inputs
// (DESIGN.md §4.24): the kernels behind lfi_upload_mosaic_yuv_derived.  A context that holds only that copy (lfi_release_inputs) takes a
// camera-array mosaic's next time step in one pass.  No new arithmetic and no new data movement: the two halves exist and are joined here.
//   - The load side is yuv_mosaic.hpp's.  grid.z is the call's tile k; mosaic_tile gives the wave-uniform (tx, ty, g).  A lane's block of
//     8 × 2 pixels comes from the tile: UNALIGNED = false (W a multiple of 8) through yuvs_block_pixels unchanged on the per-tile copy of the
//     arguments (yuvs_mosaic_tile_frame); UNALIGNED = true through yuvs_mosaic_block_pixels, pieces assembled from covering aligned dwords,
//     none loaded beyond the pitch of its own plane row, no misaligned pointer dereferenced.  Both proofs are that header's and hold here
//     word for word: the blocks asked for are blocks of the tile (bx ≤ (W − 1) / 8 — yuvs_derived_spans clamps the span's pixels to
//     [0, W − 1] — and by < ch).
//   - The store side is yuv_derived.hpp's yuvs_derived_spans, called with the tile's pixel source and the image g: a workgroup owns
//     YUVD_SPAN output bytes of the 2 · YUVD_ROWS plane rows of the three planes of image g, stages the blocks' bytes in LDS at their output
//     position and stores 16-byte pieces.  g — not g0 + grid.z — indexes phase[] and the planes: under LFI_MOSAIC_GRID g = tx·rows + r is not
//     contiguous.  No atomics, no read of the destination, no store outside [0, pitch) of the rows of image g.
// Staged chunks hold some tile rows only: ty_bias is the frame's tile row that is tile row 0 of the staged planes, as in YuvsMosaicArgs.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "yuv_derived.hpp"
#include "yuv_mosaic.hpp"

namespace lfi {

struct YuvsMosaicDerivedArgs
{
    YuvsDerivedArgs d; // in.s: the FRAME's surfaces (or the staged tile rows); in.W, H, cw, ch, blocks_x: a TILE's; the copy; g0 is not used
    MosaicMap map;
    uint32_t k0;      // the launch's first tile: tile k0 + grid.z
    uint32_t ty_bias; // the frame's tile row that is tile row 0 of in.s (in place: 0)
};

// the pixel sources (yuvs_derived_spans' policy) for tile k0 + grid.z, image g
// W a multiple of 8: the tile as a frame of its own — yuvs_block_pixels on the patched copy of the arguments
struct YuvsMosaicTileSource
{
    static constexpr bool ASSEMBLED = false;
    YuvsInArgs t;         // yuvs_mosaic_tile_frame's copy
    const uint8_t *origin; // the tile's Y origin
    uint32_t g;
    __device__ __forceinline__ uint32_t image() const { return g; }
    __device__ __forceinline__ const YuvsInArgs &args() const { return t; }
    __device__ __forceinline__ const uint8_t *frame() const { return origin; }
};

// every other even W: the tile's blocks assembled from covering aligned dwords — yuvs_mosaic_block_pixels at the tile's Y origin (ox, oy)
struct YuvsMosaicAssembledSource
{
    static constexpr bool ASSEMBLED = true;
    const YuvsInArgs &in;
    uint32_t ox, oy, g;
    __device__ __forceinline__ uint32_t image() const { return g; }
    template <int FORMAT, bool NEAREST, bool LEFT>
    __device__ __forceinline__ void block_pixels(const uint32_t bx, const uint32_t by, uint32_t (&px)[2][8]) const
    {
        yuvs_mosaic_block_pixels<FORMAT, NEAREST, LEFT>(in, ox, oy, bx, by, px);
    }
};

template <int FORMAT, bool NEAREST, bool LEFT, bool UNALIGNED>
__device__ __forceinline__ void yuvs_mosaic_derived_spans(const YuvsMosaicDerivedArgs &a)
{
    uint32_t tx, ty, g; // wave-uniform
    mosaic_tile(a.map, a.k0 + blockIdx.z, tx, ty, g);
    const uint32_t ox = tx * a.d.in.W, oy = (ty - a.ty_bias) * a.d.in.H; // the tile's Y origin: column and row of the frame a.d.in.s
    if constexpr(UNALIGNED)
        yuvs_derived_spans<FORMAT, NEAREST, LEFT>(a.d, YuvsMosaicAssembledSource{a.d.in, ox, oy, g});
    else
    {
        YuvsMosaicTileSource src{a.d.in, nullptr, g};
        src.origin = yuvs_mosaic_tile_frame<FORMAT>(a.d.in, ox, oy, src.t);
        yuvs_derived_spans<FORMAT, NEAREST, LEFT>(a.d, src);
    }
}

template <int FORMAT, bool NEAREST, bool UNALIGNED>
__global__ void __launch_bounds__(YUVD_THREADS) yuvs_mosaic_derived_expand(const YuvsMosaicDerivedArgs a)
{
    yuvs_mosaic_derived_spans<FORMAT, NEAREST, false, UNALIGNED>(a);
}

// left-sited chroma, BILINEAR (NEAREST is yuvs_mosaic_derived_expand's under either siting)
template <int FORMAT, bool UNALIGNED>
__global__ void __launch_bounds__(YUVD_THREADS) yuvs_mosaic_derived_expand_left(const YuvsMosaicDerivedArgs a)
{
    yuvs_mosaic_derived_spans<FORMAT, false, true, UNALIGNED>(a);
}

// Enqueues the ONE launch for n tiles from a.k0 on.  The caller has checked the map, sizes, alignment and memory: a.d.in.s holds the tile rows
// the n tiles lie in, a.d.planar every image the map names with a.d.in.H rows of a.d.pitch bytes per plane, a.d.pitch a multiple of 16.
// unaligned: the tile width is no multiple of 8
inline hipError_t launch_yuvs_mosaic_derived_expand(hipStream_t stream, const int format, const bool nearest, const bool left, const bool unaligned,
                                                    const YuvsMosaicDerivedArgs &a, const int n)
{
    const dim3 grid((a.d.pitch + YUVD_SPAN - 1) / YUVD_SPAN, (a.d.in.ch + YUVD_ROWS - 1) / YUVD_ROWS, n), block(YUVD_THREADS);
    // KERNEL<…, UNALIGNED>: the two instantiations of one kernel that differ in the last template argument
#define LFI_MOSAIC_DERIVED_LAUNCH(...)                                                \
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
            LFI_MOSAIC_DERIVED_LAUNCH(yuvs_mosaic_derived_expand_left < YUVS_NV12);
        else
            LFI_MOSAIC_DERIVED_LAUNCH(yuvs_mosaic_derived_expand_left < YUVS_I420);
    }
    else if(format == YUVS_NV12)
    {
        if(nearest)
            LFI_MOSAIC_DERIVED_LAUNCH(yuvs_mosaic_derived_expand < YUVS_NV12, true);
        else
            LFI_MOSAIC_DERIVED_LAUNCH(yuvs_mosaic_derived_expand < YUVS_NV12, false);
    }
    else
    {
        if(nearest)
            LFI_MOSAIC_DERIVED_LAUNCH(yuvs_mosaic_derived_expand < YUVS_I420, true);
        else
            LFI_MOSAIC_DERIVED_LAUNCH(yuvs_mosaic_derived_expand < YUVS_I420, false);
    }
#undef LFI_MOSAIC_DERIVED_LAUNCH
    return hipGetLastError();
}

} // namespace lfi
