// params.h — host parameterisation of the shift-and-sum kernels: everything the reference's Interpolator computes on
// the CPU before a launch (reference src/interpolator.cu:139-246, 318-337), kept above the C-ABI so that every consumer
// of include/lfi.h is handed identical bytes.
#pragma once

#include <cstdint>
#include <string>
#include <array>
#include <vector>

#include "../../../include/lfi.h"
#include "vec.h"

namespace lfi {

// IEEE binary16 bit pattern of a float, round-to-nearest-even: static_cast<half>(float) on the host
// (reference src/interpolator.cu:219)
uint16_t floatToHalfBits(float value);
float halfBitsToFloat(uint16_t bits);

// The reference's per-launch parameter block (its __constant__ symbols + the weight matrix), owned by value.
struct HostParams
{
    int views{LFI_REFERENCE_VIEWS};
    std::vector<lfi_int2> focusedOffsets;   // [N]
    std::vector<lfi_float2> offsets;        // [N]
    std::vector<uint16_t> weights;          // [views][N] fp16 bits
    std::vector<int32_t> focusMapIDs;       // ≤ 32
    float focus{0}, range{0};
    int blockRadius[2]{1, 1};
    uint32_t flags{0};

    // view of this block for lfi_set_params; valid while *this is alive and unmodified
    lfi_params abi() const;
};

class Parameterizer
{
    public:
        Parameterizer(IVec2 colsRows, IVec3 resolution) : colsRows{colsRows}, resolution{resolution} {}

        // "startCol,startRow,endCol,endRow" in normalised grid coordinates → absolute grid coordinates
        Vec4 interpretTrajectory(const std::string &trajectory) const;
        std::vector<Vec2> generateTrajectory(Vec4 startEndPoints, int views) const;
        std::vector<float> generateWeights(Vec2 coords, float effect) const;
        std::vector<uint16_t> weightMatrix(Vec4 startEndPoints, float effect, int views) const;
        void offsets(float aspect, float focus, Vec4 startEndPoints, std::vector<lfi_float2> &offsets,
                     std::vector<lfi_int2> &focusedOffsets) const;
        // per-view focus (lfi_set_view_offsets): [views][N] integer offsets, row v = offsets(aspect, focus[v], …)'s focused offsets
        std::vector<lfi_int2> viewOffsets(float aspect, const std::vector<float> &focus, Vec4 startEndPoints) const;
        // each view shifted about its own camera (lfi_set_view_float_offsets / lfi_set_view_offsets): row v of offsets [views][N] and
        // focused [views][N] is offsets(aspect, focus[v], {cam_v, cam_v}) for camera v of generateTrajectory(startEndPoints, views) — the
        // trajectory collapsed onto that camera, whose centre is the camera itself
        void viewCentredOffsets(float aspect, const std::vector<float> &focus, Vec4 startEndPoints, std::vector<lfi_float2> &offsets,
                                std::vector<lfi_int2> &focused) const;
        std::vector<int32_t> selectFocusMapViews(Vec4 startEndPoints) const;
        // each view's focus-map images: row v of [views][min(32, N)] = selectFocusMapViews of the trajectory collapsed onto camera v
        std::vector<int32_t> viewFocusMapIDs(Vec4 startEndPoints, int views) const;
        IVec2 blockRadius() const;

        // everything at once: what Interpolator::interpolate prepares before its launches
        HostParams build(const std::string &trajectory, float focus, float range, float effect, float aspect,
                         int views = LFI_REFERENCE_VIEWS) const;

    private:
        IVec2 colsRows;
        IVec3 resolution;
};

Vec2 trajectoryCenter(Vec4 startEndPoints);

// views focus values from f0 to f1, equally spaced: f0 + ((f1 − f0) / (views − 1))·i in float — the rounding of generateTrajectory; one
// view gets f0
std::vector<float> focusRamp(float f0, float f1, int views);
// The focus candidates of lfi_focus_curve (for 32 steps: of FocusMap::estimate, reference src/kernels.cu:245-250), steps ≥ 2:
// f_i = fmaf(range / (steps − 1), i, focus) in float — the device's arithmetic, so that nobody recomputes them with other rounding
std::vector<float> focusCandidates(float focus, float range, int steps);
// Tile (tx, ty) of lfi_focus_tiles' tilesX × tilesY grid over a width × height frame: {x0, y0, x1, y1} with x0 = tx·width / tilesX,
// x1 = (tx + 1)·width / tilesX (integer divisions of 64-bit products), likewise in y — the tiles cover the frame exactly once
std::array<int, 4> focusTileRect(int width, int height, int tilesX, int tilesY, int tx, int ty);
// The search interval an all-focus render needs, from the tiles' best candidates of a search over [focus, focus + range] with `steps`
// candidates (lfi_focus_tiles: 32; lfi_focus_tiles_steps): lo / hi = the smallest / largest index, widened by one candidate on either side
// inside [0, steps − 1]; the values are focusCandidates(focus, range, steps)'
struct FocusAutoRange
{
    int lo, hi;   // the candidates kept: max(lo − 1, 0), min(hi + 1, steps − 1)
    float focus;  // candidate lo
    float range;  // candidate hi − candidate lo in float: always > 0
};
FocusAutoRange focusAutoRange(const int32_t *bestIndex, size_t tiles, float focus, float range, int steps = LFI_FOCUS_TILE_STEPS);

} // namespace lfi
