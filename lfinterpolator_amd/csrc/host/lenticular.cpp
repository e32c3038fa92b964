// lenticular.cpp — see lenticular.h.  The order of the operations below is part of the definition (tests/native_ref.py restates it).
#include "lenticular.h"

#include <cmath>
#include <stdexcept>

namespace lfi {

namespace {

// round to the nearest integer, ties away from zero, reduced mod 2³² (a negative value wraps)
uint32_t roundToPhase(double v)
{
    const double mag = v < 0.0 ? -v : v;
    if(!(mag < 4503599627370496.0)) // 2⁵²: below it mag + ½ is exact
        throw std::runtime_error("The lens calibration gives a phase step beyond 2^52 units!");
    const int64_t r = static_cast<int64_t>(mag + 0.5);
    return static_cast<uint32_t>(static_cast<uint64_t>(v < 0.0 ? -r : r));
}

} // namespace

lfi_lenticular lenticularFromCalibration(const LensCalibration &c, int out_w, int out_h, int n)
{
    if(!(c.pitch > 0.0) || !(c.dpi > 0.0) || !std::isfinite(c.pitch) || !std::isfinite(c.dpi) || !std::isfinite(c.slope) || c.slope == 0.0 ||
       !std::isfinite(c.center))
        throw std::runtime_error("A lens calibration needs pitch > 0, dpi > 0, a slope other than 0 and a finite center!");
    if(out_w < 1 || out_h < 1 || n < 1)
        throw std::runtime_error("A lens calibration needs an output of at least 1x1 pixels and at least one view!");
    const double w = out_w, h = out_h, two32 = 4294967296.0;
    const double absSlope = c.slope < 0.0 ? -c.slope : c.slope;
    const double p = ((c.pitch * w) / c.dpi) * (absSlope / std::sqrt(c.slope * c.slope + 1.0));
    const double tilt = h / (w * c.slope);
    lfi_lenticular lens{};
    lens.x_step = roundToPhase((two32 * p) / (3.0 * w));
    lens.y_step = roundToPhase(((two32 * p) * tilt) / h);
    lens.phase0 = roundToPhase(two32 * (p * (0.5 / w + (0.5 * tilt) / h) - c.center));
    lens.views = n;
    lens.flags = c.invert ? LFI_LENT_INVERT : 0u;
    return lens;
}

} // namespace lfi
