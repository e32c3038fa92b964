// lenticular.h — a lenticular display's calibration turned into the fixed-point lens description of lfi_download_native (include/lfi.h).
//
// A Looking-Glass-type calibration gives the lens sheet as pitch (lenses per inch, measured along the panel's x axis before the slant is
// taken into account), slope (the slant: pixels of height per pixel of width the lens edge runs), center (the phase offset, in lens
// periods) and the panel's dpi.  With pixel centres at (x + ½) / out_w and (y + ½) / out_h, origin top-left, the usual shader computes per
// subpixel  fract((u + v·tilt)·p − center)  with u advanced by a third of a pixel per subpixel; here the same quantities become three u32
// in units of 2⁻³² lens periods, so that the device side is pure integer arithmetic and byte-exact:
//     p      = pitch · out_w / dpi · |slope| / sqrt(slope² + 1)          (lens periods across the width; cos(atan(1 / slope)) without libm)
//     tilt   = out_h / (out_w · slope)
//     x_step = round(2³² · p / (3 · out_w))
//     y_step = round(2³² · p · tilt / out_h)
//     phase0 = round(2³² · (p · (½ / out_w + ½ · tilt / out_h) − center))
// each reduced mod 2³² (negative values wrap: two's complement), ties rounded away from zero.  Everything is evaluated in doubles with
// +, −, ×, ÷ and sqrt only, in exactly the order written in lenticular.cpp, and this file is built with -ffp-contract=off: a restatement
// in any IEEE-754 double arithmetic (tests/native_ref.py in Python floats) gives the same bits.
//
// Accuracy: a step is off by at most half a unit, 2⁻³³ of a lens period; along a row of 7680 pixels the phase adds x_step 3 · 7680 =
// 23040 < 2¹⁵ times, so the accumulated error stays under 2⁻¹⁸ of a lens period — with n views a view is 1 / n of a period wide, so far
// below one view for any n a display has.
#pragma once

#include "../../../include/lfi.h"

namespace lfi {

struct LensCalibration
{
    double pitch = 0, slope = 0, center = 0, dpi = 0;
    bool invert = false;
};

// throws std::runtime_error unless pitch, dpi > 0, slope ≠ 0, all finite, out_w, out_h, n ≥ 1 and every rounded value is below 2⁵² in magnitude
lfi_lenticular lenticularFromCalibration(const LensCalibration &c, int out_w, int out_h, int n);

} // namespace lfi
