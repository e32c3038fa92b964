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
//
// A calibration FILE (lensCalibrationFromJson) is the flat JSON object such displays report about themselves: every numeric entry is either
// "name": {"value": x} or "name": x.  Taken: pitch, slope, center, DPI, invView (non-zero: reversed view order, LFI_LENT_INVERT), flipSubp
// (non-zero: the subpixels run B, G, R — LFI_LENT_BGR), screenW and screenH (the panel's size, for the caller to compare with its own).
// flipImageX / flipImageY non-zero are refused: mirrored panels are not built.  Strings, other keys and whatever they hold are skipped; the
// order of the keys does not matter; a key given twice counts as its last entry.  Errors name the key.
#pragma once

#include <string>

#include "../../../include/lfi.h"

namespace lfi {

struct LensCalibration
{
    double pitch = 0, slope = 0, center = 0, dpi = 0;
    bool invert = false;
};

// throws std::runtime_error unless pitch, dpi > 0, slope ≠ 0, all finite, out_w, out_h, n ≥ 1 and every rounded value is below 2⁵² in magnitude
lfi_lenticular lenticularFromCalibration(const LensCalibration &c, int out_w, int out_h, int n);

// a calibration file's content: the calibration, LFI_LENT_BGR or 0, and the panel's size (0: not stated)
struct LensFile
{
    LensCalibration lens;
    uint32_t flags = 0;
    int screenW = 0, screenH = 0;
};

// throws std::runtime_error for text that is no JSON object, a taken key without a number, a missing pitch, slope, center or DPI, and a mirrored panel
LensFile lensCalibrationFromJson(const std::string &text);
// … of the file at path; throws also when it cannot be read
LensFile lensCalibrationFromFile(const std::string &path);

} // namespace lfi
