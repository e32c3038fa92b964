/* cuda_fp16.h — the half type as far as the reference's src/kernels.cu uses it, over the compiler's _Float16.
 * TEST INFRASTRUCTURE ONLY; every line is this project's (see ref_cuda.h). */
#ifndef REF_SHIM_CUDA_FP16_H
#define REF_SHIM_CUDA_FP16_H

#include "ref_cuda.h"

struct half
{
    _Float16 value;

    half() = default;
    /* CUDA Math API, __float2half: "converts float number to half precision in round-to-nearest-even mode" — what the
     * float → _Float16 conversion does (IEEE binary16, default rounding mode) */
    half(float f) : value(static_cast<_Float16>(f)) {}
    /* integers up to 2048 are exact in binary16; the kernels convert bytes */
    half(unsigned char b) : value(static_cast<_Float16>(static_cast<int>(b))) {}
    half(int i) : value(static_cast<_Float16>(i)) {}

    /* half → float is exact */
    operator float() const { return static_cast<float>(value); }
    /* CUDA Math API, __half2uchar_rz (the conversion operator of __half): "convert a half to an unsigned char in
     * round-towards-zero mode"; PTX cvt to an integer type clamps out-of-range values to the destination's range and
     * converts NaN to 0 */
    operator unsigned char() const
    {
        float f = static_cast<float>(value);
        if(!(f > 0.0f))
            return 0;
        if(f >= 255.0f)
            return 255;
        return static_cast<unsigned char>(static_cast<int>(f));
    }
};

struct half2 { half x, y; };

static_assert(sizeof(half) == 2 && sizeof(half2) == 4, "half is two bytes");

#endif
