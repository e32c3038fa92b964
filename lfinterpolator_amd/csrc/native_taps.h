// native_taps.h — the tap arithmetic of the bilinear tile sampling of lfi_download_native (LFI_LENT_BILINEAR, include/lfi.h): ONE copy,
// compiled into the device code (hip/native_filter.hpp) and into the host library (lfi_host_native_taps, host/host_capi.cpp), so that the
// kernel and the tests work from the same taps.
//
// One axis of `src` tile pixels is sampled at the centres of `dst` output pixels, pixel centres at +½ on both sides.  With D = 2·dst,
//     U  = clamp((2·o + 1)·src − dst, 0, (src − 1)·D)      (the first term signed before the clamp)
//     p0 = U / D,  f = (256·(U − p0·D)) / D ∈ [0, 255],  p1 = min(p0 + 1, src − 1)
// In 32 bits: (2·o + 1)·src reaches 2³³, so with q, r = quotient and remainder of o·src by dst (o·src < 65535²)
//     (2·o + 1)·src − dst + D = D·q + e,   e = 2·r + src + dst < 3·dst + src < 4·65535
// and with qe, re = quotient and remainder of e by D the unclamped U is D·(q + qe − 1) + re: q + qe = 0 is the lower clamp (U < 0), a
// quotient of src − 1 or more the upper one, and 256·re < 2²⁵.  Every intermediate stays below 2³² for 1 ≤ src, dst ≤ 65535, o < dst.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LFI_NATIVE_TAPS_FN __host__ __device__ __forceinline__
#else
#define LFI_NATIVE_TAPS_FN inline
#endif

namespace lfi {

struct NativeTaps
{
    uint32_t p0, p1; // the two tile pixels, p0 ≤ p1 ≤ src − 1
    uint32_t f;      // the weight of p1 in 1/256; p0 weighs 256 − f
};

LFI_NATIVE_TAPS_FN NativeTaps native_taps(const uint32_t o, const uint32_t src, const uint32_t dst)
{
    const uint32_t D = 2u * dst, num = o * src, q = num / dst, r = num - q * dst;
    const uint32_t e = 2u * r + src + dst, qe = e / D, re = e - qe * D;
    const uint32_t above = q + qe; // p0 + 1 before the clamps
    NativeTaps t;
    t.p0 = above ? above - 1u : 0u;
    t.f = above ? (256u * re) / D : 0u;
    if(t.p0 >= src - 1u)
    {
        t.p0 = src - 1u;
        t.f = 0u;
    }
    t.p1 = t.p0 + 1u < src ? t.p0 + 1u : src - 1u;
    return t;
}

} // namespace lfi
