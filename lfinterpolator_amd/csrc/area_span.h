// area_span.h — the span arithmetic of the area resize (lfi_download_quilt_scaled): ONE copy, compiled into the device code
// (hip/quilt_scaled.hpp) and into the host library (lfi_host_area_span, host/host_capi.cpp), so that the kernel and the tests work from the
// same spans.
//
// One axis of `src` source pixels becomes `dst` output pixels, 1 ≤ dst ≤ src.  Both lie on a grid of src·dst units: output pixel o covers
// [o·src, (o + 1)·src), source pixel s covers [s·dst, (s + 1)·dst).  The weight of s in o is the length of the overlap — an integer; over s
// the weights of one output sum to src.  The sources with a non-empty overlap are first … last; every source strictly between them lies
// inside the output pixel and weighs dst; first and last weigh their partial overlaps (first = last only where dst = src: both weights = src).
//
// All products stay below src² in uint32_t: src ≤ LFI_AREA_SPAN_MAX.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LFI_AREA_SPAN_FN __host__ __device__ __forceinline__
#else
#define LFI_AREA_SPAN_FN inline
#endif

namespace lfi {

constexpr uint32_t LFI_AREA_SPAN_MAX = 65535u;

struct AreaSpan
{
    uint32_t first, last;     // the source pixels output o overlaps
    uint32_t w_first, w_last; // the overlaps with first and last
};

LFI_AREA_SPAN_FN AreaSpan area_span(const uint32_t src, const uint32_t dst, const uint32_t o)
{
    const uint32_t lo = o * src, hi = lo + src;
    AreaSpan s;
    s.first = lo / dst;
    s.last = (hi - 1u) / dst;
    const uint32_t first_end = (s.first + 1u) * dst, last_begin = s.last * dst;
    s.w_first = (first_end < hi ? first_end : hi) - lo;
    s.w_last = hi - (last_begin > lo ? last_begin : lo);
    return s;
}

// the weight of source pixel s (first ≤ s ≤ last) in the output pixel the span belongs to
LFI_AREA_SPAN_FN uint32_t area_weight(const AreaSpan &a, const uint32_t dst, const uint32_t s)
{
    return s == a.first ? a.w_first : s == a.last ? a.w_last : dst;
}

} // namespace lfi
