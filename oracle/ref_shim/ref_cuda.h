/* ref_cuda.h — the part of the CUDA device language that the reference's src/kernels.cu uses, restated for a CPU build.
 *
 * TEST INFRASTRUCTURE ONLY.  Every line here is this project's; the reference's kernels are reached at build time through
 * the include path alone (oracle/Makefile, -I$(REF)/src) and nothing of them is copied.  oracle/ref_kernels.cpp states the
 * execution model (one OS thread per CUDA thread, blocks one after another); this header holds what a kernel sees of it.
 *
 * Each semantic below names the wording of NVIDIA's CUDA C++ Programming Guide / CUDA Math API / PTX ISA that it follows.
 */
#ifndef REF_SHIM_REF_CUDA_H
#define REF_SHIM_REF_CUDA_H

#include <cfloat>
#include <climits>
#include <cmath>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <math.h> /* brings the float overloads (round, …) into the global namespace, where CUDA has them */
#include <mutex>
#include <type_traits>

/* function and variable space qualifiers mean nothing on the host */
#define __device__
#define __global__
#define __constant__
#define __shared__

/* built-in vector types (Programming Guide, "Built-in Vector Types"): plain aggregates.  Their CUDA alignment (int4: 16)
 * is not modelled: the kernels cast differently aligned local arrays to int4 *, which only an unaligned type reads safely. */
struct int2 { int x, y; };
struct int4 { int x, y, z, w; };
struct uint3 { unsigned x, y, z; };
struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct alignas(4) uchar4 { unsigned char x, y, z, w; };
typedef uint3 dim3;

namespace ref_shim
{
/* A barrier whose party can shrink: a CUDA thread that returns from its kernel no longer takes part ("drop"). */
class Barrier
{
    std::mutex m;
    std::condition_variable cv;
    int expected{0}, waiting{0};
    unsigned generation{0};

  public:
    void reset(int parties)
    {
        expected = parties;
        waiting = 0;
    }
    void wait()
    {
        std::unique_lock<std::mutex> lock(m);
        unsigned g = generation;
        if(++waiting == expected)
        {
            waiting = 0;
            generation++;
            cv.notify_all();
        }
        else
            cv.wait(lock, [&] { return generation != g; });
    }
    void drop()
    {
        std::lock_guard<std::mutex> lock(m);
        expected--;
        if(expected > 0 && waiting == expected)
        {
            waiting = 0;
            generation++;
            cv.notify_all();
        }
    }
};

constexpr int WARP = 32;
constexpr int MAX_BLOCK_THREADS = 256;
inline Barrier blockBarrier;
inline Barrier warpBarrier[MAX_BLOCK_THREADS / WARP];
inline thread_local int linearThread; /* threadIdx.x + threadIdx.y * blockDim.x */

inline int lane() { return linearThread % WARP; }
inline void syncWarp() { warpBarrier[linearThread / WARP].wait(); }

/* surface objects: a handle is an index into this table of host RGBA8 planes (0 stays invalid) */
struct Surface { unsigned char *data; int width, height; };
constexpr int MAX_SURFACE_HANDLES = 1024;
inline Surface surfaces[MAX_SURFACE_HANDLES];

[[noreturn]] inline void trap(const char *what, long long handle, int x, int y)
{
    std::fprintf(stderr, "ref_shim: %s (surface %lld, x %d, y %d)\n", what, handle, x, y);
    std::abort();
}
} // namespace ref_shim

/* built-in variables: one OS thread per CUDA thread, so the thread's own indices are thread-local */
inline thread_local uint3 threadIdx;
inline thread_local uint3 blockIdx;
inline dim3 blockDim, gridDim;

/* "__syncthreads() waits until all threads in the thread block have reached this point": a real barrier */
inline void __syncthreads() { ref_shim::blockBarrier.wait(); }

typedef unsigned long long cudaSurfaceObject_t;
enum cudaSurfaceBoundaryMode { cudaBoundaryModeZero = 0, cudaBoundaryModeClamp = 1, cudaBoundaryModeTrap = 2 };

/* surf2Dread: "x is the byte coordinate"; cudaBoundaryModeClamp: "out-of-range coordinates are clamped to the valid range".
 * The clamp acts on the pixel that the byte coordinate addresses, in each axis on its own. */
template <typename T>
inline T surf2Dread(cudaSurfaceObject_t surface, int xBytes, int y, cudaSurfaceBoundaryMode mode = cudaBoundaryModeTrap)
{
    static_assert(sizeof(T) == 4, "the kernels read RGBA8 pixels only");
    if(surface == 0 || surface >= ref_shim::MAX_SURFACE_HANDLES || !ref_shim::surfaces[surface].data)
        ref_shim::trap("read of an invalid surface", static_cast<long long>(surface), xBytes, y);
    const ref_shim::Surface &s = ref_shim::surfaces[surface];
    int x = xBytes >> 2; /* arithmetic shift: floor for the negative coordinates a shifted pixel can have */
    if(mode != cudaBoundaryModeClamp && (x < 0 || x >= s.width || y < 0 || y >= s.height))
        ref_shim::trap("out-of-range surface read without clamp", static_cast<long long>(surface), x, y);
    x = x < 0 ? 0 : (x >= s.width ? s.width - 1 : x);
    y = y < 0 ? 0 : (y >= s.height ? s.height - 1 : y);
    T value;
    __builtin_memcpy(&value, s.data + (static_cast<size_t>(y) * s.width + x) * 4, 4);
    return value;
}

/* surf2Dwrite, default cudaBoundaryModeTrap: "out-of-range accesses cause the kernel execution to fail" */
template <typename T>
inline void surf2Dwrite(T value, cudaSurfaceObject_t surface, int xBytes, int y, cudaSurfaceBoundaryMode = cudaBoundaryModeTrap)
{
    static_assert(sizeof(T) == 4, "the kernels write RGBA8 pixels only");
    if(surface == 0 || surface >= ref_shim::MAX_SURFACE_HANDLES || !ref_shim::surfaces[surface].data)
        ref_shim::trap("write to an invalid surface", static_cast<long long>(surface), xBytes, y);
    const ref_shim::Surface &s = ref_shim::surfaces[surface];
    int x = xBytes >> 2;
    if(x < 0 || x >= s.width || y < 0 || y >= s.height)
        ref_shim::trap("out-of-range surface write", static_cast<long long>(surface), x, y);
    __builtin_memcpy(s.data + (static_cast<size_t>(y) * s.width + x) * 4, &value, 4);
}

/* __fmaf_rn: "compute x × y + z as a single operation, in round-to-nearest-even mode" — fused in every build */
inline float __fmaf_rn(float x, float y, float z) { return __builtin_fmaf(x, y, z); }
/* __float2int_rn: "convert a float to a signed integer in round-to-nearest-even mode" (the default rounding mode here) */
inline int __float2int_rn(float x) { return static_cast<int>(__builtin_rintf(x)); }

/* min / max on floats, for the reference's unused clampColorValue (its half argument converts) */
inline float max(float a, float b) { return __builtin_fmaxf(a, b); }
inline float min(float a, float b) { return __builtin_fminf(a, b); }

/* round(float) has to be the float overload (CUDA: "round to nearest integer value in floating-point", halfway cases away from zero) */
static_assert(std::is_same_v<decltype(round(1.0f)), float>, "round(float) must not promote to double");

#endif
