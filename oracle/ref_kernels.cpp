/* ref_kernels.cpp — runs the reference's OWN kernels (its src/kernels.cu, unchanged) on the CPU, as a library for the tests.
 *
 * TEST INFRASTRUCTURE ONLY.  oracle/Makefile compiles THIS file with -I$(REF)/src and -Iref_shim into
 * oracle/_ref/libref_kernels.so (-ffp-contract=fast, standing for nvcc's default --fmad=true) and
 * oracle/_ref/libref_kernels_nofma.so (-ffp-contract=off: exists only to show that the tests can tell the two apart).
 * The kernel source is reached through the include path at build time; nothing of it is copied, generated or quoted here.
 * The CUDA language it needs comes from the headers in oracle/ref_shim/, every line of which is this project's.
 *
 * Execution model (what a launch below does):
 *   - blocks of 16×16 threads, the grid W/16+1 × H/16+1 — the reference's src/interpolator.cu:258-259;
 *   - dynamic shared memory of 2·N·64 bytes, plus (32·16)·2·(256/32) bytes for the tensor kernel — src/interpolator.cu:49, 276;
 *     it is zeroed for each launch (on the device it is undefined: a kernel that reads what it never wrote cannot be compared);
 *   - one OS thread per CUDA thread, so __syncthreads is a real barrier over the block's threads and a kernel may
 *     synchronise as often as it likes; a thread that returns from the kernel leaves the barriers;
 *   - the wmma calls are collective over the 32 consecutive linear thread ids of a warp (ref_shim/mma.h);
 *   - blocks run one after another, in the order of blockIdx.y, then blockIdx.x.
 *
 * The parameters a launch takes (offsets, weights, focus-map image ids, block radius) are what the reference's host class
 * computes with glm in src/interpolator.cu:139-246; that file needs a CUDA compiler and is NOT built: the callers pass the
 * oracle's restatement of it, as data.
 *
 * A launch refuses, with a message (ref_last_error), what the reference's kernels cannot do:
 *   a view count other than 64 (VIEW_TOTAL_COUNT); more than 256 images (MAX_IMAGES); an image count that is no multiple of 8
 *   (STD: loadWeightsSync copies N·64/256/2 dwords per thread, truncated) or of 16 (tensor: gridSize() >> 4 batches);
 *   fewer than 32 images for estimate (it reads 32 focusMapIDs); filter with a block radius under 10 in either axis (0/0);
 *   tensor launches whose warps are not whole (W no multiple of 16 or H odd: the lanes that left never join the collective calls).
 *
 * Built as C++20: the kernels shift negative pixel coordinates left (x << 2), which is two's-complement arithmetic on the
 * device and in C++20 but undefined before it.  -fno-strict-aliasing: they move halves through int4 pointers.
 */
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <cuda_fp16.h>
#include <mma.h>

#include <kernels.cu>

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#include <sanitizer/asan_interface.h>
#define REF_POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define REF_UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#endif
#endif
#ifndef REF_POISON
#define REF_POISON(p, n) ((void)0)
#define REF_UNPOISON(p, n) ((void)0)
#endif

namespace Kernels
{
/* the block's dynamic shared memory, at the largest size a launch can ask for: MAX_IMAGES·64 weights + 8 warps × 32×16 pixels */
constexpr int SHARED_HALVES = MAX_IMAGES * VIEW_TOTAL_COUNT + 32 * 16 * 8;
alignas(16) half localMemory[SHARED_HALVES];
} // namespace Kernels

namespace
{
constexpr int BLOCK = 16;
constexpr int VIEWS = Kernels::VIEW_TOTAL_COUNT;
thread_local std::string lastError;

int fail(const std::string &message)
{
    lastError = message;
    return -1;
}

/* surface handles: inputs 1…N, outputs N+1…N+64, maps N+65 and N+66 — the order src/interpolator.cu:105-136 creates them in */
cudaSurfaceObject_t bindSurface(int handle, const unsigned char *data, int width, int height)
{
    ref_shim::surfaces[handle] = {const_cast<unsigned char *>(data), width, height};
    return static_cast<cudaSurfaceObject_t>(handle);
}

void clearSurfaces()
{
    for(auto &s : ref_shim::surfaces)
        s = {nullptr, 0, 0};
}

void setConstants(int width, int height, int cols, int rows, float focus, float range, const int32_t radius[2])
{
    int n = cols * rows;
    int values[Kernels::CONSTANTS_COUNT] = {width, height, cols, rows, 0, n, n * VIEWS,
                                            static_cast<int>(std::round(focus * width)), static_cast<int>(std::round(range * width)),
                                            radius ? radius[0] : 0, radius ? radius[1] : 0};
    std::memcpy(Kernels::constants, values, sizeof(values));
    Kernels::inFocus = focus;
    Kernels::inRange = range;
}

template <typename Kernel>
void launch(int width, int height, size_t sharedBytes, Kernel kernel)
{
    blockDim = {BLOCK, BLOCK, 1};
    gridDim = {static_cast<unsigned>(width / BLOCK + 1), static_cast<unsigned>(height / BLOCK + 1), 1};
    const int threads = BLOCK * BLOCK;
    REF_UNPOISON(Kernels::localMemory, sizeof(Kernels::localMemory));
    std::memset(static_cast<void *>(Kernels::localMemory), 0, sizeof(Kernels::localMemory));
    REF_POISON(reinterpret_cast<char *>(Kernels::localMemory) + sharedBytes, sizeof(Kernels::localMemory) - sharedBytes);
    std::vector<std::thread> pool;
    pool.reserve(threads);
    for(unsigned by = 0; by < gridDim.y; by++)
        for(unsigned bx = 0; bx < gridDim.x; bx++)
        {
            ref_shim::blockBarrier.reset(threads);
            for(auto &w : ref_shim::warpBarrier)
                w.reset(ref_shim::WARP);
            pool.clear();
            for(int t = 0; t < threads; t++)
                pool.emplace_back([=] {
                    threadIdx = {static_cast<unsigned>(t % BLOCK), static_cast<unsigned>(t / BLOCK), 0};
                    blockIdx = {bx, by, 0};
                    ref_shim::linearThread = t;
                    kernel();
                    ref_shim::warpBarrier[t / ref_shim::WARP].drop();
                    ref_shim::blockBarrier.drop();
                });
            for(auto &th : pool)
                th.join();
        }
    REF_UNPOISON(Kernels::localMemory, sizeof(Kernels::localMemory));
}

struct BlendArgs
{
    const uint8_t *in;
    int cols, rows, width, height, views;
    const int32_t *focused;
    const float *offsets;
    const uint16_t *weights;
    int allFocus;
    const uint8_t *map0, *map1;
    float focus, range;
    uint8_t *out;
};

int checkBlend(const BlendArgs &a, int multiple, const char *what)
{
    int n = a.cols * a.rows;
    if(a.views != VIEWS)
        return fail(std::string(what) + ": the reference renders 64 views, not " + std::to_string(a.views));
    if(n < 1 || n > Kernels::MAX_IMAGES)
        return fail(std::string(what) + ": the reference holds at most 256 images, not " + std::to_string(n));
    if(n % multiple != 0)
        return fail(std::string(what) + ": the image count " + std::to_string(n) + " is no multiple of " + std::to_string(multiple));
    if(a.width < 1 || a.height < 1)
        return fail(std::string(what) + ": empty image");
    if(a.allFocus && (!a.map0 || !a.map1))
        return fail(std::string(what) + ": an all-focus launch needs both maps");
    return 0;
}

/* binds the inputs, outputs and maps, and uploads offsets and constants, as src/interpolator.cu:95-154, 226-246 does */
void bindBlend(const BlendArgs &a, std::vector<uint8_t> &blank)
{
    int n = a.cols * a.rows;
    size_t plane = static_cast<size_t>(a.width) * a.height * 4;
    clearSurfaces();
    for(int g = 0; g < n; g++)
        Kernels::inputSurfaces[g] = bindSurface(1 + g, a.in + plane * g, a.width, a.height);
    for(int v = 0; v < VIEWS; v++)
        Kernels::outputSurfaces[v] = bindSurface(1 + n + v, a.out + plane * v, a.width, a.height);
    blank.assign(plane, 0);
    Kernels::mapSurfaces[0] = bindSurface(1 + n + VIEWS, a.map0 ? a.map0 : blank.data(), a.width, a.height);
    Kernels::mapSurfaces[1] = bindSurface(2 + n + VIEWS, a.map1 ? a.map1 : blank.data(), a.width, a.height);
    for(int g = 0; g < n; g++)
    {
        Kernels::focusedOffsets[g] = {a.focused[2 * g], a.focused[2 * g + 1]};
        Kernels::offsets[g] = {a.offsets[2 * g], a.offsets[2 * g + 1]};
    }
    setConstants(a.width, a.height, a.cols, a.rows, a.focus, a.range, nullptr);
}
} // namespace

extern "C"
{
const char *ref_last_error(void)
{
    return lastError.c_str();
}

/* 1 in the library built with -ffp-contract=fast, 0 in the one built with -ffp-contract=off */
int ref_contracts(void)
{
#ifdef REF_CONTRACT_OFF
    return 0;
#else
    return 1;
#endif
}

/* Standard::process<false|true>: in [N][H][W][4], focused [N][2], offsets [N][2], weights [64][N] fp16 bits, out [64][H][W][4] */
int ref_std(const uint8_t *in, int cols, int rows, int width, int height, int views, const int32_t *focused, const float *offsets,
            const uint16_t *weights, int allFocus, const uint8_t *map0, const uint8_t *map1, float focus, float range, uint8_t *out)
{
    BlendArgs a{in, cols, rows, width, height, views, focused, offsets, weights, allFocus, map0, map1, focus, range, out};
    if(checkBlend(a, 8, "STD"))
        return -1;
    std::vector<uint8_t> blank;
    bindBlend(a, blank);
    std::vector<half> w(static_cast<size_t>(cols) * rows * VIEWS);
    std::memcpy(static_cast<void *>(w.data()), weights, w.size() * sizeof(half));
    size_t shared = sizeof(half) * w.size();
    if(allFocus)
        launch(width, height, shared, [&] { Kernels::Standard::process<true>(w.data()); });
    else
        launch(width, height, shared, [&] { Kernels::Standard::process<false>(w.data()); });
    clearSurfaces();
    return 0;
}

/* Tensors::process<false|true>: arguments as ref_std */
int ref_ten(const uint8_t *in, int cols, int rows, int width, int height, int views, const int32_t *focused, const float *offsets,
            const uint16_t *weights, int allFocus, const uint8_t *map0, const uint8_t *map1, float focus, float range, uint8_t *out)
{
    BlendArgs a{in, cols, rows, width, height, views, focused, offsets, weights, allFocus, map0, map1, focus, range, out};
    if(checkBlend(a, 16, "TEN_WM"))
        return -1;
    if(width % BLOCK != 0 || height % 2 != 0)
        return fail("TEN_WM: " + std::to_string(width) + "x" + std::to_string(height) +
                    " leaves warps that are not whole (the width must be a multiple of 16 and the height even)");
    std::vector<uint8_t> blank;
    bindBlend(a, blank);
    std::vector<half> w(static_cast<size_t>(cols) * rows * VIEWS);
    std::memcpy(static_cast<void *>(w.data()), weights, w.size() * sizeof(half));
    size_t shared = sizeof(half) * w.size() + (32 * 16) * sizeof(half) * (BLOCK * BLOCK / 32);
    if(allFocus)
        launch(width, height, shared, [&] { Kernels::Tensors::process<true>(w.data()); });
    else
        launch(width, height, shared, [&] { Kernels::Tensors::process<false>(w.data()); });
    clearSurfaces();
    return 0;
}

/* FocusMap::estimate: ids[32] are the focus-map images, map0 [H][W][4] is written */
int ref_estimate(const uint8_t *in, int cols, int rows, int width, int height, const float *offsets, const int32_t *ids, int nIds,
                 float focus, float range, const int32_t radius[2], uint8_t *map0)
{
    int n = cols * rows;
    if(n > Kernels::MAX_IMAGES)
        return fail("estimate: the reference holds at most 256 images, not " + std::to_string(n));
    if(n < Kernels::FOCUS_MAP_IDS_COUNT || nIds != Kernels::FOCUS_MAP_IDS_COUNT)
        return fail("estimate: the reference reads 32 focus-map images; " + std::to_string(n) + " images and " + std::to_string(nIds) +
                    " ids were given");
    for(int i = 0; i < nIds; i++)
        if(ids[i] < 0 || ids[i] >= n)
            return fail("estimate: focus-map image id out of range");
    if(width < 1 || height < 1 || radius[0] < 1 || radius[1] < 1)
        return fail("estimate: empty image, or a block radius under 1 (the tap loops would not advance)");
    size_t plane = static_cast<size_t>(width) * height * 4;
    clearSurfaces();
    for(int g = 0; g < n; g++)
    {
        Kernels::inputSurfaces[g] = bindSurface(1 + g, in + plane * g, width, height);
        Kernels::offsets[g] = {offsets[2 * g], offsets[2 * g + 1]};
    }
    std::vector<uint8_t> map1(plane, 0);
    Kernels::mapSurfaces[0] = bindSurface(1 + n + VIEWS, map0, width, height);
    Kernels::mapSurfaces[1] = bindSurface(2 + n + VIEWS, map1.data(), width, height);
    std::memcpy(Kernels::focusMapIDs, ids, sizeof(int) * Kernels::FOCUS_MAP_IDS_COUNT);
    setConstants(width, height, cols, rows, focus, range, radius);
    launch(width, height, sizeof(half) * static_cast<size_t>(n) * VIEWS, [] { Kernels::FocusMap::estimate(); });
    clearSurfaces();
    return 0;
}

/* FocusMap::filter: reads map0, writes map1 */
int ref_filter(const uint8_t *map0, int width, int height, const int32_t radius[2], uint8_t *map1)
{
    if(radius[0] < 10 || radius[1] < 10)
        return fail("filter: a block radius under 10 makes radius/10 zero, and the reference then divides 0 by 0");
    if(width < 1 || height < 1)
        return fail("filter: empty image");
    clearSurfaces();
    Kernels::mapSurfaces[0] = bindSurface(1, map0, width, height);
    Kernels::mapSurfaces[1] = bindSurface(2, map1, width, height);
    setConstants(width, height, 1, 1, 0.0f, 0.0f, radius);
    launch(width, height, sizeof(half) * VIEWS, [] { Kernels::FocusMap::filter(); });
    clearSurfaces();
    return 0;
}
} // extern "C"

#ifdef REF_SELFTEST
/* One tiny case per kernel, for a build with -fsanitize=address,undefined: any report makes the run fail.  The checks are
 * properties that need no second implementation: one-hot weights copy the shifted input, a constant map filters to itself. */
#include <cstdio>

namespace
{
int failures = 0;

void expect(bool ok, const char *what)
{
    if(!ok)
    {
        std::fprintf(stderr, "ref-selftest: FAILED %s\n", what);
        failures++;
    }
}

uint8_t noise(uint32_t i)
{
    i = i * 747796405u + 2891336453u;
    i = ((i >> ((i >> 28) + 4)) ^ i) * 277803737u;
    return static_cast<uint8_t>(((i >> 22) ^ i) >> 13);
}
} // namespace

int main()
{
    const int cols = 4, rows = 8, n = cols * rows, W = 32, H = 18;
    const size_t plane = static_cast<size_t>(W) * H * 4;
    std::vector<uint8_t> in(plane * n), out(plane * VIEWS), map0(plane), map1(plane);
    for(size_t i = 0; i < in.size(); i++)
        in[i] = i % 4 == 3 ? 255 : noise(static_cast<uint32_t>(i));
    std::vector<int32_t> focused(2 * n);
    std::vector<float> offsets(2 * n);
    for(int g = 0; g < n; g++)
    {
        focused[2 * g] = g % 7 - 3;
        focused[2 * g + 1] = g % 5 - 2;
        offsets[2 * g] = (g % 7 - 3) * 4.25f;
        offsets[2 * g + 1] = (g % 5 - 2) * 3.5f;
    }
    /* view v copies image v % n: weight 1.0 (0x3c00) there, 0 elsewhere */
    std::vector<uint16_t> weights(static_cast<size_t>(VIEWS) * n, 0);
    for(int v = 0; v < VIEWS; v++)
        weights[static_cast<size_t>(v) * n + v % n] = 0x3c00;
    auto copiesShiftedInput = [&](const char *what) {
        bool ok = true;
        for(int v = 0; v < VIEWS && ok; v++)
            for(int y = 0; y < H && ok; y++)
                for(int x = 0; x < W && ok; x++)
                {
                    int g = v % n;
                    int sx = std::min(std::max(x + focused[2 * g], 0), W - 1), sy = std::min(std::max(y + focused[2 * g + 1], 0), H - 1);
                    ok = std::memcmp(&out[plane * v + (static_cast<size_t>(y) * W + x) * 4], &in[plane * g + (static_cast<size_t>(sy) * W + sx) * 4], 4) == 0;
                }
        expect(ok, what);
    };
    std::fill(out.begin(), out.end(), 0x5a);
    expect(ref_std(in.data(), cols, rows, W, H, VIEWS, focused.data(), offsets.data(), weights.data(), 0, nullptr, nullptr, 0.0f, 0.0f, out.data()) == 0, "ref_std runs");
    copiesShiftedInput("STD with one-hot weights copies the shifted input");
    std::fill(out.begin(), out.end(), 0x5a);
    expect(ref_ten(in.data(), cols, rows, W, H, VIEWS, focused.data(), offsets.data(), weights.data(), 0, nullptr, nullptr, 0.0f, 0.0f, out.data()) == 0, "ref_ten runs");
    copiesShiftedInput("TEN_WM with one-hot weights copies the shifted input");

    int32_t ids[32], radius[2] = {12, 10};
    for(int i = 0; i < 32; i++)
        ids[i] = (i * 5) % n;
    expect(ref_estimate(in.data(), cols, rows, W, H, offsets.data(), ids, 32, -0.1f, 0.7f, radius, map0.data()) == 0, "ref_estimate runs");
    bool grey = true;
    for(size_t i = 0; i < plane; i += 4)
        grey = grey && map0[i] == map0[i + 1] && map0[i] == map0[i + 2] && map0[i + 3] == 255;
    expect(grey, "estimate writes grey opaque pixels everywhere");
    expect(ref_filter(map0.data(), W, H, radius, map1.data()) == 0, "ref_filter runs");
    std::vector<uint8_t> flat(plane, 77), filtered(plane, 0);
    expect(ref_filter(flat.data(), W, H, radius, filtered.data()) == 0, "ref_filter runs on a constant map");
    bool same = true;
    for(size_t i = 0; i < plane; i += 4)
        same = same && filtered[i] == 77 && filtered[i + 3] == 255;
    expect(same, "a constant map filters to itself");
    /* all-focus launches from the maps just made; zero offsets make every view a copy again */
    std::vector<float> still(2 * n, 0.0f);
    std::vector<int32_t> keep = focused;
    std::fill(focused.begin(), focused.end(), 0);
    expect(ref_std(in.data(), cols, rows, W, H, VIEWS, focused.data(), still.data(), weights.data(), 1, map0.data(), map1.data(), -0.1f, 0.7f, out.data()) == 0, "all-focus ref_std runs");
    copiesShiftedInput("all-focus STD with zero offsets copies the input");
    expect(ref_ten(in.data(), cols, rows, W, H, VIEWS, focused.data(), offsets.data(), weights.data(), 1, map0.data(), map1.data(), -0.1f, 0.7f, out.data()) == 0, "all-focus ref_ten runs");

    /* refusals */
    int32_t small[2] = {9, 25};
    expect(ref_filter(map0.data(), W, H, small, map1.data()) != 0, "filter refuses a radius under 10");
    expect(ref_std(in.data(), cols, rows, W, H, 32, keep.data(), offsets.data(), weights.data(), 0, nullptr, nullptr, 0, 0, out.data()) != 0, "STD refuses 32 views");
    expect(ref_std(in.data(), 3, 4, W, H, VIEWS, keep.data(), offsets.data(), weights.data(), 0, nullptr, nullptr, 0, 0, out.data()) != 0, "STD refuses 12 images");
    expect(ref_ten(in.data(), 3, 8, W, H, VIEWS, keep.data(), offsets.data(), weights.data(), 0, nullptr, nullptr, 0, 0, out.data()) != 0, "TEN_WM refuses 24 images");
    expect(ref_ten(in.data(), cols, rows, 31, H, VIEWS, keep.data(), offsets.data(), weights.data(), 0, nullptr, nullptr, 0, 0, out.data()) != 0, "TEN_WM refuses a ragged width");
    expect(ref_ten(in.data(), cols, rows, W, 17, VIEWS, keep.data(), offsets.data(), weights.data(), 0, nullptr, nullptr, 0, 0, out.data()) != 0, "TEN_WM refuses an odd height");
    expect(ref_estimate(in.data(), 4, 4, W, H, offsets.data(), ids, 32, 0, 1, radius, map0.data()) != 0, "estimate refuses 16 images");
    expect(ref_std(in.data(), 16, 17, W, H, VIEWS, keep.data(), offsets.data(), weights.data(), 0, nullptr, nullptr, 0, 0, out.data()) != 0, "STD refuses 272 images");
    if(failures == 0)
        std::printf("ref-selftest: ok (%s build)\n", ref_contracts() ? "contracting" : "non-contracting");
    return failures ? 1 : 0;
}
#endif
