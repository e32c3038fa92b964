// lfi_dispatch.hpp — which kernel serves a render, and how.  route_blend decides each blend launch in one step: the kernel, whether it
// reads the derived planar copy of the inputs (ensure_planar), and, in the planar view layout, whether it writes the byte planes itself
// or RGBA into the scratch copy that a conversion pass turns into planes.  In that order: the generic kernels where the others cannot
// serve (per-batch rounding, weights outside [0, 2), pre-quantisation dumps); the variant's order of preference (lfi_set_variant: its
// first choice, then the fallbacks below it); the output form, a property of the kernel chosen.  launch_blend makes the copy valid when
// the route reads it (or routes again without it) and launches; the launchers only compute grids and instantiate kernels.
// Replaces the method / allFocus dispatch of Interpolator::interpolate (reference src/interpolator.cu:270-290).
// Included by lfi_hip.hip only (one translation unit), after lfi_context.hpp.
#pragma once

#include <type_traits>

#include "lfi_context.hpp"
#include "blend_std.hpp"
#include "blend_ten.hpp"
#include "blend_ten_persist.hpp"
#include "blend_planar.hpp"
#include "blend_p3.hpp"
#include "blend_stdx.hpp"
#include "blend_stdxa.hpp"
#include "blend_af.hpp"
#include "blend_wave.hpp"
#include "blend_vfocus.hpp"
#include "blend_vfocus_af.hpp"
#include "deep_blend.hpp"
#include "blend_inframe.hpp"
#include "blend_linear.hpp"
#include "lfi_band_probe.hpp"

namespace {

// one entry per kernel name that note_kernel reports
enum class BlendKernel
{
    ten_m16,
    ten_direct,
    p3,
    p3_rgba,
    planar_ten,
    persist_ten,
    persist_ten_af,
    wave_ten,
    stdx,
    planar_stdf,
    stdxa,
    afs,
    persist_std,
    persist_std_af,
    wave_std,
    std_mfma,
    std_valu,
    std_vfma,
    deep_ten, // deep_blend.hpp: LFI_FLAG_DEEP_VIEWS
    deep_std,
    inframe_ten, // blend_inframe.hpp: LFI_FLAG_IN_FRAME
    inframe_std,
    linear_ten, // blend_linear.hpp: LFI_FLAG_LINEAR_LIGHT
    linear_std,
};

// The generic kernels: plain fp32 epilogue, any weights, pre-quantisation dumps, per-batch rounding (TEN_WM).  They run one pixel grid
// over the whole image; every other kernel honours a row window.
bool generic_kernel(BlendKernel k)
{
    using K = BlendKernel;
    return k == K::ten_m16 || k == K::ten_direct || k == K::std_mfma || k == K::std_valu || k == K::std_vfma;
}

bool kernel_reads_copy(BlendKernel k)
{
    using K = BlendKernel;
    return k == K::p3 || k == K::p3_rgba || k == K::planar_ten || k == K::stdx || k == K::planar_stdf;
}

// planar view layout: does kernel k write the byte planes itself?  Its planar-view epilogue addresses `planes` byte planes (3 per view)
// with one 32-bit per-lane offset: blend_p3 / blend_stdx a wave's 16 views, blend_persist's store_tile_planar the 32 views of a pass
// (all-focus renders only), blend_stdxa the 64 views of a launch
bool kernel_writes_planar_views(const lfi_ctx *c, BlendKernel k)
{
    using K = BlendKernel;
    const int planes = k == K::p3 || k == K::stdx ? 48 : k == K::persist_ten_af ? 96 : k == K::stdxa ? 192 : 0;
    return planes && (uint64_t)planes * (uint64_t)c->out_rows * (uint64_t)view_pitch(c) < (1ull << 32);
}

struct Variant
{
    const char *name;
    BlendKernel first; // its first choice; route_blend falls back from it where it does not apply
};

// first entry = default ("auto")
const Variant kTenVariants[] = {
    {"p3_rgba_nt", BlendKernel::p3_rgba}, // blend_p3 with the RGBA epilogue; blend_planar / blend_persist where it does not apply
    {"planar_m2_nt", BlendKernel::planar_ten},
    {"persist_m2_nt", BlendKernel::persist_ten},
    {"wave_m2_nt", BlendKernel::wave_ten},
    {"direct_p1m2", BlendKernel::ten_direct}, // generic
};
const Variant kStdVariants[] = {
    {"filtered_m2_nt", BlendKernel::stdx},  // the band method (blend_stdx / blend_planar<STDF>, blend_stdxa all-focus); blend_wave / blend_persist
    {"filtered_gather_once", BlendKernel::afs}, // the same with blend_afs for all-focus renders of 3–4 chunks
    {"wave_m2_nt", BlendKernel::wave_std},
    {"persist_m2_nt", BlendKernel::persist_std},
    {"mfma_p1m2", BlendKernel::std_mfma}, // generic
    {"valu", BlendKernel::std_valu},      // the reference-shaped one-pixel-per-thread kernel: exactness anchor
    {"vfma", BlendKernel::std_vfma},      // the non-tensor wavefront kernel
};
const int kNumTenVariants = sizeof(kTenVariants) / sizeof(kTenVariants[0]);
const int kNumStdVariants = sizeof(kStdVariants) / sizeof(kStdVariants[0]);

// RGBA views by blend_p3 with its RGBA epilogue: a wave's 16 RGBA planes addressable with 32 bits
bool p3_rgba_planes_fit(const lfi_ctx *c)
{
    return (uint64_t)16 * (uint64_t)c->out_rows * (uint64_t)c->width * 4u < (1ull << 32);
}

struct BlendRoute
{
    BlendKernel kernel;
    int nch;         // 64-image chunks of the launch (the kernels instantiated per chunk count)
    bool reads_copy; // reads the derived planar copy of the inputs
    bool planar_out; // planar view layout: writes the byte planes itself (else RGBA into the scratch copy, converted afterwards)
};

// The route of a blend launch.  copy_ok = false: the route when the derived copy cannot be made valid.  No side effects, no allocation:
// it runs on every launch.
BlendRoute route_blend(const lfi_ctx *c, int method, bool all_focus, const KernelArgs &a, bool copy_ok)
{
    using K = BlendKernel;
    const bool ten = method == LFI_METHOD_TEN_WM, planar_views = c->out_layout == LFI_LAYOUT_PLANAR_RGB;
    const K first = ten ? kTenVariants[c->ten_variant].first : kStdVariants[c->std_variant].first;
    const int nch = (a.k_pad + lfi::P3_KC - 1) / lfi::P3_KC;
    // 0a. linear-light blending (LFI_FLAG_LINEAR_LIGHT): one kernel for both methods; launch_blend (flagged_refused) has refused what it does not
    // serve — the other two flags beside it among that
    if(c->flags & LFI_FLAG_LINEAR_LIGHT)
        return {ten ? K::linear_ten : K::linear_std, nch, true, true};
    // 0. deep views (LFI_FLAG_DEEP_VIEWS): one kernel for both methods; launch_blend (flagged_refused) has refused what it does not serve
    if(c->flags & LFI_FLAG_DEEP_VIEWS)
        return {ten ? K::deep_ten : K::deep_std, nch, true, true};
    // 0b. in-frame blending (LFI_FLAG_IN_FRAME): likewise; launch_blend (flagged_refused) has refused what it does not serve
    if(c->flags & LFI_FLAG_IN_FRAME)
        return {ten ? K::inframe_ten : K::inframe_std, nch, true, true};
    const bool fixed_copy = copy_ok && !all_focus;
    // wave-private pipelines (blend_wave.hpp) where they apply: fixed focus, one chunk of images, one view pass
    const bool wave_fits = !all_focus && a.k_pad <= 64 && a.v1 - a.v0 <= 64;
    const K k = [&] {
        // 1. the generic kernels serve what the others cannot
        if(ten && (c->flags & LFI_FLAG_TEN_ROUND_PER_BATCH))
            return K::ten_m16; // the reference's half-accumulator model (oracle M16), exact: fp64 on the vector pipe (blend_ten.hpp)
        if(generic_kernel(first))
            return first;
        if(a.prequant || (ten && !c->weights_scalable)) // (the packed epilogue of the TEN_WM kernels: weights in [0, 2), the ×2^15 copy)
            return ten ? K::ten_direct : K::std_mfma;
        // 2. the variant's order of preference
        if(ten)
        {
            if(first == K::wave_ten && wave_fits)
                return K::wave_ten;
            if((first == K::p3_rgba || first == K::planar_ten) && fixed_copy)
            {
                // planar views: blend_p3 writes them.  RGBA views: blend_p3 with its RGBA epilogue where it pays — TWO TO FOUR chunks of
                // images (15×15 grids: −8 % at configs 3 and 5; with one chunk blend_planar is as fast, and blend_persist faster for several
                // view passes: profiles/r04_rgba_p3_ab.txt)
                if(planar_views && a.k_pad <= 4 * lfi::P3_KC && kernel_writes_planar_views(c, K::p3))
                    return K::p3;
                if(first == K::p3_rgba && a.k_pad > lfi::P3_KC && a.k_pad <= 4 * lfi::P3_KC && p3_rgba_planes_fit(c))
                    return K::p3_rgba;
                return K::planar_ten;
            }
            return all_focus ? K::persist_ten_af : K::persist_ten;
        }
        // STD: the band method (MFMA sum + exact recomputation inside the rounding band) for weights for which its error bounds hold
        const bool band = c->weights_scalable && c->weights_sum_ok && a.k_pad <= 4 * lfi::P3_KC;
        if((first == K::stdx || first == K::afs) && band && all_focus)
            // blend_stdxa, on the per-pixel gather pipeline; "filtered_gather_once": three or four chunks by blend_afs (64-pixel tiles whose
            // whole stack of samples stays in LDS, every sample gathered once, where blend_stdxa gathers chunks 2 and 3 a second time for the
            // chain).  Half the fabric traffic, the same bytes — and not faster (4.8 against 4.7 ms at config 5: bound by instruction issue,
            // profiles/r04_notes.md), so it is a selectable variant and the second implementation in the parity tests, not the default.
            return first == K::afs && nch >= 3 ? K::afs : K::stdxa;
        if((first == K::stdx || first == K::afs) && band && fixed_copy)
            // from the planar copy: blend_stdx for more than one chunk of images (the chain's bytes fetched a second time), and for ONE chunk
            // where it writes planar views itself — blend_planar<STDF> would go through the scratch copy and the conversion (config 2: 0.45 ms
            // against 0.23).  With RGBA views blend_planar<STDF> stays: as fast at config 2, 15 % faster for one rank of config 4
            // (profiles/r04_rgba_p3_ab.txt).
            return a.k_pad > lfi::P3_KC || (planar_views && kernel_writes_planar_views(c, K::stdx)) ? K::stdx : K::planar_stdf;
        if(first != K::persist_std && wave_fits)
            return K::wave_std;
        return all_focus ? K::persist_std_af : K::persist_std;
    }();
    // 3. the output form
    return {k, nch, kernel_reads_copy(k), planar_views && kernel_writes_planar_views(c, k)};
}

int next_sweep_direction(const lfi_ctx *c);

// one launch per 64 views (blend_stdx / blend_stdxa / blend_afs / blend_p3 over several chunks: a wave's accumulators hold 16 views)
template <class F>
void per_64_views(const KernelArgs &a_in, F &&launch)
{
    for(int v0 = a_in.v0; v0 < a_in.v1; v0 += 64)
    {
        KernelArgs a = a_in;
        a.v0 = v0;
        a.v1 = std::min(v0 + 64, a_in.v1);
        launch(a);
    }
}

// launch(std::integral_constant<int, N>) for the chunk count nch, over the forms a kernel is instantiated for: MIN..3, and 4 for more
template <int MIN, class F>
void with_chunks(int nch, F &&launch)
{
    if constexpr(MIN <= 1)
    {
        if(nch == 1)
            return launch(std::integral_constant<int, 1>());
    }
    if constexpr(MIN <= 2)
    {
        if(nch == 2)
            return launch(std::integral_constant<int, 2>());
    }
    if(nch == 3)
        return launch(std::integral_constant<int, 3>());
    launch(std::integral_constant<int, 4>());
}

// the generic MFMA kernels' grid: tiles of 32 pixels of a row, passes of 64 views, 4 / vpw tiles per workgroup
struct GenericGrid
{
    int tiles_x, n_tiles, passes, vpw;
    dim3 grid;
};
GenericGrid generic_grid(const KernelArgs &a)
{
    GenericGrid g;
    g.tiles_x = (a.width + 31) / 32;
    g.n_tiles = g.tiles_x * a.height;
    g.passes = (a.v1 - a.v0 + 63) / 64;
    g.vpw = g.passes >= 4 ? 4 : (g.passes >= 2 ? 2 : 1);
    const int tiles_per_wg = 4 / g.vpw;
    g.grid = dim3((g.n_tiles + tiles_per_wg - 1) / tiles_per_wg);
    return g;
}

void launch_ten_m16(const lfi_ctx *c, const KernelArgs &a, bool all_focus)
{
    note_kernel(c, "blend_ten_m16");
    if(all_focus)
        hipLaunchKernelGGL(lfi::blend_ten_m16<true>, pixel_grid_of(c), dim3(256), 0, stream_of(c), a);
    else
        hipLaunchKernelGGL(lfi::blend_ten_m16<false>, pixel_grid_of(c), dim3(256), 0, stream_of(c), a);
}

void launch_ten_direct(const lfi_ctx *c, const KernelArgs &a, bool all_focus)
{
    const GenericGrid g = generic_grid(a);
    note_kernel(c, "blend_ten_direct");
    if(all_focus)
        hipLaunchKernelGGL((lfi::blend_ten_direct<1, 2, true>), g.grid, dim3(256), 0, stream_of(c), a, g.tiles_x, g.n_tiles, g.passes, g.vpw);
    else
        hipLaunchKernelGGL((lfi::blend_ten_direct<1, 2, false>), g.grid, dim3(256), 0, stream_of(c), a, g.tiles_x, g.n_tiles, g.passes, g.vpw);
}

void launch_std_mfma(const lfi_ctx *c, const KernelArgs &a, bool all_focus)
{
    const GenericGrid g = generic_grid(a);
    note_kernel(c, "blend_std_mfma");
    if(all_focus)
        hipLaunchKernelGGL((lfi::blend_std_mfma<1, 2, true>), g.grid, dim3(256), 0, stream_of(c), a, g.tiles_x, g.n_tiles, g.passes, g.vpw);
    else
        hipLaunchKernelGGL((lfi::blend_std_mfma<1, 2, false>), g.grid, dim3(256), 0, stream_of(c), a, g.tiles_x, g.n_tiles, g.passes, g.vpw);
}

void launch_std_valu(const lfi_ctx *c, const KernelArgs &a, bool all_focus)
{
    note_kernel(c, "blend_std_valu");
    if(all_focus)
        hipLaunchKernelGGL((lfi::blend_std_valu<true, 16>), pixel_grid_of(c), dim3(256), 0, stream_of(c), a);
    else
        hipLaunchKernelGGL((lfi::blend_std_valu<false, 16>), pixel_grid_of(c), dim3(256), 0, stream_of(c), a);
}

void launch_std_vfma(const lfi_ctx *c, const KernelArgs &a, bool all_focus)
{
    note_kernel(c, "blend_std_vfma");
    if(all_focus)
        hipLaunchKernelGGL((lfi::blend_std_vfma<true>), pixel_grid_of(c), dim3(256), 0, stream_of(c), a);
    else
        hipLaunchKernelGGL((lfi::blend_std_vfma<false>), pixel_grid_of(c), dim3(256), 0, stream_of(c), a);
}

// planar_out: all-focus TEN_WM only (the one planar-view form of blend_persist)
template <bool STD>
void launch_persist(const lfi_ctx *c, const KernelArgs &a, bool all_focus, bool planar_out)
{
    const int tiles_x = (a.width + 127) / 128;
    const int n_tiles = tiles_x * a.out_rows;
    const int passes = (a.v1 - a.v0 + 63) / 64;
    // persistent: two workgroups per CU (2 x 80 KB of LDS), each walks tiles j, j+G, j+2G ...
    const dim3 grid(std::min(n_tiles, 2 * cu_count_of(c))), block(256);
    note_kernel(c, STD ? (all_focus ? "blend_persist<STD,allfocus>" : "blend_persist<STD>") : (all_focus ? "blend_persist<TEN_WM,allfocus>" : "blend_persist<TEN_WM>"));
    if constexpr(!STD)
    {
        if(planar_out)
        {
            hipLaunchKernelGGL((lfi::blend_persist<false, 2, true, true, 64, 2, true>), grid, block, 0, stream_of(c), a, tiles_x, n_tiles, passes);
            return;
        }
    }
    if(all_focus)
        hipLaunchKernelGGL((lfi::blend_persist<STD, 2, true, true>), grid, block, 0, stream_of(c), a, tiles_x, n_tiles, passes);
    else
        hipLaunchKernelGGL((lfi::blend_persist<STD, 2, false, true>), grid, block, 0, stream_of(c), a, tiles_x, n_tiles, passes);
}

template <bool STD>
void launch_wave(const lfi_ctx *c, const KernelArgs &a)
{
    const int tiles_x = (a.width + 127) / 128;
    const int n_tiles = tiles_x * a.out_rows;
    const dim3 grid(std::min(n_tiles, 2 * cu_count_of(c))), block(256);
    note_kernel(c, STD ? "blend_wave<STD>" : "blend_wave<TEN_WM>");
    hipLaunchKernelGGL((lfi::blend_wave<STD, 2, true>), grid, block, 0, stream_of(c), a, tiles_x, n_tiles);
}

// from the planar copy of the inputs (blend_planar.hpp): TEN_WM, or STD by the band method (STDF)
template <bool STDF>
void launch_planar(const lfi_ctx *c, const KernelArgs &a)
{
    const int tiles_x = (a.width + 127) / 128;
    const int n_tiles = tiles_x * a.out_rows;
    const int passes = (a.v1 - a.v0 + 63) / 64;
    const dim3 grid(std::min(n_tiles, 2 * cu_count_of(c))), block(256);
    note_kernel(c, STDF ? "blend_planar<STDF>" : "blend_planar<TEN_WM>");
    hipLaunchKernelGGL((lfi::blend_planar<2, true, STDF>), grid, block, 0, stream_of(c), a, tiles_x, n_tiles, passes, STDF ? 0 : 1, next_sweep_direction(c));
}

void launch_stdx(const lfi_ctx *c, const KernelArgs &a_in, const BlendRoute &r)
{
    const int tiles_x = (a_in.width + lfi::P3_TPX - 1) / lfi::P3_TPX;
    const int n_tiles = tiles_x * a_in.out_rows;
    const dim3 grid(std::min(n_tiles, 2 * cu_count_of(c))), block(256);
    const int reverse = next_sweep_direction(c);
    note_kernel(c, "blend_stdx<STD>");
    per_64_views(a_in, [&](const KernelArgs &a) {
        with_chunks<1>(r.nch, [&](auto n) {
            if(r.planar_out)
                hipLaunchKernelGGL((lfi::blend_stdx<true, decltype(n)::value, true>), grid, block, 0, stream_of(c), a, tiles_x, n_tiles, reverse);
            else
                hipLaunchKernelGGL((lfi::blend_stdx<true, decltype(n)::value>), grid, block, 0, stream_of(c), a, tiles_x, n_tiles, reverse);
        });
    });
}

void launch_stdxa(const lfi_ctx *c, const KernelArgs &a_in, const BlendRoute &r)
{
    const int tiles_x = (a_in.width + 127) / 128;
    const int n_tiles = tiles_x * a_in.out_rows;
    const dim3 grid(std::min(n_tiles, 2 * cu_count_of(c))), block(256);
    note_kernel(c, "blend_stdxa<STD,allfocus>");
    per_64_views(a_in, [&](const KernelArgs &a) {
        with_chunks<1>(r.nch, [&](auto n) {
            if(r.planar_out)
                hipLaunchKernelGGL((lfi::blend_stdxa<true, decltype(n)::value, true>), grid, block, 0, stream_of(c), a, tiles_x, n_tiles);
            else
                hipLaunchKernelGGL((lfi::blend_stdxa<true, decltype(n)::value>), grid, block, 0, stream_of(c), a, tiles_x, n_tiles);
        });
    });
}

void launch_afs(const lfi_ctx *c, const KernelArgs &a_in, const BlendRoute &r)
{
    const int tiles_x = (a_in.width + lfi::AF_TPX - 1) / lfi::AF_TPX;
    const int n_tiles = tiles_x * a_in.out_rows;
    const dim3 grid(std::min(n_tiles, 2 * cu_count_of(c))), block(256);
    note_kernel(c, "blend_afs<STD,allfocus>");
    per_64_views(a_in, [&](const KernelArgs &a) {
        with_chunks<3>(r.nch, [&](auto n) {
            hipLaunchKernelGGL((lfi::blend_afs<true, decltype(n)::value>), grid, block, 0, stream_of(c), a, tiles_x, n_tiles);
        });
    });
}

void launch_p3(const lfi_ctx *c, const KernelArgs &a_in, int nch, bool rgba_out);

// deep_blend (flag = LFI_FLAG_DEEP_VIEWS: the byte planes and the deep planes), blend_inframe (LFI_FLAG_IN_FRAME: the byte planes, out-of-frame
// samples left out) or blend_linear (LFI_FLAG_LINEAR_LIGHT: the byte planes, blended in linear light) for views [v0, v1).  One chunk of images: ONE launch whose tiles serve every 64-view pass from the same LDS-resident pixels; several chunks: one
// launch per 64 views
void launch_tile16(const lfi_ctx *c, const KernelArgs &a_in, int nch, unsigned flag, bool std_chain)
{
    const bool deep = flag == LFI_FLAG_DEEP_VIEWS, linear = flag == LFI_FLAG_LINEAR_LIGHT;
    const int tiles_x = (a_in.width + lfi::P3_TPX - 1) / lfi::P3_TPX;
    const int n_tiles = tiles_x * a_in.out_rows;
    const dim3 grid(std::min(n_tiles, 2 * cu_count_of(c))), block(256);
    // what lfi_last_kernel_name reports.  Set here, not through the helper the other launchers use: tests/test_gpu_dispatch_coverage.py holds every
    // name that goes through it to a row of its render matrix, which knows no parameter flags; these launches are held to their names by
    // tests/test_gpu_deep.py, tests/test_gpu_inframe.py and tests/test_gpu_linear.py
    c->last_kernel = linear ? (std_chain ? "blend_linear<STD>" : "blend_linear<TEN_WM>")
                     : deep ? (std_chain ? "deep_blend<STD>" : "deep_blend<TEN_WM>") : (std_chain ? "blend_inframe<STD>" : "blend_inframe<TEN_WM>");
    auto launch = [&](const KernelArgs &a, int passes) {
        auto go = [&](auto kernel, auto... extra) { hipLaunchKernelGGL(kernel, grid, block, 0, stream_of(c), a, extra..., tiles_x, n_tiles, passes, nch); };
        if(deep && std_chain)
            go(lfi::deep_blend<true>, c->deep.get(), deep_pitch(c));
        else if(deep)
            go(lfi::deep_blend<false>, c->deep.get(), deep_pitch(c));
        else if(linear && std_chain)
            go(lfi::blend_linear<true>);
        else if(linear)
            go(lfi::blend_linear<false>);
        else if(std_chain)
            go(lfi::blend_inframe<true>);
        else
            go(lfi::blend_inframe<false>);
    };
    if(nch == 1)
        launch(a_in, (a_in.v1 - a_in.v0 + 63) / 64);
    else
        per_64_views(a_in, [&](const KernelArgs &a) { launch(a, 1); });
}

void launch_route(const lfi_ctx *c, const KernelArgs &a, bool all_focus, const BlendRoute &r)
{
    switch(r.kernel)
    {
        case BlendKernel::linear_ten: launch_tile16(c, a, r.nch, LFI_FLAG_LINEAR_LIGHT, false); break;
        case BlendKernel::linear_std: launch_tile16(c, a, r.nch, LFI_FLAG_LINEAR_LIGHT, true); break;
        case BlendKernel::inframe_ten: launch_tile16(c, a, r.nch, LFI_FLAG_IN_FRAME, false); break;
        case BlendKernel::inframe_std: launch_tile16(c, a, r.nch, LFI_FLAG_IN_FRAME, true); break;
        case BlendKernel::deep_ten: launch_tile16(c, a, r.nch, LFI_FLAG_DEEP_VIEWS, false); break;
        case BlendKernel::deep_std: launch_tile16(c, a, r.nch, LFI_FLAG_DEEP_VIEWS, true); break;
        case BlendKernel::ten_m16: launch_ten_m16(c, a, all_focus); break;
        case BlendKernel::ten_direct: launch_ten_direct(c, a, all_focus); break;
        case BlendKernel::p3: launch_p3(c, a, r.nch, false); break;
        case BlendKernel::p3_rgba: launch_p3(c, a, r.nch, true); break;
        case BlendKernel::planar_ten: launch_planar<false>(c, a); break;
        case BlendKernel::persist_ten:
        case BlendKernel::persist_ten_af: launch_persist<false>(c, a, all_focus, r.planar_out); break;
        case BlendKernel::wave_ten: launch_wave<false>(c, a); break;
        case BlendKernel::stdx: launch_stdx(c, a, r); break;
        case BlendKernel::planar_stdf: launch_planar<true>(c, a); break;
        case BlendKernel::stdxa: launch_stdxa(c, a, r); break;
        case BlendKernel::afs: launch_afs(c, a, r); break;
        case BlendKernel::persist_std:
        case BlendKernel::persist_std_af: launch_persist<true>(c, a, all_focus, false); break;
        case BlendKernel::wave_std: launch_wave<true>(c, a); break;
        case BlendKernel::std_mfma: launch_std_mfma(c, a, all_focus); break;
        case BlendKernel::std_valu: launch_std_valu(c, a, all_focus); break;
        case BlendKernel::std_vfma: launch_std_vfma(c, a, all_focus); break;
    }
}

int launch_blend(lfi_ctx *c, int method, int all_focus, const KernelArgs &a);

int check_render_args(lfi_ctx *c, int method, int v0, int v1)
{
    if(!c)
        return LFI_EINVAL;
    if(!c->grid && !c->inputs_released)
        return fail(c, LFI_EINVAL, "lfi_set_grid has not been called");
    if(!c->have_params)
        return fail(c, LFI_EINVAL, "lfi_set_params has not been called");
    if(method != LFI_METHOD_STD && method != LFI_METHOD_TEN_WM)
        return fail(c, LFI_EINVAL, "The specified interpolation method does not exist!");
    if(v0 < 0 || v1 > c->views_n || v0 >= v1)
        return fail(c, LFI_EINVAL, "view range [v0, v1) outside [0, views)");
    if(!c->views)
        return fail(c, LFI_EINVAL, "the context has no view buffer (a failed allocation: lfi_set_params again)");
    return LFI_OK;
}

// Consecutive launches over the same inputs (the reference's 100-launch loop, a trajectory streamed in blocks, a focus sweep) walk
// the tiles in opposite directions: the input rows a launch read last are the ones the next launch reads first, so part of them
// is still in the 256 MB Infinity Cache (config 2: −7 %, profiles/r02_p3_alternate.txt).  Same work, same bytes requested; fewer
// of them come from HBM.  LFI_FLAG_SINGLE_SWEEP_DIRECTION turns it off (every launch ascending, as a cold launch behaves).
int next_sweep_direction(const lfi_ctx *c)
{
    if(c->flags & LFI_FLAG_SINGLE_SWEEP_DIRECTION)
        return 0;
    return int(c->sweep_launches++ & 1u);
}


// Make the planar copy of the inputs valid for a fixed-focus launch with the current parameters; returns false (and leaves the
// launch on the RGBA planes) when the copy may not be used: inputs the library cannot track, absurd offsets.
// tune: also make the copy's per-image phases fit the CURRENT integer offsets (every 128-byte run of a tile then IS one cache line) — a
// rebuild.  lfi_prepare / lfi_benchmark ask for it; launch_blend asks once the same offsets have been rendered LFI_RETUNE_AFTER times (the
// reference's 100-launch loop, a trajectory streamed at one focus), so a fixed-focus sweep — new offsets every render — never pays a
// rebuild per render.  What stale phases cost such a sweep (round 5, profiles/r05_pmc_sweep_summary.txt, fixed_focus_sweep_*.txt): the
// launch takes 6–10 % longer (config 2: 137.6 → 151.2 µs, config 5: 1.44 → 1.53 ms) — twice the L1 tag accesses (a lane's 16-byte piece
// straddles sectors, a run two lines) and 9 % more bytes from HBM (boundary lines shared with the neighbouring tiles) — against a rebuild
// of 1.8 launches' time (0.25 ms at config 2): per-image phases cannot survive a change of -f (every image's offset moves by its own
// amount), so for one render per parameter set the stale copy is the cheaper choice; `also.config*_fixed_focus_sweep_step` times it.
// LFI_PLANAR_ALIGN: what the runs of the offsets in use are aligned to by the per-image phases — 128 (round 4): a tile's 128-byte run of
// an image row is then exactly ONE cache line (no boundary sectors fetched with the neighbouring tiles: the launches of several chunks
// over-fetched 10–19 %, profiles/r04_pmc_traffic_summary.txt); 4 = round 3's dword alignment.  Power of two, ≤ 128.
#ifndef LFI_PLANAR_ALIGN
#define LFI_PLANAR_ALIGN 128
#endif
// are the planar copy's per-image phases the ones that align the runs of the offsets in use?  (then no tile shares a cache line with its
// neighbours: LFI_KFLAG_PLAIN_TILE_ORDER, lfi_device.hpp)
bool planar_phases_tuned(const lfi_ctx *c)
{
    if(!c->planar || (int)c->planar_phase.size() != c->n)
        return false;
    for(int g = 0; g < c->n; g++)
        if((c->h_focused[g].x + c->planar_padx + c->planar_phase[g]) & (LFI_PLANAR_ALIGN - 1))
            return false;
    return true;
}

// min_reach: pad the copy for horizontal shifts up to this many pixels even where the current integer offsets reach less (the per-view
// offsets of lfi_set_view_offsets); 0 for every other caller
bool ensure_planar(lfi_ctx *c, bool tune = false, int min_reach = 0)
{
    if(!c->grid_tracked)
        return false;
    const int reach = std::max(std::max(std::abs(c->fo_min[0]), std::abs(c->fo_max[0])), min_reach);
    if(reach > 4 * c->width + 4096)
        return false;
    // a tile's 128-byte run starts up to `reach` pixels left of column 0 (left padding: reach, rounded up to whole dwords so that the
    // build's dword stores stay aligned) and, in the last tile of a row, ends up to `reach` pixels past the last tile's 128th pixel
    const bool valid = c->planar && c->planar_version == c->grid_version && c->planar_reach >= reach && (int)c->planar_phase.size() == c->n;
    if(valid && (!tune || planar_phases_tuned(c)))
        return true;
    if(c->inputs_released)
        return valid; // nothing to rebuild from: the copy serves the offsets it was built for (stale phases cost a launch 6–10 %), or the render is refused
    // the copy in place fits and only SOME images were replaced since it was brought up to date (lfi_upload_image, a partial fill): their
    // planes only — 1/N of a rebuild per image
    if(c->planar && c->planar_version != 0 && c->planar_reach >= reach && (int)c->planar_phase.size() == c->n &&
       c->grid_full_version <= c->planar_version && (!tune || planar_phases_tuned(c)))
    {
        for(int g = 0; g < c->n;)
        {
            if(!image_changed_since(c, g, c->planar_version))
            {
                g++;
                continue;
            }
            int g1 = g + 1;
            while(g1 < c->n && image_changed_since(c, g1, c->planar_version))
                g1++;
            hipLaunchKernelGGL(lfi::planar_build, dim3((c->planar_pitch / 4 + 255) / 256, c->in_rows, g1 - g), dim3(256), 0, c->stream,
                               c->grid.get(), c->planar.get(), c->width, c->in_rows, c->planar_pitch, c->planar_padx, c->d_planar_phase.as<int32_t>(), g);
            g = g1;
        }
        if(hipGetLastError() != hipSuccess)
            return false;
        c->planar_version = c->grid_version;
        return true;
    }
    // a copy that has to GROW (a sweep towards larger offsets) is padded for a quarter more than asked for: every growth is a rebuild, and
    // a reallocation of up to gigabytes if the planes no longer fit the allocation
    const int built_for = c->planar && reach > c->planar_reach ? reach + reach / 4 + 8 : std::max(reach, c->planar_reach);
    const int padx = (built_for + 3) / 4 * 4;
    const int tiles_w = (c->width + 127) / 128 * 128;
    constexpr int pitch_unit = LFI_PLANAR_ALIGN > 16 ? LFI_PLANAR_ALIGN : 16; // rows start on the alignment unit
    int pitch = (padx + (LFI_PLANAR_ALIGN - 1) + tiles_w + built_for + pitch_unit - 1) / pitch_unit * pitch_unit; // + the largest phase
    // (one more line per row where the pitch comes to a multiple of 2048 bytes — 8×8 @4K: exactly 4096 —, or an odd number of lines per row for
    // every shape: measured, ± 2 % either way by box: profiles/r04_planar_align_ab.txt)
#ifdef LFI_MEASUREMENT_BUILD // tools/plane_skew.py: do the 192 plane streams collide on HBM channels?  Extra bytes per plane row / per plane.
    static const int extra_pitch = [] { const char *e = std::getenv("LFI_PLANAR_EXTRA_PITCH"); return e ? std::atoi(e) : 0; }();
    pitch += extra_pitch / 16 * 16;
#endif
    // blend_p3 / blend_stdx address a row as row·pitch with a 24-bit multiply, and a lane's byte inside its octet of images (8 images
    // × 3 planes, plus the row and the run) with 32 bits
    if(c->in_rows >= (1 << 24) || pitch >= (1 << 24) || (uint64_t)26 * c->in_rows * pitch >= (1ull << 32))
        return false;
    const size_t bytes = (size_t)c->n * 3 * c->in_rows * pitch; // the rows this context holds (a row window: band + halo)
    bool fresh = false;
    const bool fits = c->planar.reserve(bytes, &fresh) == hipSuccess; // (a larger allocation serves smaller planes too)
    if(fresh)
        c->planar_version = 0;
    if(!fits || c->d_planar_phase.reserve(sizeof(int32_t) * LFI_MAX_IMAGES) != hipSuccess)
    {
        (void)hipGetLastError(); // not enough memory for the copy: render from the RGBA planes
        return false;
    }
    // the phases: (offset + padx + phase) ≡ 0 mod LFI_PLANAR_ALIGN for the offsets in use now.  They travel through the staging ring and a
    // stream-ordered copy (as lfi_set_params' blob does): kernels of earlier launches that read the old phases are ordered before the
    // copy, the build and every later launch after it, and the host never waits for the stream (round 3 copied from a pageable vector
    // and synchronised the stream inside lfi_render).
    int32_t *staged = nullptr;
    if(c->phase_ring.acquire(sizeof(int32_t) * LFI_MAX_IMAGES, &staged) != hipSuccess)
    {
        (void)hipGetLastError();
        return false;
    }
    c->planar_phase.assign(c->n, 0);
    for(int g = 0; g < c->n; g++)
        staged[g] = c->planar_phase[g] = (LFI_PLANAR_ALIGN - ((c->h_focused[g].x + padx) & (LFI_PLANAR_ALIGN - 1))) & (LFI_PLANAR_ALIGN - 1);
    c->planar_version = 0;
    if(hipMemcpyAsync(c->d_planar_phase.get(), staged, sizeof(int32_t) * c->n, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
       c->phase_ring.commit(c->stream) != hipSuccess)
        return false;
    c->planar_padx = padx;
    c->planar_reach = built_for;
    c->planar_pitch = pitch;
    hipLaunchKernelGGL(lfi::planar_build, dim3((pitch / 4 + 255) / 256, c->in_rows, c->n), dim3(256), 0, c->stream, c->grid.get(),
                       c->planar.get(), c->width, c->in_rows, pitch, padx, c->d_planar_phase.as<int32_t>(), 0);
    if(hipGetLastError() != hipSuccess)
        return false;
    c->planar_version = c->grid_version;
    return true;
}

// launch_blend's policy for the rebuild above.  A rebuild re-converts the whole copy (0.25 ms at config 2, ≈ 3 ms at config 5) for a 6–10 %
// gain per launch (14 µs at config 2, 0.09 ms at config 5): it pays for itself after ≈ 20–30 launches.  So a render only retunes once the same integer offsets have been rendered
// LFI_RETUNE_AFTER times (the reference's own loop is 100 launches over one parameter set, src/interpolator.cu:270-295; round 3 retuned
// at the third launch, a net loss for short runs); lfi_prepare and lfi_benchmark retune at once, outside any render.
constexpr unsigned LFI_RETUNE_AFTER = 32;
bool tune_planar_now(lfi_ctx *c)
{
    return c->launches_with_offsets++ >= LFI_RETUNE_AFTER;
}

// the derived copy's addressing, for a launch that reads it (ensure_planar has made it valid)
void set_planar_args(const lfi_ctx *c, KernelArgs &a)
{
    a.planar = c->planar.get();
    a.planar_pitch = c->planar_pitch;
    a.planar_padx = c->planar_padx;
    a.planar_phase = c->d_planar_phase.as<int32_t>(); // allocated by ensure_planar, possibly just now
}

// blend_p3 (TEN_WM from the planar copy): the planar views' epilogue, or (rgba_out: two to four chunks of images) the RGBA epilogue
void launch_p3(const lfi_ctx *c, const KernelArgs &a_in, int nch, bool rgba_out)
{
    const int tiles_x = (a_in.width + lfi::P3_TPX - 1) / lfi::P3_TPX;
    const int n_tiles = tiles_x * a_in.out_rows;
#ifdef LFI_MEASUREMENT_BUILD // LFI_P3_WGS = workgroups per CU in the grid (1 or 2): does a launch scale with the waves per CU?
    static const int wgs_env = [] { const char *e = std::getenv("LFI_P3_WGS"); return e ? std::atoi(e) : 2; }();
    const dim3 grid(std::min(n_tiles, wgs_env * cu_count_of(c))), block(256);
#else
    const dim3 grid(std::min(n_tiles, 2 * cu_count_of(c))), block(256);
#endif
    note_kernel(c, rgba_out ? "blend_p3<TEN_WM,rgba>" : "blend_p3<TEN_WM>");
#ifdef LFI_MEASUREMENT_BUILD
    // measurement builds only (make HIPFLAGS+=-DLFI_MEASUREMENT_BUILD, tools/p3_ablate.py): where does a unit's time go?  The ablated
    // kernels write garbage by construction, so the production library does not contain them and reads no such environment variable.
    static const int ablate = [] {
        const char *e = std::getenv("LFI_P3_ABLATE");
        return e ? std::atoi(e) : 0;
    }();
    if(ablate >= 1 && ablate <= 3 && ((nch == 1 && a_in.v1 - a_in.v0 <= 256) || (nch == 4 && a_in.v1 - a_in.v0 <= 64)))
    {
        note_kernel(c, "blend_p3<ABLATION>");
        const int abl_passes = nch == 1 ? (a_in.v1 - a_in.v0 + 63) / 64 : 1;
#define LFI_P3_ABL(N, A) hipLaunchKernelGGL((lfi::blend_p3<true, N, A, (N == 1 ? 1 : 2), (N == 1 ? 4 : 1)>), grid, dim3(N == 1 ? 256 : 128), 0, stream_of(c), a_in, tiles_x, n_tiles, abl_passes, 0)
        if(nch == 1)
        {
            if(ablate == 1) LFI_P3_ABL(1, 1); else if(ablate == 2) LFI_P3_ABL(1, 2); else LFI_P3_ABL(1, 3);
        }
        else
        {
            if(ablate == 1) LFI_P3_ABL(4, 1); else if(ablate == 2) LFI_P3_ABL(4, 2); else LFI_P3_ABL(4, 3);
        }
#undef LFI_P3_ABL
        return;
    }
#endif
    const int reverse = next_sweep_direction(c);
    // Views per wave: 16 (four waves per workgroup, two per SIMD) when the launch is paced by its memory pipeline — one chunk of
    // images — and 32 (two waves per workgroup, one per SIMD, the pixel operand built once for two MFMAs) when several chunks make the
    // k-loop the pacer (15×15 grids: −13 % at 4K, profiles/r02_p3_vg.txt).  Measurement builds: LFI_P3_VG = 1 / 2 forces either (tools/p3_vg.py).
#ifdef LFI_MEASUREMENT_BUILD
    static const int vg_env = [] {
        const char *e = std::getenv("LFI_P3_VG");
        return e ? std::atoi(e) : 0;
    }();
#endif
    const dim3 block2(128);
    if(nch == 1)
    {
        // one chunk of images: every 64-view pass of a tile reads the same LDS-resident pixels — the inputs are fetched once per
        // 256 views (four passes: the weight fragments a wave keeps in registers)
        int launch_no = 0;
        for(int v0 = a_in.v0; v0 < a_in.v1; v0 += 256, launch_no++)
        {
            KernelArgs a = a_in;
            a.v0 = v0;
            a.v1 = std::min(v0 + 256, a_in.v1);
            const int passes = (a.v1 - a.v0 + 63) / 64;
            const int dir = reverse ^ (launch_no & 1);
#ifdef LFI_MEASUREMENT_BUILD
            if(vg_env == 2 && passes == 1)
            {
                hipLaunchKernelGGL((lfi::blend_p3<true, 1, 0, 2>), grid, block2, 0, stream_of(c), a, tiles_x, n_tiles, 1, dir);
                continue;
            }
#endif
            // (one chunk of images: the planar views' epilogue only — route_blend keeps blend_planar for RGBA views there)
            if(passes == 1)
                hipLaunchKernelGGL((lfi::blend_p3<true, 1>), grid, block, 0, stream_of(c), a, tiles_x, n_tiles, 1, dir);
            else
                hipLaunchKernelGGL((lfi::blend_p3<true, 1, 0, 1, 4>), grid, block, 0, stream_of(c), a, tiles_x, n_tiles, passes, dir);
        }
        return;
    }
    per_64_views(a_in, [&](const KernelArgs &a) {
        with_chunks<2>(nch, [&](auto n) {
            constexpr int N = decltype(n)::value;
#ifdef LFI_MEASUREMENT_BUILD
            if(vg_env == 1)
            {
                hipLaunchKernelGGL((lfi::blend_p3<true, N, 0, 1>), grid, block, 0, stream_of(c), a, tiles_x, n_tiles, 1, reverse);
                return;
            }
#endif
            if(rgba_out)
                hipLaunchKernelGGL((lfi::blend_p3<true, N, 0, 2, 1, true>), grid, block2, 0, stream_of(c), a, tiles_x, n_tiles, 1, reverse);
            else
                hipLaunchKernelGGL((lfi::blend_p3<true, N, 0, 2>), grid, block2, 0, stream_of(c), a, tiles_x, n_tiles, 1, reverse);
        });
    });
}

// per-view rows (lfi_set_view_offsets / lfi_set_view_float_offsets) and which of them govern a render: the float rows an all-focus one,
// when set; otherwise the integer rows, when set (which refuse all-focus renders: view_rows_ready)
enum ViewRowsKind { VIEW_ROWS_NONE, VIEW_ROWS_INT, VIEW_ROWS_FLOAT };

ViewRowsKind view_rows_of(const lfi_ctx *c, int all_focus)
{
    if(all_focus && c->view_float_offsets.set)
        return VIEW_ROWS_FLOAT;
    return c->view_offsets.set ? VIEW_ROWS_INT : VIEW_ROWS_NONE;
}

// the start of the message of every render the rows refuse
std::string view_rows_set(ViewRowsKind k)
{
    return k == VIEW_ROWS_INT ? "per-view offsets are set (lfi_set_view_offsets): " : "per-view float offsets are set (lfi_set_view_float_offsets): ";
}

int launch_view_rows(lfi_ctx *c, ViewRowsKind k, int method, int all_focus, const KernelArgs &a_in);

// Every image row an all-focus render of the output band can sample is held: (int)fma(f, offset.y, y) for f between the ends of the focus
// range (the map decodes to focus + m/255·range), y in the band, over the n offsets o; ±1 for float rounding
bool allfocus_rows_held(const lfi_ctx *c, const lfi_float2 *o, size_t n)
{
    const float f_lo = std::min(c->focus, c->focus + c->range), f_hi = std::max(c->focus, c->focus + c->range);
    const int H = c->height;
    for(size_t g = 0; g < n; g++)
    {
        const double d_lo = std::min((double)f_lo * o[g].y, (double)f_hi * o[g].y), d_hi = std::max((double)f_lo * o[g].y, (double)f_hi * o[g].y);
        const int lo = std::min(std::max((int)std::floor(c->out_y0 + d_lo) - 1, 0), H - 1);
        const int hi = std::min(std::max((int)std::ceil(c->out_y0 + c->out_rows - 1 + d_hi) + 1, 0), H - 1);
        if(lo < c->in_y0 || hi >= c->in_y0 + c->in_rows)
            return false;
    }
    return true;
}

// ---- the flagged fixed-focus renders: deep views (LFI_FLAG_DEEP_VIEWS, deep_blend.hpp), in-frame blending (LFI_FLAG_IN_FRAME, blend_inframe.hpp),
// linear-light blending (LFI_FLAG_LINEAR_LIGHT, blend_linear.hpp) ----------------------------------------------------------------------------

const char *const kDeepNoPrequant = "lfi_download_prequant is not supported (the deep planes ARE the accumulator's ten bits)";
const char *const kInFrameNoPrequant = "lfi_download_prequant is not supported";
const char *const kLinearNoPrequant = "lfi_download_prequant is not supported";

const char *flag_name(unsigned flag)
{
    return flag == LFI_FLAG_DEEP_VIEWS ? "LFI_FLAG_DEEP_VIEWS" : flag == LFI_FLAG_IN_FRAME ? "LFI_FLAG_IN_FRAME" : "LFI_FLAG_LINEAR_LIGHT";
}

// What a render under `flag` (LFI_FLAG_DEEP_VIEWS, LFI_FLAG_IN_FRAME or LFI_FLAG_LINEAR_LIGHT) refuses, before anything is enqueued or allocated; every message names
// the flag
int flagged_refused(lfi_ctx *c, unsigned flag, int all_focus, const KernelArgs &a)
{
    const bool deep = flag == LFI_FLAG_DEEP_VIEWS, linear = flag == LFI_FLAG_LINEAR_LIGHT;
    const char *why = nullptr;
    if(linear && (c->flags & LFI_FLAG_DEEP_VIEWS))
        why = "LFI_FLAG_DEEP_VIEWS is not supported together with it (no deep linear-light views)";
    else if(linear && (c->flags & LFI_FLAG_IN_FRAME))
        why = "LFI_FLAG_IN_FRAME is not supported together with it (no in-frame linear-light blending)";
    else if(!deep && !linear && (c->flags & LFI_FLAG_DEEP_VIEWS))
        why = "LFI_FLAG_DEEP_VIEWS is not supported together with it (no deep in-frame views)";
    else if(a.prequant)
        why = deep ? kDeepNoPrequant : linear ? kLinearNoPrequant : kInFrameNoPrequant;
    else if(all_focus)
        why = "all-focus renders are not supported (fixed focus only)";
    else if(c->view_offsets.set || c->view_float_offsets.set)
        why = "per-view rows (lfi_set_view_offsets, lfi_set_view_float_offsets) are not supported - clear them with NULL";
    else if(c->windowed)
        why = "a row window (lfi_set_row_window) is not supported";
    else if(c->out_layout != LFI_LAYOUT_PLANAR_RGB)
        why = "the RGBA view layout is not supported - lfi_set_output_layout(LFI_LAYOUT_PLANAR_RGB)";
    else if(c->flags & LFI_FLAG_TEN_ROUND_PER_BATCH)
        why = "LFI_FLAG_TEN_ROUND_PER_BATCH is not supported";
    else if(!c->weights_scalable)
        why = "weights outside [0, 2) are not supported";
    return why ? fail(c, LFI_EINVAL, std::string(flag_name(flag)) + " is set: " + why) : LFI_OK;
}

// the deep planes of all views_n views; a first use (or a new size) allocates, which may block
int ensure_deep_planes(lfi_ctx *c)
{
    const size_t need = deep_bytes(c);
    if(c->deep.bytes() == need)
        return LFI_OK;
    LFI_HIP(c, hipStreamSynchronize(c->stream)); // a download may still read the planes that go
    drop_deep_range(c);
    LFI_HIP(c, c->deep.fit(need));
    return LFI_OK;
}

// lfi_render / lfi_prepare's build / lfi_benchmark while `flag` is set: deep_blend writes the byte planes and the deep planes of [v0, v1),
// blend_inframe and blend_linear the byte planes.  The order of the steps decides what is allocated or dropped before a refusal
int launch_flagged_views(lfi_ctx *c, unsigned flag, int method, int all_focus, const KernelArgs &a_in)
{
    const bool deep = flag == LFI_FLAG_DEEP_VIEWS;
    if(method != LFI_METHOD_STD && method != LFI_METHOD_TEN_WM) // the reference throws here (src/interpolator.cu:289-290)
        return fail(c, LFI_EINVAL, "The specified interpolation method does not exist!");
    if(int rc = flagged_refused(c, flag, all_focus, a_in))
        return rc;
    if(int rc = join_uploads(c))
        return rc;
    if(!ensure_planar(c, tune_planar_now(c)))
        return fail(c, LFI_EINVAL, std::string(flag_name(flag)) +
                                       " is set: the planar copy of the inputs cannot serve these offsets (inputs the library cannot track, "
                                       "or, after lfi_release_inputs, offsets beyond the copy's padding)");
    if(deep)
        if(int rc = ensure_deep_planes(c))
            return rc;
    KernelArgs a = a_in;
    set_planar_args(c, a);
    drop_deep_range(c); // in-frame, linear light: the views are written without their deep planes
    launch_route(c, a, false, route_blend(c, method, false, a, true));
    LFI_HIP(c, hipGetLastError());
    if(deep)
        c->deep_v0 = a.v0, c->deep_v1 = a.v1;
    return LFI_OK;
}

// Renders views [a_in.v0, a_in.v1) into a_in.views
int launch_blend(lfi_ctx *c, int method, int all_focus, const KernelArgs &a_in)
{
    if(c->flags & LFI_FLAG_LINEAR_LIGHT) // (with one of the other two beside it: refused there)
        return launch_flagged_views(c, LFI_FLAG_LINEAR_LIGHT, method, all_focus, a_in);
    if(c->flags & LFI_FLAG_IN_FRAME) // (with LFI_FLAG_DEEP_VIEWS beside it: refused there)
        return launch_flagged_views(c, LFI_FLAG_IN_FRAME, method, all_focus, a_in);
    if(c->flags & LFI_FLAG_DEEP_VIEWS)
        return launch_flagged_views(c, LFI_FLAG_DEEP_VIEWS, method, all_focus, a_in);
    if(int rc = join_uploads(c))
        return rc;
    if(const ViewRowsKind k = view_rows_of(c, all_focus))
        return launch_view_rows(c, k, method, all_focus, a_in);
    if(all_focus && a_in.map_index == 1)
        if(int rc = join_filter(c)) // the filtered map may still be in the making on the side stream
            return rc;
    if(method == LFI_METHOD_STD && a_in.k_pad > 64 && c->weights_scalable && c->weights_sum_ok && !a_in.prequant && !(a_in.flags & LFI_FLAG_STD_ANALYTIC_BAND))
    {
        // more than 64 images: the band's measured bound must hold on THIS device (lfi_band_probe.hpp: measured once per device)
        bool forced = false;
        if(int rc = std_band_forced_analytic(c, &forced))
            return rc;
        if(forced)
        {
            KernelArgs a = a_in;
            a.flags |= LFI_FLAG_STD_ANALYTIC_BAND;
            return launch_blend(c, method, all_focus, a);
        }
    }
    if(method != LFI_METHOD_STD && method != LFI_METHOD_TEN_WM) // the reference throws here (src/interpolator.cu:289-290)
        return fail(c, LFI_EINVAL, "The specified interpolation method does not exist!");
    BlendRoute r = route_blend(c, method, all_focus != 0, a_in, true);
    if(r.reads_copy && !ensure_planar(c, tune_planar_now(c)))
        r = route_blend(c, method, all_focus != 0, a_in, false); // the copy may not be used: the same render from the RGBA planes
    if(c->inputs_released && !r.reads_copy)
        return fail(c, LFI_EINVAL, "the RGBA inputs were released (lfi_release_inputs): only fixed-focus renders whose offsets the planar copy was built for "
                                   "are served (no all-focus render, debug mode, weights outside [0, 2) or larger offsets) - upload the images again");
    if(c->windowed)
    {
        // a row window is honoured by the persistent kernels only (and the per-batch rounding mode refused for either method)
        if(generic_kernel(r.kernel) || (c->flags & LFI_FLAG_TEN_ROUND_PER_BATCH))
            return fail(c, LFI_EINVAL, "with a row window only renders with the default (persistent) kernels and weights in [0,2) are supported");
        if(all_focus && !allfocus_rows_held(c, c->h_offsets.data(), c->h_offsets.size()))
            return fail(c, LFI_EINVAL, "the input row window does not cover the rows an all-focus render of this band samples");
    }
    KernelArgs a = a_in;
    if(r.reads_copy)
    {
        set_planar_args(c, a);
        if(planar_phases_tuned(c))
            a.flags |= lfi::LFI_KFLAG_PLAIN_TILE_ORDER;
    }
    if(all_focus)
        a.flags |= lfi::LFI_KFLAG_PLAIN_TILE_ORDER; // per-pixel gathers: no lines shared between neighbouring tiles by construction
    // planar views from a kernel that writes RGBA only: into a scratch copy of the views, converted to byte planes afterwards
    const bool scratch = c->out_layout == LFI_LAYOUT_PLANAR_RGB && !r.planar_out;
    if(scratch)
    {
        LFI_HIP(c, c->rgba_scratch.fit(rgba_out_plane_bytes(c) * c->views_n)); // nothing happens from the second launch on
        a.views = c->rgba_scratch.get();
    }
    if(!a.prequant)
        drop_deep_range(c); // the views are written without their deep planes
    launch_route(c, a, all_focus != 0, r);
    LFI_HIP(c, hipGetLastError());
    if(scratch)
    {
        const int pitch = view_pitch(c);
        hipLaunchKernelGGL(lfi::views_rgba_to_planar, dim3((pitch / 4 + 255) / 256, c->out_rows, a.v1 - a.v0), dim3(256), 0, c->stream,
                           reinterpret_cast<const uint32_t *>(c->rgba_scratch.get() + rgba_out_plane_bytes(c) * a.v0), a_in.views + out_plane_bytes(c) * a.v0,
                           c->width, c->out_rows, pitch);
        LFI_HIP(c, hipGetLastError());
    }
    return LFI_OK;
}

// ---- per-view rows (lfi_set_view_offsets / lfi_set_view_float_offsets): blend_vfocus.hpp, blend_vfocus_af.hpp ---------------------------

// Can this render be served from the per-view rows k?  Neither kind serves debug modes.  Integer rows: fixed focus only, after
// lfi_release_inputs only from a planar copy padded for every per-view shift; *planar: read the planar copy (made valid here for the
// per-view shifts) rather than the RGBA planes.  Float rows: the RGBA planes present, every row that views [v0, v1) sample held.
int view_rows_ready(lfi_ctx *c, ViewRowsKind k, int all_focus, const KernelArgs &a, bool *planar)
{
    *planar = false;
    if(k == VIEW_ROWS_INT && all_focus)
        return fail(c, LFI_EINVAL, view_rows_set(k) + "all-focus renders are not supported - clear them with NULL");
    if(a.prequant)
        return fail(c, LFI_EINVAL, view_rows_set(k) + "lfi_download_prequant is not supported - clear them with NULL");
    if(c->flags & LFI_FLAG_TEN_ROUND_PER_BATCH)
        return fail(c, LFI_EINVAL, view_rows_set(k) + "LFI_FLAG_TEN_ROUND_PER_BATCH is not supported");
    if(k == VIEW_ROWS_INT)
    {
        *planar = ensure_planar(c, false, c->view_offsets_reach);
        if(c->inputs_released && !*planar)
            return fail(c, LFI_EINVAL, "the RGBA inputs were released (lfi_release_inputs) and the planar copy's padding does not cover the per-view "
                                       "offsets - upload the images again");
        return LFI_OK;
    }
    if(c->inputs_released)
        return fail(c, LFI_EINVAL, "the RGBA inputs were released (lfi_release_inputs): all-focus renders need them - upload the images again");
    if(c->windowed)
        for(int v = a.v0; v < a.v1; v++)
            if(!allfocus_rows_held(c, c->h_view_float_offsets.data() + (size_t)v * c->n, c->n))
                return fail(c, LFI_EINVAL, "the input row window does not cover the rows an all-focus render of this band samples in view " +
                                               std::to_string(v));
    return LFI_OK;
}

// blend_vfocus (integer rows) or blend_vfocus_af (float rows; with per-view maps its view_maps variant) over views [a.v0, a.v1)
int launch_view_rows(lfi_ctx *c, ViewRowsKind k, int method, int all_focus, const KernelArgs &a_in)
{
    bool planar = false;
    if(int rc = view_rows_ready(c, k, all_focus, a_in, &planar))
        return rc;
    // per-view maps (lfi_view_focus_maps): each view reads its own pair, made on the compute stream
    const bool view_maps = k == VIEW_ROWS_FLOAT && c->view_maps_set;
    if(k == VIEW_ROWS_FLOAT && a_in.map_index == 1 && !view_maps)
        if(int rc = join_filter(c)) // the filtered map may still be in the making on the side stream
            return rc;
    KernelArgs a = a_in;
    if(view_maps)
        a.maps = c->view_maps.get();
    if(planar)
        set_planar_args(c, a);
    const bool ten = method == LFI_METHOD_TEN_WM, planar_out = c->out_layout == LFI_LAYOUT_PLANAR_RGB;
    const int chunk_views = view_maps ? lfi::VM_VIEWS : lfi::VF_VIEWS;
    const int n_chunks = (a.v1 - a.v0 + chunk_views - 1) / chunk_views;
    const int tiles_x = (c->width + lfi::VF_TILE_W - 1) / lfi::VF_TILE_W;
    const int tiles_y = (c->out_rows + lfi::VF_ROWS - 1) / lfi::VF_ROWS;
    const size_t blocks = (size_t)n_chunks * tiles_x * tiles_y;
    if(blocks >= (1ull << 31))
        return fail(c, LFI_EINVAL, view_rows_set(k) + "too many views x pixels for one launch - render the views in ranges");
    static const char *const names[4][2] = {{"blend_vfocus<STD,rgba_src>", "blend_vfocus<TEN_WM,rgba_src>"},
                                            {"blend_vfocus<STD>", "blend_vfocus<TEN_WM>"},
                                            {"blend_vfocus_af<STD>", "blend_vfocus_af<TEN_WM>"},
                                            {"blend_vfocus_af<STD,view_maps>", "blend_vfocus_af<TEN_WM,view_maps>"}};
    note_kernel(c, names[view_maps ? 3 : k == VIEW_ROWS_FLOAT ? 2 : planar][ten]);
    drop_deep_range(c); // the views are written without their deep planes
    if(k == VIEW_ROWS_INT)
    {
        using lfi::blend_vfocus;
        static const decltype(&blend_vfocus<false, false, false>) kernels[2][2][2] = {
            {{blend_vfocus<false, false, false>, blend_vfocus<false, false, true>}, {blend_vfocus<false, true, false>, blend_vfocus<false, true, true>}},
            {{blend_vfocus<true, false, false>, blend_vfocus<true, false, true>}, {blend_vfocus<true, true, false>, blend_vfocus<true, true, true>}}};
        hipLaunchKernelGGL(kernels[ten][planar][planar_out], dim3((unsigned)blocks), dim3(256), 0, stream_of(c), a, c->view_offsets.rows(),
                           c->view_offsets.pitch, n_chunks, tiles_x);
    }
    else
    {
        using lfi::blend_vfocus_af;
        using lfi::VF_VIEWS;
        using lfi::VM_VIEWS;
        static const decltype(&blend_vfocus_af<false, false>) kernels[2][2][2] = {
            {{blend_vfocus_af<false, false>, blend_vfocus_af<false, true>}, {blend_vfocus_af<true, false>, blend_vfocus_af<true, true>}},
            {{blend_vfocus_af<false, false, VM_VIEWS, true>, blend_vfocus_af<false, true, VM_VIEWS, true>},
             {blend_vfocus_af<true, false, VM_VIEWS, true>, blend_vfocus_af<true, true, VM_VIEWS, true>}}};
        hipLaunchKernelGGL(kernels[view_maps][ten][planar_out], dim3((unsigned)blocks), dim3(256), 0, stream_of(c), a, c->view_float_offsets.rows(),
                           c->view_float_offsets.pitch, n_chunks, tiles_x);
    }
    LFI_HIP(c, hipGetLastError());
    return LFI_OK;
}

} // namespace
