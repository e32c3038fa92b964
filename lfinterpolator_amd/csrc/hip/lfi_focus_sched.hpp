// lfi_focus_sched.hpp — scheduling of the focus-map estimate: the factored pipeline's workspace and its two-stream pass graph
// (focus_factored.hpp), and the choice between it, the row-window path and the other estimate variants; the focus curve's workspace and
// its three launches (focus_curve.hpp); the focus tiles' pass behind the factored estimate (focus_tiles.hpp).
// Replaces the FocusMap::estimate / FocusMap::filter launches (reference src/interpolator.cu:261-266).
// Included by lfi_hip.hip only (one translation unit), after lfi_context.hpp.
#pragma once

#include "lfi_context.hpp"
#include "focus_factored.hpp"
#include "focus_curve.hpp"
#include "focus_tiles.hpp"

namespace {

// What one factored estimate samples: the host copies of the sampled images' offsets and ids, in pad-slot order (slot k is padded from image
// ids[k]); the device arrays are the caller's a.offsets / a.focus_ids / a.maps.  The centre map (lfi_focus_map) is ctx->h_focus_offsets /
// h_focus_ids; a per-view batch (lfi_view_focus_maps) passes each view's, with the padding sized for the whole batch.
struct FocusJob
{
    const lfi_float2 *offsets = nullptr; // [n_ids]: offsets[k] of image ids[k]
    const int32_t *ids = nullptr;        // [n_ids]
    int n_ids = 0;
    int need_shift[2] = {0, 0}; // padding asked for on top of this job's own shifts (a batch's bound over all its views)
    // slot-stable re-padding: planes of the right geometry are kept slot by slot — only slots whose image differs from pad_ids (or has
    // changed since) are padded.  Off (the centre map): the planes are kept only when pad_ids equals ids as a whole, else all are re-padded.
    bool slot_reuse = false;
    int padded = 0; // out: focus_pad slots enqueued
};

// lfi_focus_route_info's record: an estimate call that has passed its checks starts a new one; the launches below note into ctx->route what
// they choose, each at the place where it is chosen (as note_kernel does for the blend)
void route_begin(lfi_ctx *ctx)
{
    const int32_t calls = ctx->route.calls;
    ctx->route = lfi_focus_route{calls + 1, 0, "", "", 0, 0, "", "", 0, 0, 0, {0, 0}, 0, 0, 0, 0, 0, 0, {0}, {0}, {0}};
}
static_assert(LFI_FOCUS_ROUTE_PASSES == lfi::FOCUS_MAX_PASSES, "lfi_focus_route holds one entry per pass of the longest sweep");

// largest |shift| any candidate gives any of the n offsets, +1 (candidates are monotone in i, so the ends bound them); false when absurd.
// The bound is the INTERVAL's: the last candidate of every sweep length lfi_set_focus_steps allows (they differ by a rounding of
// fma(range / (steps − 1), steps − 1, focus) at most), so a change of the number of candidates alone never asks for other planes.
bool focus_pad_shift(const lfi_ctx *ctx, const lfi_float2 *offsets, int n, int *Sx, int *Sy)
{
    double fmax = std::fabs((double)ctx->focus);
    for(int steps = lfi::FOCUS_STEPS; steps <= lfi::FOCUS_STEPS * lfi::FOCUS_MAX_PASSES; steps += lfi::FOCUS_STEPS)
        fmax = std::max(fmax, std::fabs((double)lfi::focus_sweep_value(ctx->focus, ctx->range, float(steps - 1), steps - 1)));
    double ox = 0, oy = 0;
    for(int k = 0; k < n; k++)
    {
        ox = std::max(ox, std::fabs((double)offsets[k].x));
        oy = std::max(oy, std::fabs((double)offsets[k].y));
    }
    if(!(fmax * ox < 1e6 && fmax * oy < 1e6))
        return false;
    *Sx = (int)std::ceil(fmax * ox) + 1, *Sy = (int)std::ceil(fmax * oy) + 1; // ≥ |floor(δ)| and ≥ |floor(δ)+1|
    return true;
}

// the factored estimate (focus_factored.hpp) up to and including focus_line_keys: carve the workspace, then plan → pad → E → exact keys.
// Behind it the workspace *w_out holds E for every candidate and K for every flagged (pixel, candidate) pair; the consumer — the pick
// (launch_focus_pick) or the tile costs (launch_focus_tiles) — is enqueued next on the compute stream.
// Returns LFI_OK with *done = false when the padded planes would be unreasonably large (the caller takes another variant).
// direct_range: the range pass by focus_range (rounds 1-4's kernel: every use loads and widens its own samples) even where focus_range_t
// applies (variant "factored_direct": the second implementation in the parity tests, and the A/B partner)
// *e_32bit_out: a candidate's plane of E lies behind one buffer descriptor (focus_pick_sep)
// The call covers the 32 candidates from a.focus_i0 of a sweep of a.focus_steps (one PASS; 0 of 32 everywhere but lfi_focus_map under
// lfi_set_focus_steps and lfi_focus_tiles_steps).  A sweep's later passes (a.focus_i0 > 0) follow its first on the same streams: the padded planes and the geometry
// are the first pass's — nothing is padded, whatever the bookkeeping says — while the plan, E, Er, Ec and K are rewritten.  Ordering: the
// side stream's writers of pass g + 1 wait for ev_fork, recorded on the compute stream behind pass g's line keys and pick — or whatever the caller enqueued in the pick's place: everything on
// that stream so far — (and the new plan);
// the compute stream's line keys and pick of pass g wait for ev_join, behind the side stream's passes — each pass's readers are done before
// the next one's writers start, on either stream.
int launch_focus_factored_keys(lfi_ctx *ctx, const KernelArgs &a, FocusJob &job, bool *done, bool direct_range, lfi::FocusWork *w_out, bool *e_32bit_out)
{
    *done = false;
    const bool later_pass = a.focus_i0 > 0;
    if(!later_pass)
        job.padded = 0;
    const int W = ctx->width, H = ctx->height, rx = ctx->radius[0], ry = ctx->radius[1];
    const int n_ids = job.n_ids;
    lfi::FocusWork w{};
    w.We_p = (W + 2 * rx + 255) / 256 * 256;
    w.He_p = (H + 2 * ry + 3) / 4 * 4;
    int Sx = 0, Sy = 0;
    if(!focus_pad_shift(ctx, job.offsets, n_ids, &Sx, &Sy))
    {
        ctx->route.declined = "shift";
        return LFI_OK;
    }
    Sx = std::max(Sx, job.need_shift[0]);
    Sy = std::max(Sy, job.need_shift[1]);
    // The padded planes of an earlier call serve this one if the inputs have not changed since and their padding covers these shifts
    // (any larger padding gives the same samples): then the geometry is theirs.  New planes are padded to the next multiple of 8, so
    // that the neighbouring steps of a focus sweep find them large enough.
    // (also when only SOME images were replaced since — lfi_upload_image —: then only the planes of the sampled images among them are redone)
    const bool same_ids = job.slot_reuse ? ctx->pad_ids.size() == (size_t)n_ids : ctx->pad_ids == std::vector<int32_t>(job.ids, job.ids + n_ids);
    const bool pad_kept = later_pass || (ctx->grid_tracked && ctx->focus_ws && ctx->pad_version != 0 && ctx->grid_full_version <= ctx->pad_version &&
                                         same_ids && ctx->pad_radius[0] == rx && ctx->pad_radius[1] == ry && ctx->pad_shift[0] >= Sx &&
                                         ctx->pad_shift[1] >= Sy);
    // Planes that have to GROW (an ascending sweep) grow by a quarter more than asked for: every change of the geometry rebuilds the planes
    // and may reallocate a workspace of gigabytes (≈ 80 ms per step when it happened on every step of a sweep).
    auto padded = [](const int need, const int had) { return ((had > 0 && need > had ? need + need / 4 : need) + 7) / 8 * 8; };
    Sx = pad_kept ? ctx->pad_shift[0] : padded(Sx, ctx->pad_shift[0]);
    Sy = pad_kept ? ctx->pad_shift[1] : padded(Sy, ctx->pad_shift[1]);
    w.Px = Sx + rx;
    w.Py = Sy + ry;
    w.Wp = (w.Px + std::max(W + Sx + rx, w.We_p - rx + Sx) + 3) / 4 * 4;
    w.Hp = w.Py + std::max(H + Sy + ry, w.He_p - ry + Sy);
    // (+ FRT_PR + 16 rows of slack behind the last plane: focus_range_t fetches whole patches, also for the rows of its last tiles that
    // lie below the extended image)
    const size_t pad_bytes = sizeof(uint32_t) * ((size_t)n_ids * w.Hp + lfi::FRT_PR + 16) * w.Wp;
    if(pad_bytes > ((size_t)16 << 30))
    {
        ctx->route.declined = "planes";
        return LFI_OK;
    }
    // Can the range pass unpack its samples once into LDS (focus_range_t)?  Within every group of CPW consecutive candidates a view's integer
    // shifts — the device's own, by the helper it shares with this check (focus_group_fits) — must span at most FRT_MAX_DX pixels and FRT_MAX_DY
    // rows: groups of 8 candidates if that holds, else groups of 4, else focus_range.  Typed loads address the planes with 32 bits.
    int range_cpw = 0;
    if(!direct_range && pad_bytes < ((size_t)1 << 32))
        for(int cpw : {8, 4})
        {
            bool fits = true;
            for(int k = 0; k < n_ids && fits; k++)
                for(int i0 = 0; i0 < lfi::FOCUS_STEPS && fits; i0 += cpw)
                    fits = lfi::focus_group_fits(a.focus, a.range, a.focus_div, a.focus_i0 + i0, cpw, job.offsets[k]);
            if(fits)
            {
                range_cpw = cpw;
                break;
            }
        }
    size_t at = 0;
    auto carve = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) / 256 * 256;
        return here;
    };
    const size_t o_shifts = carve(sizeof(int32_t) * 4 * lfi::FOCUS_STEPS * lfi::FOCUS_MAX_IDS);
    const size_t o_badx = carve(sizeof(uint32_t) * W), o_bady = carve(sizeof(uint32_t) * H);
    const size_t o_tapx = carve(sizeof(uint32_t) * 3 * W), o_tapy = carve(sizeof(uint32_t) * 3 * H); // cleared with badx / bady: adjacent
    const size_t o_cols = carve(sizeof(uint16_t) * lfi::FOCUS_STEPS * W), o_rows = carve(sizeof(uint16_t) * lfi::FOCUS_STEPS * H);
    const size_t o_ncols = carve(sizeof(int32_t) * lfi::FOCUS_STEPS), o_nrows = carve(sizeof(int32_t) * lfi::FOCUS_STEPS);
    // (behind the three tables, prefix[100 … 115]: the two totals of each pass of a sweep, [FOCUS_MAX_PASSES][2], for lfi_focus_route_info)
    const size_t o_prefix = carve(sizeof(uint32_t) * (lfi::FOCUS_ROUTE_COUNTS + 2 * lfi::FOCUS_MAX_PASSES));
    const size_t o_rowbase = carve(sizeof(uint32_t) * H), o_colbase = carve(sizeof(uint32_t) * (W + 1));
    // line buffers for 4× the typical number of flagged rows / columns (three bands of r per candidate ≈ 0.03·H each);
    // anything beyond takes the tap-by-tap path
    w.R_cap = 4 * H;
    w.C_cap = 4 * W;
    const size_t o_Er = carve(sizeof(uint16_t) * (size_t)w.R_cap * 3 * w.We_p);
    const size_t o_Ec = carve(sizeof(uint16_t) * (size_t)w.C_cap * 3 * w.He_p);
    const size_t o_E = carve(sizeof(uint16_t) * lfi::FOCUS_STEPS * (size_t)w.He_p * w.We_p);
    const size_t o_K = carve(sizeof(uint16_t) * lfi::FOCUS_STEPS * (size_t)H * W);
    const size_t o_deltas = carve(sizeof(int64_t) * lfi::FOCUS_STEPS * lfi::FOCUS_MAX_IDS);
    const size_t o_patches = carve(sizeof(lfi::FocusPatch) * (lfi::FOCUS_STEPS / 4) * lfi::FOCUS_MAX_IDS);
    // the carry plane of a sweep of several passes (focus_pick_store).  Its room is carved whatever the sweep's length — in front of the padded
    // planes, whose place in the workspace a change of lfi_set_focus_steps must not move — and touched only by such a sweep.
    const size_t o_carry = carve(sizeof(uint32_t) * (size_t)H * W);
    const size_t o_pad = carve(pad_bytes);
    bool fresh = false;
    const hipError_t focus_ws_reserve = ctx->focus_ws.reserve(at, &fresh); // a larger workspace serves smaller geometries too
    if(fresh)
        ctx->pad_version = 0;
    LFI_HIP(ctx, focus_ws_reserve);
    uint8_t *base = ctx->focus_ws.get();
    w.shifts = reinterpret_cast<int32_t *>(base + o_shifts);
    w.badx = reinterpret_cast<uint32_t *>(base + o_badx);
    w.bady = reinterpret_cast<uint32_t *>(base + o_bady);
    w.tapx = reinterpret_cast<uint32_t *>(base + o_tapx);
    w.tapy = reinterpret_cast<uint32_t *>(base + o_tapy);
    w.cols = reinterpret_cast<uint16_t *>(base + o_cols);
    w.rows = reinterpret_cast<uint16_t *>(base + o_rows);
    w.ncols = reinterpret_cast<int32_t *>(base + o_ncols);
    w.nrows = reinterpret_cast<int32_t *>(base + o_nrows);
    w.prefix = reinterpret_cast<uint32_t *>(base + o_prefix);
    w.rowbase = reinterpret_cast<uint32_t *>(base + o_rowbase);
    w.colbase = reinterpret_cast<uint32_t *>(base + o_colbase);
    w.Er = reinterpret_cast<uint16_t *>(base + o_Er);
    w.Ec = reinterpret_cast<uint16_t *>(base + o_Ec);
    w.E = reinterpret_cast<uint16_t *>(base + o_E);
    const bool e_32bit = sizeof(uint16_t) * (size_t)w.He_p * w.We_p < ((size_t)1 << 31); // focus_pick_sep: a candidate's plane of E behind one buffer descriptor
    w.K = reinterpret_cast<uint16_t *>(base + o_K);
    w.deltas = reinterpret_cast<int64_t *>(base + o_deltas);
    w.pad = reinterpret_cast<uint32_t *>(base + o_pad);
    w.carry = reinterpret_cast<uint32_t *>(base + o_carry);
    lfi::FocusPatch *patches = reinterpret_cast<lfi::FocusPatch *>(base + o_patches);
    // Two streams: the plan and the flagged-pair passes are small, latency-bound kernels; they run beside the padded copy
    // and the range pass (bandwidth / VALU bound) instead of in front of them.
    //   main:  plan_shifts ─┬─ pad ─┬─ range ───────────────────────────────────────────┬─ line_keys → pick (→ filter, by the caller)
    //   aux:                └─ flags → lists → prefix ─┴─ {lines_rows, lines_cols, exact} ─┘
    if(int rc = ensure_aux_stream(ctx))
        return rc;
    hipStream_t st = ctx->stream;
    hipStream_t aux = ctx->aux_stream;
    // host launch order = the critical path first: the main stream's kernels are enqueued before the side stream's
    // (the patch plans of focus_range_t by the same launch: one kernel less in front of the range pass)
    hipLaunchKernelGGL(lfi::focus_plan_shifts, dim3(1), dim3(1024), 0, st, a, w, patches, range_cpw);
    LFI_HIP(ctx, hipEventRecord(ctx->ev_fork, st));
    bool padded_any = true; // something was enqueued between ev_fork and the range pass
    if(later_pass)
        padded_any = false;
    else if(pad_kept && ctx->pad_version != 0) // (a reallocated workspace cleared pad_version)
    {
        padded_any = false;
        for(int k = 0; k < n_ids; k++)
            if(ctx->pad_ids[k] != job.ids[k] || image_changed_since(ctx, job.ids[k], ctx->pad_version))
            {
                hipLaunchKernelGGL(lfi::focus_pad, dim3((w.Wp + 255) / 256, (w.Hp + lfi::FOCUS_PAD_ROWS - 1) / lfi::FOCUS_PAD_ROWS, 1), dim3(64), 0, st, a, w, k);
                padded_any = true;
                job.padded++;
            }
        ctx->pad_version = ctx->grid_version;
        ctx->pad_ids.assign(job.ids, job.ids + n_ids);
    }
    else
    {
        hipLaunchKernelGGL(lfi::focus_pad, dim3((w.Wp + 255) / 256, (w.Hp + lfi::FOCUS_PAD_ROWS - 1) / lfi::FOCUS_PAD_ROWS, n_ids), dim3(64), 0, st, a, w, 0);
        job.padded = n_ids;
        ctx->pad_version = ctx->grid_tracked ? ctx->grid_version : 0;
        ctx->pad_shift[0] = Sx;
        ctx->pad_shift[1] = Sy;
        ctx->pad_radius[0] = rx;
        ctx->pad_radius[1] = ry;
        ctx->pad_ids.assign(job.ids, job.ids + n_ids);
    }
    // (planes kept and nothing re-padded: ev_fork says all the side stream needs to know — one event packet less in front of the range pass)
    if(padded_any)
        LFI_HIP(ctx, hipEventRecord(ctx->ev_pad, st));
    {
        lfi_focus_route &r = ctx->route;
        const int p = a.focus_i0 / lfi::FOCUS_STEPS;
        if(!later_pass)
        {
            r.jobs++;
            r.planes_padded += job.padded;
            r.planes_kept += n_ids - job.padded;
            r.pad_shift[0] = Sx, r.pad_shift[1] = Sy;
            r.We_p = w.We_p, r.He_p = w.He_p, r.Wp = w.Wp, r.Hp = w.Hp, r.R_cap = w.R_cap, r.C_cap = w.C_cap;
        }
        r.estimate = direct_range ? "factored_direct" : "factored";
        r.passes = p + 1;
        r.range_cpw[p] = range_cpw;
        ctx->route_counts_at = o_prefix + sizeof(uint32_t) * lfi::FOCUS_ROUTE_COUNTS;
    }
    const uint32_t tiles_x = uint32_t(w.We_p / 256), tiles_y = uint32_t(w.He_p / 4);
    if(range_cpw)
    {
        const uint32_t groups = uint32_t(lfi::FOCUS_STEPS / range_cpw);
        const uint32_t ttx = uint32_t(w.We_p / lfi::FRT_TW), tty = uint32_t((w.He_p + lfi::FRT_TH - 1) / lfi::FRT_TH);
        const int striped = ttx >= 8; // (row-major order of the items instead: range pass 1.64 → 1.71 ms at 4K)
        const uint32_t nblocks = striped ? 8u * lfi::stripe_blocks_per_xcd(ttx, tty, groups) : ttx * tty * groups;
        // persistent: one workgroup per CU (it owns the whole LDS), a multiple of 8 so that a workgroup's work items stay on its XCD
        const uint32_t grid = std::min(nblocks, uint32_t(std::max(ctx->cu_count / 8 * 8, 8)));
        ctx->route.range_kernel = range_cpw == 8 ? "focus_range_t<8>" : "focus_range_t<4>";
        ctx->route.range_striped = striped;
        if(range_cpw == 8)
            hipLaunchKernelGGL(lfi::focus_range_t<8>, dim3(grid), dim3(64 * (lfi::FRT_NW + lfi::FRT_LW)), 0, st, a, w, patches, uint32_t(pad_bytes), nblocks, striped);
        else
            hipLaunchKernelGGL(lfi::focus_range_t<4>, dim3(grid), dim3(64 * (lfi::FRT_NW + lfi::FRT_LW)), 0, st, a, w, patches, uint32_t(pad_bytes), nblocks, striped);
    }
    else
    {
        constexpr int CPW = 4, GROUPS = lfi::FOCUS_STEPS / CPW;
        const int striped = tiles_x >= 8;
        const uint32_t nblocks = striped ? 8u * lfi::stripe_blocks_per_xcd(tiles_x, tiles_y, GROUPS) : tiles_x * tiles_y * GROUPS;
        ctx->route.range_kernel = "focus_range<4>";
        ctx->route.range_striped = striped;
        hipLaunchKernelGGL(lfi::focus_range<CPW>, dim3(nblocks), dim3(256), 0, st, a, w, nblocks, striped);
    }
    LFI_HIP(ctx, hipStreamWaitEvent(aux, ctx->ev_fork, 0));
    LFI_HIP(ctx, hipMemsetAsync(w.badx, 0, o_cols - o_badx, aux)); // badx, bady, tapx, tapy are adjacent
    hipLaunchKernelGGL(lfi::focus_plan_flags, dim3((std::max(W, H) + 255) / 256, lfi::FOCUS_STEPS, 2), dim3(256), 0, aux, a, w);
    hipLaunchKernelGGL(lfi::focus_plan_lists, dim3(lfi::FOCUS_STEPS, 2), dim3(64), 0, aux, a, w);
    hipLaunchKernelGGL(lfi::focus_plan_prefix, dim3(1), dim3(1), 0, aux, a, w);
    if(padded_any)
        LFI_HIP(ctx, hipStreamWaitEvent(aux, ctx->ev_pad, 0));
    {
        const uint32_t per_pass = uint32_t(ctx->cu_count) * 4u / 8u * 8u;
#ifdef LFI_MEASUREMENT_BUILD // one launch per pass, so that a kernel trace shows what each of the three costs
        for(uint32_t pass = 0; pass < 3; pass++)
            hipLaunchKernelGGL(lfi::focus_flagged, dim3(per_pass), dim3(256), 0, aux, a, w, per_pass, pass);
#else
        hipLaunchKernelGGL(lfi::focus_flagged, dim3(3 * per_pass), dim3(256), 0, aux, a, w, per_pass, 0u);
#endif
    }
    // The keys of single-axis pairs take their unflagged taps from E: focus_line_keys runs behind BOTH streams' work.  On the main stream —
    // the flagged passes end before the range pass does, so the join is an event already signalled, and the keys, the pick and whatever the
    // caller enqueues next follow the range pass in one queue (on the side stream they cost two more hops between queues, ≈ 10 µs each).
    LFI_HIP(ctx, hipEventRecord(ctx->ev_join, aux));
    LFI_HIP(ctx, hipStreamWaitEvent(st, ctx->ev_join, 0));
    hipLaunchKernelGGL(lfi::focus_line_keys, dim3(ctx->cu_count * 8), dim3(256), 0, st, a, w);
    *w_out = w;
    *e_32bit_out = e_32bit;
    *done = true;
    return LFI_OK;
}

// pixels per lane of the kernels behind the keys (focus_pick, focus_tile_costs): two need dword-aligned sample pairs — an even radius_x (the reference's is)
int focus_keys_ppl(const lfi_ctx *ctx) { return (ctx->radius[0] % 2 == 0 && ctx->width >= 2) ? 2 : 1; }

// the factored estimate's last pass: per pixel the first strict minimum of the keys → map 0 (the caller filters it into map 1).
// A sweep of more than 32 candidates: the same kernels' carrying forms, once per pass (focus_pick_store)
int launch_focus_pick(lfi_ctx *ctx, const KernelArgs &a, const lfi::FocusWork &w, bool e_32bit, bool direct_range)
{
    const bool carry = a.focus_steps > lfi::FOCUS_STEPS;
    const int W = ctx->width, H = ctx->height, rx = ctx->radius[0], ry = ctx->radius[1];
    hipStream_t st = ctx->stream;
    const int ppl = focus_keys_ppl(ctx);
    const uint32_t blocks_x = uint32_t((W + 64 * ppl - 1) / (64 * ppl)), blocks_y = uint32_t((H + 3) / 4);
    const int striped = blocks_x >= 8;
    const uint32_t nblocks = striped ? 8u * lfi::stripe_blocks_per_xcd(blocks_x, blocks_y, 1u) : blocks_x * blocks_y;
    // the tap block taken apart (focus_pick_sep): even radius_x of at most 64; variant "factored_direct" keeps focus_pick<2>, the other implementation
    lfi_focus_route &r = ctx->route;
    r.consumer_striped = striped;
    if(ppl == 2 && rx <= 64 && e_32bit && !direct_range)
    {
        r.consumer = carry ? "focus_pick_sep_carry" : "focus_pick_sep";
        r.consumer_striped = 0;
        // (row-major order of the workgroups, not stripes per XCD: this kernel's re-use of E's rows happens inside a workgroup)
        const uint32_t nb = blocks_x * lfi::focus_pick_sep_block_rows(H, ry);
        if(carry)
            hipLaunchKernelGGL(lfi::focus_pick_sep_carry, dim3(nb), dim3(64 * lfi::FPS_WAVES), 0, st, a, w);
        else
            hipLaunchKernelGGL(lfi::focus_pick_sep, dim3(nb), dim3(64 * lfi::FPS_WAVES), 0, st, a, w);
    }
    else if(ppl == 2 && carry)
    {
        r.consumer = "focus_pick_carry<2>";
        hipLaunchKernelGGL(lfi::focus_pick_carry<2>, dim3(nblocks), dim3(256), 0, st, a, w, striped);
    }
    else if(ppl == 2)
    {
        r.consumer = "focus_pick<2>";
        hipLaunchKernelGGL(lfi::focus_pick<2>, dim3(nblocks), dim3(256), 0, st, a, w, striped);
    }
    else if(carry)
    {
        r.consumer = "focus_pick_carry<1>";
        hipLaunchKernelGGL(lfi::focus_pick_carry<1>, dim3(nblocks), dim3(256), 0, st, a, w, striped);
    }
    else
    {
        r.consumer = "focus_pick<1>";
        hipLaunchKernelGGL(lfi::focus_pick<1>, dim3(nblocks), dim3(256), 0, st, a, w, striped);
    }
    LFI_HIP(ctx, hipGetLastError());
    return LFI_OK;
}

// The passes of a factored sweep: plan → pad → E → exact keys (launch_focus_factored_keys), then consume(pass, w, e_32bit) — whatever reads E
// and K — once per 32 candidates of a.focus_steps, the padding by the first pass only.  *done = false when the first pass declined (the
// later ones take its geometry): then nothing has been enqueued and consume has not been called.
template <class Consume>
int focus_factored_passes(lfi_ctx *ctx, const KernelArgs &a, FocusJob &job, bool *done, bool direct_range, Consume &&consume)
{
    KernelArgs pass = a;
    for(pass.focus_i0 = 0; pass.focus_i0 < a.focus_steps; pass.focus_i0 += lfi::FOCUS_STEPS)
    {
        lfi::FocusWork w{};
        bool e_32bit = false;
        if(int rc = launch_focus_factored_keys(ctx, pass, job, done, direct_range, &w, &e_32bit))
            return rc;
        if(!*done)
            return LFI_OK;
        if(int rc = consume(pass, w, e_32bit))
            return rc;
    }
    return LFI_OK;
}

// the whole factored estimate: every pass's keys, then its pick
int launch_focus_factored(lfi_ctx *ctx, const KernelArgs &a, FocusJob &job, bool *done, bool direct_range)
{
    return focus_factored_passes(ctx, a, job, done, direct_range, [&](const KernelArgs &pass, const lfi::FocusWork &w, bool e_32bit) {
        return launch_focus_pick(ctx, pass, w, e_32bit, direct_range);
    });
}

// A focus curve in memory: cost[steps] (u64), then its lfi_focus_curve_result — what focus_curve_sum / focus_curve_pick write and the host
// copies in one piece.  ctx->curve_ws holds one (lfi_focus_curve) or one per tile, row-major (lfi_focus_tiles), then the partial sums.
constexpr size_t focus_curve_head(const int steps) { return sizeof(uint64_t) * size_t(steps) + sizeof(lfi_focus_curve_result); }
constexpr size_t FOCUS_CURVE_HEAD = (focus_curve_head(lfi::FOCUS_CURVE_MAX_STEPS) + 255) / 256 * 256;

constexpr int FOCUS_CURVE_PPL = 2; // pixels per lane: focus_estimate_packed<2, 4>'s shape (row-window path, variant "packed_p2"), five waves per SIMD
inline uint32_t focus_curve_blocks_x(const int width) { return uint32_t((width + 64 * FOCUS_CURVE_PPL - 1) / (64 * FOCUS_CURVE_PPL)); }

// The focus curve of the rectangle [x0, x1) × [y0, y1) over `steps` candidates: partial sums per workgroup and candidate, their sum per
// candidate, the first strict minimum — three launches on the compute stream.  head: where the curve and its result go (focus_curve_head(steps)
// bytes); partial: room for steps × blocks_x × min(rows, max_rows) u64.  max_rows caps the workgroups: a wave walks one row of the rectangle
// while its rows are at most that many, else several.  Nothing of the estimate's state (focus_ws, the padded planes, the maps) is touched.
void launch_focus_curve_rect(lfi_ctx *ctx, const KernelArgs &a, int x0, int y0, int x1, int y1, int steps, uint8_t *head, uint8_t *partial, uint32_t max_rows)
{
    const uint32_t blocks_x = focus_curve_blocks_x(x1 - x0), blocks_y = std::min(uint32_t(y1 - y0), max_rows);
    lfi::FocusCurveArgs q{};
    q.x0 = x0, q.y0 = y0, q.x1 = x1, q.y1 = y1;
    q.steps = steps;
    q.n_wg = blocks_x * blocks_y;
    // A small region (click-to-focus) has too few rows × 128-pixel runs to fill the GPU, and a wave that walks all candidates lives ≈ 1 ms:
    // the candidates are split over blockIdx.z until there are about four waves per SIMD.  Whole frames keep one wave per row and run.
    const uint32_t want_z = std::min(uint32_t(steps), std::max(1u, uint32_t(ctx->cu_count) * 16u / q.n_wg));
    q.steps_per_wg = (steps + int(want_z) - 1) / int(want_z);
    const uint32_t blocks_z = uint32_t((steps + q.steps_per_wg - 1) / q.steps_per_wg);
    q.pixels = uint64_t(x1 - x0) * uint64_t(y1 - y0);
    q.cost = reinterpret_cast<uint64_t *>(head);
    q.partial = reinterpret_cast<uint64_t *>(partial);
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL((lfi::focus_curve_partial<FOCUS_CURVE_PPL, 4>), dim3(blocks_x, blocks_y, blocks_z), dim3(64), 0, st, a, q);
    hipLaunchKernelGGL(lfi::focus_curve_sum, dim3(steps), dim3(256), 0, st, q);
    hipLaunchKernelGGL(lfi::focus_curve_pick, dim3(1), dim3(256), 0, st, a, q);
}

// lfi_focus_curve (the caller has checked the arguments).  *d_head = the device address of the curve.
int launch_focus_curve(lfi_ctx *ctx, const KernelArgs &a, int x0, int y0, int x1, int y1, int steps, const uint8_t **d_head)
{
    const uint32_t blocks_x = focus_curve_blocks_x(x1 - x0);
    // One row per wave while the partials stay small (fine-grained dispatch fills the tail: a wave lives ≈ 1 ms per row at 32 images); beyond
    // 2 Mi partials (16 MB) — whole 4K frames with more than 32 candidates — a wave walks several rows, never fewer than 8192 waves.
    const uint32_t max_wg = std::min(65536u, std::max(8192u, (2u << 20) / uint32_t(steps)));
    const uint32_t max_rows = std::max(1u, max_wg / blocks_x);
    LFI_HIP(ctx, ctx->curve_ws.reserve(FOCUS_CURVE_HEAD + sizeof(uint64_t) * size_t(steps) * blocks_x * std::min(uint32_t(y1 - y0), max_rows)));
    launch_focus_curve_rect(ctx, a, x0, y0, x1, y1, steps, ctx->curve_ws.get(), ctx->curve_ws.get() + FOCUS_CURVE_HEAD, max_rows);
    LFI_HIP(ctx, hipGetLastError());
    *d_head = ctx->curve_ws.get();
    return LFI_OK;
}

// The focus curves of the tiles_x × tiles_y tiles over `steps` candidates, a multiple of 32 up to 256 (lfi_focus_tiles: 32; lfi_focus_tiles_steps;
// the caller has checked the arguments).  ctx->curve_ws holds, per tile, the curve and its result back to back (focus_curve_head(steps) bytes
// each, row-major over the tiles: what the host copies), then the partial sums.
//   factored: focus_factored_passes with focus_steps = steps and, in the pick's place, focus_tile_costs, then focus_curve_sum for the pass's
//             slice cost[tile][32g … 32g + 31]; behind the last pass focus_curve_pick over all tiles and all steps.  2·passes + 1 launches
//             behind the keys whatever the grid; at 32 steps the three launches lfi_focus_tiles has always made.  The partials stay
//             [tiles][32][n_wg]: every pass overwrites them, behind the sum that read them (one stream).  Pass g + 1 rewrites E and K, which
//             pass g's focus_tile_costs reads: launch_focus_factored_keys records ev_fork on the compute stream behind everything enqueued
//             there so far — the tile costs and the sum — and the side stream's writers wait for it; the range pass follows the tile costs
//             in the compute stream's own order.
//   else (another estimate variant, or the factored estimate's first pass declined — then nothing has been enqueued):
//             launch_focus_curve_rect tile by tile with all the steps — the same numbers; the partials' room is shared (one stream).
int launch_focus_tiles(lfi_ctx *ctx, const KernelArgs &a, int tiles_x, int tiles_y, int steps, const uint8_t **d_head)
{
    const int W = ctx->width, H = ctx->height;
    const size_t tiles = size_t(tiles_x) * size_t(tiles_y);
    const size_t tile_head = focus_curve_head(steps);
    const size_t head_bytes = (tile_head * tiles + 255) / 256 * 256;
    const int tile_w = (W + tiles_x - 1) / tiles_x, tile_h = (H + tiles_y - 1) / tiles_y; // the widest, the tallest
    hipStream_t st = ctx->stream;
    if((ctx->focus_variant == 0 || ctx->focus_variant == 4) && W <= 65535 && H <= 65535)
    {
        FocusJob job;
        job.offsets = ctx->h_focus_offsets.data();
        job.ids = ctx->h_focus_ids.data();
        job.n_ids = ctx->n_focus_ids;
        const int ppl = focus_keys_ppl(ctx);
        lfi::FocusTileArgs t{};
        t.tiles_x = tiles_x, t.tiles_y = tiles_y;
        t.chunks = (tile_w + (ppl - 1) + 64 * ppl - 1) / (64 * ppl); // (+1: a tile's first column rounded down to even)
        // one row per wave (the pick's shape) while that keeps the partials small: beyond 64 Ki workgroups a wave walks more rows
        const size_t wg_1 = tiles * t.chunks * ((tile_h + 3) / 4);
        t.rows_per_wave = int(std::min<size_t>(lfi::FOCUS_TILE_MAX_ROWS_PER_WAVE, std::max<size_t>(1, (wg_1 + 65535) / 65536)));
        t.rows_per_wave = std::min(t.rows_per_wave, (tile_h + 3) / 4);
        t.bands = (tile_h + 4 * t.rows_per_wave - 1) / (4 * t.rows_per_wave);
        t.n_wg = uint32_t(t.chunks) * uint32_t(t.bands);
        const size_t n_blocks = tiles * t.n_wg;
        lfi::FocusCurveArgs q{};
        q.steps = steps;
        q.n_wg = t.n_wg;
        q.tiled = 1;
        KernelArgs sweep = a;
        sweep.focus_steps = steps;
        sweep.focus_div = float(steps - 1);
        bool done = false;
        const int rc = focus_factored_passes(ctx, sweep, job, &done, ctx->focus_variant == 4, [&](const KernelArgs &pass, const lfi::FocusWork &w, bool) {
            if(pass.focus_i0 == 0)
            {
                if(n_blocks > 0x7fffffffu)
                    return fail(ctx, LFI_EINVAL, "lfi_focus_tiles: too many tiles for an image of this size");
                LFI_HIP(ctx, ctx->curve_ws.reserve(head_bytes + sizeof(uint64_t) * lfi::FOCUS_STEPS * n_blocks));
                q.cost = reinterpret_cast<uint64_t *>(ctx->curve_ws.get());
                q.partial = t.partial = reinterpret_cast<uint64_t *>(ctx->curve_ws.get() + head_bytes);
            }
            ctx->route.consumer = ppl == 2 ? "focus_tile_costs<2>" : "focus_tile_costs<1>";
            if(ppl == 2)
                hipLaunchKernelGGL(lfi::focus_tile_costs<2>, dim3(uint32_t(n_blocks)), dim3(256), 0, st, pass, w, t);
            else
                hipLaunchKernelGGL(lfi::focus_tile_costs<1>, dim3(uint32_t(n_blocks)), dim3(256), 0, st, pass, w, t);
            q.sum_at = pass.focus_i0;
            hipLaunchKernelGGL(lfi::focus_curve_sum, dim3(lfi::FOCUS_STEPS, tiles_x, tiles_y), dim3(256), 0, st, q);
            return int(LFI_OK);
        });
        if(rc)
            return rc;
        if(done)
        {
            ctx->tiles_passes = steps / lfi::FOCUS_STEPS;
            hipLaunchKernelGGL(lfi::focus_curve_pick, dim3(tiles_x, tiles_y), dim3(256), 0, st, a, q);
            LFI_HIP(ctx, hipGetLastError());
            *d_head = ctx->curve_ws.get();
            return LFI_OK;
        }
    }
    ctx->tiles_passes = 0;
    ctx->route.estimate = "focus_curve";
    const uint32_t blocks_x = focus_curve_blocks_x(tile_w);
    const uint32_t max_rows = std::max(1u, 8192u / blocks_x);
    LFI_HIP(ctx, ctx->curve_ws.reserve(head_bytes + sizeof(uint64_t) * size_t(steps) * blocks_x * std::min(uint32_t(tile_h), max_rows)));
    for(int ty = 0; ty < tiles_y; ty++)
        for(int tx = 0; tx < tiles_x; tx++)
            launch_focus_curve_rect(ctx, a, lfi::focus_tile_edge(tx, W, tiles_x), lfi::focus_tile_edge(ty, H, tiles_y), lfi::focus_tile_edge(tx + 1, W, tiles_x),
                                    lfi::focus_tile_edge(ty + 1, H, tiles_y), steps, ctx->curve_ws.get() + tile_head * (size_t(ty) * tiles_x + tx),
                                    ctx->curve_ws.get() + head_bytes, max_rows);
    LFI_HIP(ctx, hipGetLastError());
    *d_head = ctx->curve_ws.get();
    return LFI_OK;
}

} // namespace
