"""GPU (-m gpu): every case of the focus routes' table (tests/focus_routes.py) under both range implementations — maps 0 and 1 `==` the oracle
and lfi_focus_route_info's record `==` the restatement's, field for field, the device's per-pass row_entries / col_entries included (which
holds the plan kernels to the definition).  The maps and the estimate's workspace are poisoned before every first call; a second call with only
the maps poisoned must pad no plane, give the same bytes and count one call more.  The marked cases also run lfi_focus_tiles,
lfi_focus_tiles_steps and lfi_view_focus_maps, each against the reference its own suite uses.  No tolerance anywhere.

tests/test_focus_routes_table.py shows on the CPU that the table reaches every leaf and that no class of flagged pairs could be skipped
unnoticed on it.  A restatement is computed once per case and shared by the variants."""
import dataclasses
import functools

import numpy as np
import pytest

import focus_routes as fr
import focus_steps_ref
import lfinterpolator_amd as L
import poison

pytestmark = pytest.mark.gpu

VARIANTS = ["factored", "factored_direct"]
NAMES = [c["name"] for c in fr.CASES]
WINDOW = (8, 16)    # the band of the row-window case: rows [8, 16) of 24, every input row held


@functools.lru_cache(maxsize=None)
def _case(name):
    """(case, hp, lf, plan, map 0, map 1, exact keys) — cached: shared and never written"""
    from oracle import lfi_oracle_c as oc
    oc.build()
    c = next(c for c in fr.CASES if c["name"] == name)
    hp, lf = fr.build(L, oc, c)
    plan = fr.plan_of(L, oc, c, hp)
    if c["steps"] == 32:
        want0 = oc.focus_estimate(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, threads=8)
    else:
        want0 = focus_steps_ref.map0(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, c["steps"])
    want1 = oc.focus_filter(want0, hp.block_radius)
    exact = fr.key_planes(plan, lf, hp.focus_map_ids)[0] if set(c["more"]) & {"tiles", "tile_steps"} else None
    for a in (lf, want0, want1):
        a.setflags(write=False)
    return c, hp, lf, plan, want0, want1, exact


def _ctx(gpu, c, hp, lf, variant, window=False):
    ctx = gpu.Context(0)
    ctx.set_grid(c["cols"], c["rows"], c["W"], c["H"])
    if window:
        ctx.set_row_window(WINDOW[0], WINDOW[1], 0, c["H"])
    ctx.upload_grid(lf)
    ctx.set_params(hp)
    ctx.set_variant("FOCUS", variant)
    if c["steps"] != 32:
        ctx.set_focus_steps(c["steps"])
    return ctx


def _expected(c, hp, plan, variant, state, consumer="pick", steps=None):
    steps = c["steps"] if steps is None else steps
    want = fr.expected_route(c["W"], c["H"], hp.block_radius, hp.offsets[hp.focus_map_ids], hp.focus_map_ids, hp.focus, hp.range, steps, variant, consumer,
                             state=state, plan=plan)
    if want["declined"]:
        # the factored estimate declined before it reserved anything: lfi_focus_map's other variants answer (32 candidates: the LDS-staged
        # kernel under `factored`, packed_p2 under `factored_direct`; a sweep: packed_p2), the tiles go through lfi_focus_curve's kernels
        answer = "focus_curve" if consumer == "tiles" else "lds" if variant == "factored" and steps == 32 else "packed_p2"
        want = dict(want, estimate=answer)
    return dict(want, jobs=0 if want["declined"] else 1)


def _assert_route(ctx, want, calls, what):
    got = ctx.focus_route()
    wrong = fr.route_matches(got, dict(want, calls=calls))
    assert not wrong, (what, {n: (got[n], dict(want, calls=calls)[n]) for n in wrong})
    return got


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", NAMES)
def test_every_case_takes_the_expected_route_and_gives_the_oracles_maps(gpu, name, variant):
    c, hp, lf, plan, want0, want1, exact = _case(name)
    window = "row_window" in c["more"]
    rows = slice(*WINDOW) if window else slice(None)
    state = fr.PadState()
    with _ctx(gpu, c, hp, lf, variant, window) as ctx:
        assert ctx.focus_route()["calls"] == 0 and ctx.focus_route()["estimate"] == ""
        byte = poison.focus_map(ctx)
        got0, got1 = ctx.download_map(0), ctx.download_map(1)
        assert (got0[rows] == want0[rows]).all(), (name, variant, "map 0", int((got0[rows] != want0[rows]).any(-1).sum()))
        assert (got1[rows] == want1[rows]).all(), (name, variant, "map 1")
        if window:
            want = dict(estimate="row_window", declined="", passes=0, jobs=0, planes_padded=0, range_kernel="", consumer="")
        else:
            want = _expected(c, hp, plan, variant, state)
        first = _assert_route(ctx, want, 1, (name, variant))
        # again, only the maps poisoned: the planes are kept, the bytes and the route are the same
        ctx.poison(L.LFI_POISON_MAPS, poison.POISON[0] ^ poison.POISON[1] ^ byte)
        ctx.focus_map()
        ctx.sync()
        again = ctx.focus_route()
        assert again["planes_padded"] == 0 and again["calls"] == 2
        assert {k: v for k, v in again.items() if k not in ("calls", "planes_padded", "planes_kept")} == \
               {k: v for k, v in first.items() if k not in ("calls", "planes_padded", "planes_kept")}
        assert again["planes_kept"] == first["planes_padded"] + first["planes_kept"]
        assert (ctx.download_map(0)[rows] == got0[rows]).all() and (ctx.download_map(1)[rows] == got1[rows]).all()


def _tile_sums(costs, W, H, nx, ny):
    """[ny][nx][steps] u64: the curve of every tile of lfi_host_focus_tile_rect's grid (tests/test_gpu_focus_tile_steps.py)"""
    xe, ye = [t * W // nx for t in range(nx)], [t * H // ny for t in range(ny)]
    assert L.focus_tile_rect(W, H, nx, ny, nx - 1, ny - 1) == (xe[-1], ye[-1], W, H)
    return np.ascontiguousarray(np.add.reduceat(np.add.reduceat(costs, ye, axis=1), xe, axis=2).transpose(1, 2, 0)).astype(np.uint64)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", [c["name"] for c in fr.CASES if set(c["more"]) & {"tiles", "tile_steps"}])
def test_the_tiles_of_the_marked_cases(gpu, name, variant):
    """lfi_focus_tiles (32 candidates) and lfi_focus_tiles_steps (the case's sweep): every tile's curve is the sum of the restatement's
    per-pixel costs, the consumer is focus_tile_costs, the plan's counts are the map's"""
    c, hp, lf, plan, want0, want1, exact = _case(name)
    W, H, steps = c["W"], c["H"], c["steps"]
    costs = fr.pixel_costs(exact)
    state = fr.PadState()
    with _ctx(gpu, c, hp, lf, variant) as ctx:
        for calls, (nx, ny) in enumerate([(1, 1), (min(W, 3), min(H, 2))], 1):
            ctx.poison(poison.FOCUS, poison.POISON[calls & 1])
            state.valid = False     # (a poisoned workspace holds no planes: lfi_debug_poison says so to the bookkeeping)
            cost, best, f = ctx.focus_tiles(nx, ny, steps=steps)
            want = _tile_sums(costs, W, H, nx, ny)
            assert (cost == want).all(), (name, variant, (nx, ny), np.argwhere(cost != want)[:4])
            assert (best == want.argmin(axis=2)).all()
            assert (f.view(np.uint32) == L.focus_candidates(hp.focus, hp.range, steps)[best].view(np.uint32)).all()
            route = _expected(c, hp, plan, variant, state, "tiles")
            _assert_route(ctx, route, calls, (name, variant, (nx, ny)))
            assert ctx.focus_tiles_passes() == (0 if route["declined"] else steps // 32)


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_per_view_maps_of_the_marked_case(gpu, variant):
    """lfi_view_focus_maps on the case with both overflows: every view's maps are the oracle's; the record is the last view's job, with the
    batch's jobs and planes — slot-stable re-padding pads fewer planes than views x images — and a second batch pads none"""
    from oracle import lfi_oracle_c as oc
    (name,) = [c["name"] for c in fr.CASES if "view_maps" in c["more"]]
    c, hp, lf, _, _, _, _ = _case(name)
    V = 3
    hp = dataclasses.replace(L.build_params(c["cols"], c["rows"], c["W"], c["H"], fr.TRAJ, c["focus"], c["range"], 3.0, 1.783, V), block_radius=hp.block_radius)
    O, _ = L.build_view_centred_offsets(c["cols"], c["rows"], c["W"], c["H"], fr.TRAJ, 1.783, np.full(V, c["focus"], np.float32))
    ids = L.build_view_focus_ids(c["cols"], c["rows"], fr.TRAJ, V)
    state = fr.PadState()
    with _ctx(gpu, c, hp, lf, variant) as ctx:
        ctx.set_view_float_offsets(O)
        for calls in (1, 2):
            ctx.poison(L.LFI_POISON_VIEW_MAPS | (L.LFI_POISON_FOCUS_WORKSPACE if calls == 1 else 0), poison.POISON[calls & 1])
            ctx.view_focus_maps(ids)
            ctx.sync()
            for v in range(V):
                m0 = oc.focus_estimate(lf, O[v], ids[v], hp.focus, hp.range, hp.block_radius, threads=8)
                assert (ctx.download_view_map(v, 0) == m0).all(), (variant, v, calls)
                assert (ctx.download_view_map(v, 1) == oc.focus_filter(m0, hp.block_radius)).all(), (variant, v, calls)
            want, rows = fr.view_maps_route(c["W"], c["H"], hp.block_radius, O, ids, hp.focus, hp.range, variant, state)
            last = fr.Plan(oc, c["W"], c["H"], hp.block_radius, O[V - 1][ids[V - 1]], hp.focus, hp.range)
            want = dict(want, row_entries=last.row_entries, col_entries=last.col_entries)
            got = _assert_route(ctx, want, calls, (variant, calls))
            if calls == 1:
                assert ids.shape[1] <= got["planes_padded"] < V * ids.shape[1] and last.row_entries[0] > last.R_cap and last.col_entries[0] > last.C_cap
            else:
                assert got["planes_padded"] == 0 and got["planes_kept"] == V * ids.shape[1]


def test_the_padded_planes_between_calls(gpu):
    """PAD_SEQUENCE on one context: planes rebuilt, kept, kept under a smaller interval, grown by a quarter under a larger one, kept but for
    an image uploaded again, rebuilt for another radius — the record says which, the maps are the oracle's every time"""
    from oracle import lfi_oracle_c as oc
    s = fr.PAD_SHAPE
    lf = oc.synthetic_lf(s["cols"] * s["rows"], s["W"], s["H"], 99)
    lf = (lf // 16 * 16).astype(np.uint8)
    lf[..., 3] = 255
    seen = set()
    with gpu.Context(0) as ctx:
        ctx.set_grid(s["cols"], s["rows"], s["W"], s["H"])
        ctx.upload_grid(lf)
        for calls, (what, hp, again, want, leaves) in enumerate(fr.pad_sequence_routes(L), 1):
            if again is not None:
                ctx.upload_image(int(hp.focus_map_ids[again]), lf[int(hp.focus_map_ids[again])])
            ctx.set_params(hp)
            ctx.poison(L.LFI_POISON_MAPS, poison.POISON[calls & 1])
            ctx.focus_map()
            ctx.sync()
            plan = fr.Plan(oc, s["W"], s["H"], hp.block_radius, hp.offsets[hp.focus_map_ids], hp.focus, hp.range)
            _assert_route(ctx, dict(want, jobs=1, row_entries=plan.row_entries, col_entries=plan.col_entries), calls, what)
            want0 = oc.focus_estimate(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, threads=8)
            assert (ctx.download_map(0) == want0).all() and (ctx.download_map(1) == oc.focus_filter(want0, hp.block_radius)).all(), what
            seen |= leaves
    assert seen == {"planes rebuilt", "planes kept", "planes grown by a quarter", "planes kept but for the uploaded image"}


def test_a_null_record_is_refused(gpu):
    with gpu.Context(0) as ctx:
        assert ctx._lib.lfi_focus_route_info(ctx._h, None) == -1 and ctx._lib.lfi_focus_route_info(None, None) == -1
