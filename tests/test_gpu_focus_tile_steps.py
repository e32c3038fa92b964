"""GPU (-m gpu): fine focus tiles — lfi_focus_tiles_steps, every tile's focus curve over a multiple of 32 candidates up to 256 from one
factored estimate per 32, and the CLI's --tile-steps / whole-frame --autofocus.

Every tile's cost[] is compared for u64 EQUALITY with the numpy restatement (tests/focus_curve_ref.py, anchored to the oracle by
tests/test_host_focus_curve.py) over the rectangle of lfinterpolator_amd.focus_tile_rect; best_index is the first minimum of the returned
costs, best_focus that candidate bit for bit, pixels the rectangle's area.  No tile and no candidate is skipped.  In the factored variants
lfi_focus_tiles_passes must say that the factored passes ran: no test passes by the tile-by-tile fallback.  The estimate's workspace and the
curves' memory are poisoned before every call a check reads, with alternating bytes."""
import dataclasses
import functools
import re

import numpy as np
import pytest

import focus_curve_ref as ref
import focus_routes
import focus_steps_ref as sref
import lfinterpolator_amd as L
import poison
from test_gpu_focus_tiles import CASES, _has_negative_shifts
from test_host_focus_steps import FUZZ, fuzz_case
from test_host_focus_tile_steps import BOUNDARY, BOUNDARY_GRID, BOUNDARY_KS, BOUNDARY_TILES, boundary_scene
from test_host_focus_tiles import two_depth_scene
from view_rows import run_cli

pytestmark = pytest.mark.gpu

CASE_NAMES = ["g3x3", "g8x8_ids5", "g15x15", "g8x8_r3x1", "g8x8_r1x3"]
STEPS = [64, 96, 256]
GRIDS = [(1, 1), (3, 2), (7, 5), "pixels"]
VARIANTS = ["auto", "factored_direct", "packed_p2"]   # focus_range_t where it applies / focus_range / the fallback through focus_curve_partial


@functools.lru_cache(maxsize=None)
def _case(case):
    """(hp, lf) of a test_gpu_focus_tiles case; cached: shared and never written"""
    from oracle import lfi_oracle_c as oc
    cols, rows, W, H, traj, focus, rng, seed, n_ids, radius = CASES[case]
    hp = L.build_params(cols, rows, W, H, traj, focus, rng, 3.0, 1.783, 3)
    if n_ids is not None:
        hp = dataclasses.replace(hp, focus_map_ids=np.ascontiguousarray(hp.focus_map_ids[:n_ids]))
    if radius is not None:
        hp = dataclasses.replace(hp, block_radius=np.array(radius, np.int32))
    lf = oc.synthetic_lf(cols * rows, W, H, seed)
    lf.setflags(write=False)
    return hp, lf


@functools.lru_cache(maxsize=None)
def _costs(case, steps):
    hp, lf = _case(case)
    costs = ref.pixel_costs(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, steps)
    costs.setflags(write=False)
    return costs


def _ctx(gpu, case, variant="auto"):
    cols, rows, W, H = CASES[case][:4]
    hp, lf = _case(case)
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, W, H)
    ctx.upload_grid(lf)
    ctx.set_params(hp)
    ctx.set_variant("FOCUS", variant)
    return ctx


def _grid(ctx, grid):
    return (min(ctx.width, 256), min(ctx.height, 256)) if grid == "pixels" else grid


def _tile_sums(costs, W, H, nx, ny):
    """[ny][nx][steps] u64: the restatement's curve of every tile, ref.curve over focus_tile_rect's rectangles in one go (the tiles are the
    runs between consecutive edges t * size // n; asserted against focus_tile_rect)"""
    xe = [t * W // nx for t in range(nx)]
    ye = [t * H // ny for t in range(ny)]
    assert L.focus_tile_rect(W, H, nx, ny, nx - 1, ny - 1) == (xe[-1], ye[-1], W, H) and L.focus_tile_rect(W, H, nx, ny, 0, 0)[:2] == (0, 0)
    s = np.add.reduceat(np.add.reduceat(costs, ye, axis=1), xe, axis=2)
    return np.ascontiguousarray(s.transpose(1, 2, 0)).astype(np.uint64)


def _check(ctx, hp, costs, grid, steps, poisoned=True, factored=None):
    nx, ny = _grid(ctx, grid)
    if poisoned:
        ctx.poison(poison.FOCUS, poison._byte(None))
    cost, best, f = ctx.focus_tiles(nx, ny, steps=steps)
    if factored is not None:
        assert ctx.focus_tiles_passes() == (steps // 32 if factored else 0), (grid, steps, ctx.focus_tiles_passes())
    assert cost.dtype == np.uint64 and cost.shape == (ny, nx, steps) and best.shape == (ny, nx) and f.shape == (ny, nx)
    W, H = ctx.width, ctx.height
    want = _tile_sums(costs, W, H, nx, ny)
    # a sample of the tiles through ref.curve and focus_tile_rect themselves (the corners and the middle)
    for tx, ty in {(0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1), (nx // 2, ny // 2)}:
        assert (want[ty, tx] == ref.curve(costs, *L.focus_tile_rect(W, H, nx, ny, tx, ty))).all()
    bad = np.argwhere(cost != want)
    assert len(bad) == 0, (grid, steps, len(bad), bad[:4], [(int(cost[tuple(b)]), int(want[tuple(b)])) for b in bad[:4]])
    first = want.argmin(axis=2)                    # np.argmin: the first of equal minima
    assert (best == first).all(), (grid, steps, np.argwhere(best != first)[:4])
    cand = L.focus_candidates(hp.focus, hp.range, steps)
    assert (f.view(np.uint32) == cand[best].view(np.uint32)).all(), (grid, steps)
    xe = np.array([t * W // nx for t in range(nx + 1)])
    ye = np.array([t * H // ny for t in range(ny + 1)])
    assert (ctx.focus_tiles_pixels == np.outer(np.diff(ye), np.diff(xe)).astype(np.uint64)).all(), (grid, steps)
    return cost, best, f


def _same(a, b):
    return all((x.view(np.uint32) == y.view(np.uint32)).all() if x.dtype == np.float32 else (x == y).all() for x, y in zip(a, b))


# ---- 1. every tile against the restatement --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("case", CASE_NAMES)
def test_every_tiles_curve_equals_the_restatement(gpu, case, steps, variant):
    hp, lf = _case(case)
    assert _has_negative_shifts(hp)
    costs = _costs(case, steps)
    with _ctx(gpu, case, variant) as ctx:
        for grid in GRIDS:
            _check(ctx, hp, costs, grid, steps, factored=variant != "packed_p2")
        focus_routes.assert_variant(ctx, variant, hp, steps, "tiles")   # the curves are the named estimate's


# ---- 2. the pass boundary -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", BOUNDARY_KS)
def test_planted_minimum_beside_a_pass_boundary(gpu, k):
    """tests/test_host_focus_tile_steps.py shows on the restatement that these tiles' strict minimum is candidate k of 96"""
    P = BOUNDARY
    hp, lf = boundary_scene(gpu, k)
    costs = ref.pixel_costs(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, P["steps"])
    for variant in VARIANTS:
        with gpu.Context(0) as ctx:
            ctx.set_grid(P["cols"], P["rows"], P["W"], P["H"])
            ctx.upload_grid(lf)
            ctx.set_params(hp)
            ctx.set_variant("FOCUS", variant)
            cost, best, f = _check(ctx, hp, costs, BOUNDARY_GRID, P["steps"], factored=variant != "packed_p2")
            for tx, ty in BOUNDARY_TILES:
                assert best[ty, tx] == k, (variant, tx, ty, best[ty, tx])
                assert (np.delete(cost[ty, tx], k) > cost[ty, tx, k]).all()


@pytest.mark.parametrize("variant", VARIANTS)
def test_all_candidates_tie_and_the_first_wins_across_seven_boundaries(gpu, variant):
    case = "g3x3"
    cols, rows, W, H = CASES[case][:4]
    hp, _ = _case(case)
    lf = np.empty((cols * rows, H, W, 4), np.uint8)
    lf[...] = (200, 100, 50, 255)
    with gpu.Context(0) as ctx:
        ctx.set_grid(cols, rows, W, H)
        ctx.upload_grid(lf)
        ctx.set_params(hp)
        ctx.set_variant("FOCUS", variant)
        for grid in [(1, 1), (7, 5), "pixels"]:      # both poison bytes come round
            nx, ny = _grid(ctx, grid)
            ctx.poison(poison.FOCUS, poison._byte(None))
            cost, best, f = ctx.focus_tiles(nx, ny, steps=256)
            assert ctx.focus_tiles_passes() == (8 if variant != "packed_p2" else 0)
            assert (cost == 0).all() and (best == 0).all()
            assert (f.view(np.uint32) == np.float32(hp.focus).view(np.uint32)).all()


# ---- 3. steps = 32 is lfi_focus_tiles -------------------------------------------------------------------------------------------------

def _tiles_steps_raw(ctx, nx, ny, steps):
    """lfi_focus_tiles_steps itself, also at 32 (Context.focus_tiles takes lfi_focus_tiles there)"""
    cost = np.full((ny, nx, steps), 0xC3C3C3C3C3C3C3C3, dtype=np.uint64)
    res = (L.abi.FocusCurveResult * (nx * ny))()
    assert ctx._lib.lfi_focus_tiles_steps(ctx._h, nx, ny, steps, cost.ctypes.data, res) == 0
    best = np.array([r.best_index for r in res], np.int32).reshape(ny, nx)
    f = np.array([r.best_focus for r in res], np.float32).reshape(ny, nx)
    pixels = np.array([r.pixels for r in res], np.uint64).reshape(ny, nx)
    return cost, best, f, pixels


@pytest.mark.parametrize("variant", VARIANTS)
def test_at_32_steps_it_is_lfi_focus_tiles(gpu, variant):
    case = "g15x15"
    with _ctx(gpu, case, variant) as ctx:
        for grid in [(7, 5), "pixels"]:
            nx, ny = _grid(ctx, grid)
            ctx.poison(poison.FOCUS, poison._byte(None))
            old = ctx.focus_tiles(nx, ny) + (ctx.focus_tiles_pixels,)
            old_passes = ctx.focus_tiles_passes()
            ctx.poison(poison.FOCUS, poison._byte(None))
            new = _tiles_steps_raw(ctx, nx, ny, 32)
            assert _same(old, new), grid
            assert ctx.focus_tiles_passes() == old_passes == (1 if variant != "packed_p2" else 0)
        hp, _ = _case(case)
        _check(ctx, hp, _costs(case, 32), (7, 5), 32)


# ---- 4. independent of the map's setting ----------------------------------------------------------------------------------------------

def test_the_maps_setting_and_the_tiles_argument_do_not_meet(gpu, oracle_c):
    case = "g8x8_ids5"
    hp, lf = _case(case)
    want32 = oracle_c.focus_estimate(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)
    with _ctx(gpu, case) as ctx:
        ctx.set_focus_steps(128)
        _check(ctx, hp, _costs(case, 64), (3, 2), 64, factored=True)
        assert ctx.focus_steps() == 128
        ctx.set_focus_steps(32)
        _check(ctx, hp, _costs(case, 96), (3, 2), 96, factored=True)
        assert ctx.focus_steps() == 32
        poison.focus_map(ctx)
        assert (ctx.download_map(0) == want32).all()
        assert (ctx.download_map(1) == oracle_c.focus_filter(want32, hp.block_radius)).all()


def test_tiles_of_128_then_the_map_of_32(gpu, oracle_c):
    case = "g3x3"
    hp, lf = _case(case)
    with _ctx(gpu, case) as ctx:
        assert ctx.focus_steps() == 32
        ctx.poison(poison.FOCUS, poison._byte(None))
        cost, best, f = ctx.focus_tiles(3, 2, steps=128)
        assert ctx.focus_tiles_passes() == 4
        want = _tile_sums(ref.pixel_costs(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, 128), ctx.width, ctx.height, 3, 2)
        assert (cost == want).all()
        ctx.poison(L.LFI_POISON_MAPS, poison._byte(None))     # not the workspace: the map runs on the planes the tiles left
        ctx.focus_map()
        ctx.sync()
        assert ctx.focus_steps() == 32
        assert (ctx.download_map(0) == oracle_c.focus_estimate(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)).all()


# ---- 5. state -------------------------------------------------------------------------------------------------------------------------

def test_poison_before_the_call_changes_nothing(gpu):
    case = "g15x15"
    hp, _ = _case(case)
    with _ctx(gpu, case) as ctx:
        plain = ctx.focus_tiles(7, 5, steps=96)
        for byte in poison.POISON + (0x00, 0xFF):
            ctx.poison(L.LFI_POISON_FOCUS_WORKSPACE, byte)
            assert _same(plain, ctx.focus_tiles(7, 5, steps=96)), byte
        _check(ctx, hp, _costs(case, 96), (7, 5), 96, factored=True)


@pytest.mark.parametrize("variant", ["auto", "packed_p2"])
def test_the_call_leaves_maps_and_views_alone_and_keeps_the_padded_plane_cache_right(gpu, oracle_c, variant):
    case, steps = "g8x8_ids5", 64
    hp, lf = _case(case)
    costs = _costs(case, steps)
    factored = variant != "packed_p2"
    with _ctx(gpu, case, variant) as ctx:
        want0 = oracle_c.focus_estimate(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)
        poison.focus_map(ctx)
        maps = [ctx.download_map(0), ctx.download_map(1)]
        assert (maps[0] == want0).all()
        poison.render(ctx, "STD")
        views = ctx.download_views()
        mem = ctx.memory_info().workspace_bytes
        # no poison here: the estimate's padded planes and workspace are shared with the call
        _check(ctx, hp, costs, (7, 5), steps, poisoned=False, factored=factored)
        assert ctx.memory_info().workspace_bytes > mem     # the tiles' memory is counted
        assert (ctx.download_map(0) == maps[0]).all() and (ctx.download_map(1) == maps[1]).all()
        assert (ctx.download_views() == views).all()
        # the maps poisoned, then the tiles: the call writes no map byte
        ctx.poison(L.LFI_POISON_MAPS, 0x77)
        _check(ctx, hp, costs, (3, 2), steps, poisoned=False, factored=factored)
        assert (ctx.download_map(0) == 0x77).all() and (ctx.download_map(1) == 0x77).all()
        ctx.focus_map()   # on the planes the tiles left
        ctx.sync()
        assert (ctx.download_map(0) == maps[0]).all() and (ctx.download_map(1) == maps[1]).all()
        # one sampled image replaced, then the tiles (they re-pad that plane), then the map on the cache the tiles left
        g = int(hp.focus_map_ids[1])
        lf2 = lf.copy()
        lf2[g] = lf[g][::-1, ::-1]
        ctx.upload_image(g, lf2[g])
        costs2 = ref.pixel_costs(lf2, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, steps)
        _check(ctx, hp, costs2, (7, 5), steps, poisoned=False, factored=factored)
        ctx.focus_map()
        ctx.sync()
        want2 = oracle_c.focus_estimate(lf2, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)
        assert (ctx.download_map(0) == want2).all()
        assert not (want2 == want0).all()
        # and the other way round: the map re-pads, the tiles reuse
        ctx.upload_image(g, lf[g])
        ctx.focus_map()
        _check(ctx, hp, costs, (7, 5), steps, poisoned=False, factored=factored)
        assert (ctx.download_map(0) == maps[0]).all() and (ctx.download_map(1) == maps[1]).all()


@pytest.mark.parametrize("variant", ["auto", "factored_direct"])
def test_fine_map_and_fine_tiles_follow_each_other(gpu, oracle_c, variant):
    """the map's carry plane in use (lfi_set_focus_steps(128)) before and after fine tiles: both give their restatements, in either order"""
    fz = next(c for c in FUZZ if c[0] == "f3_4x4_96x64_r4x2")
    hp, lf = fuzz_case(L, oracle_c, fz)
    W, H = fz[3], fz[4]
    want_map = sref.map0(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, 128)
    costs = ref.pixel_costs(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, 96)
    with gpu.Context(0) as ctx:
        ctx.set_grid(fz[1], fz[2], W, H)
        ctx.upload_grid(lf)
        ctx.set_params(hp)
        ctx.set_variant("FOCUS", variant)
        ctx.set_focus_steps(128)
        for _ in range(2):
            ctx.poison(L.LFI_POISON_MAPS, poison._byte(None))
            ctx.focus_map()
            ctx.sync()
            assert (ctx.download_map(0) == want_map).all()
            _check(ctx, hp, costs, (7, 5), 96, poisoned=False, factored=True)
        poison.focus_map(ctx)
        assert (ctx.download_map(0) == want_map).all()


# ---- 6. a second implementation on the device, at the size where dispatch changes ----------------------------------------------------

def test_large_frame_equals_focus_curve_per_tile_on_the_device(gpu):
    """8 x 8 @1080p, 16 x 9 tiles, 128 candidates against lfi_focus_curve(rect, 128) per tile on the same context"""
    cols, rows, W, H, steps = 8, 8, 1920, 1080, 128
    hp = gpu.build_params(cols, rows, W, H, "0,0,1,1", 0.0, 0.5, 3.0, 1.0, 4)
    assert _has_negative_shifts(hp)
    with gpu.Context(0) as ctx:
        ctx.set_grid(cols, rows, W, H)
        ctx.set_params(hp)
        ctx.fill_synthetic_scene(0x1F1F)
        ctx.poison(poison.FOCUS, poison._byte(None))
        cost, best, f = ctx.focus_tiles(16, 9, steps=steps)
        assert ctx.focus_tiles_passes() == 4
        pixels = ctx.focus_tiles_pixels                  # of the 16 x 9 call: the next call replaces the attribute
        whole, whole_best, whole_f = ctx.focus_tiles(1, 1, steps=steps)
        assert ctx.focus_tiles_passes() == 4
        assert ctx.focus_tiles_pixels[0, 0] == W * H
        assert (whole[0, 0] == cost.sum(axis=(0, 1), dtype=np.uint64)).all()
        for ty in range(9):
            for tx in range(16):
                rect = L.focus_tile_rect(W, H, 16, 9, tx, ty)
                c, b, bf = ctx.focus_curve(*rect, steps=steps)
                assert (cost[ty, tx] == c).all(), (tx, ty, cost[ty, tx], c)
                assert best[ty, tx] == b and f[ty, tx].view(np.uint32) == np.float32(bf).view(np.uint32), (tx, ty)
                assert pixels[ty, tx] == ctx.focus_curve_pixels == (rect[2] - rect[0]) * (rect[3] - rect[1])
        c, b, bf = ctx.focus_curve(0, 0, W, H, steps=steps)
        assert (whole[0, 0] == c).all() and whole_best[0, 0] == b
        assert whole_f[0, 0].view(np.uint32) == np.float32(bf).view(np.uint32)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------

def _refused(ctx, *args, **kw):
    with pytest.raises(L.LfiError, match=r"lfi error -1:"):
        ctx.focus_tiles(*args, **kw)


def test_refusals_return_einval_and_leave_the_context_usable(gpu):
    with gpu.Context(0) as fresh:
        _refused(fresh, 1, 1, steps=64)                 # no grid
        fresh.set_grid(3, 3, 32, 8)
        _refused(fresh, 1, 1, steps=64)                 # no parameters
    case = "g3x3"
    hp, lf = _case(case)
    costs = _costs(case, 64)
    with _ctx(gpu, case) as ctx:
        W, H = ctx.width, ctx.height                    # 300 x 40
        for bad in (0, 31, 33, 288, -32):
            with pytest.raises(L.LfiError, match=r"lfi error -1:.*lfi_focus_tiles_steps"):
                ctx.focus_tiles(3, 2, steps=bad)
            _check(ctx, hp, costs, (3, 2), 64)          # a following valid call succeeds
        for grid in [(0, 1), (1, 0), (-2, 3), (3, -2), (257, 1), (1, H + 1), (1, 257), (300, 1)]:
            _refused(ctx, *grid, steps=64)
        _check(ctx, hp, costs, (3, 2), 64)
        res = (L.abi.FocusCurveResult * 6)()
        assert ctx._lib.lfi_focus_tiles_steps(ctx._h, 3, 2, 64, None, None) == -1        # out == NULL
        assert ctx._lib.lfi_focus_tiles_steps(None, 3, 2, 64, None, res) == -1
        ctx.set_params(dataclasses.replace(hp, range=0.0))
        _refused(ctx, 3, 2, steps=64)                   # range <= 0
        ctx.set_params(dataclasses.replace(hp, range=-0.25))
        _refused(ctx, 3, 2, steps=64)
        ctx.set_params(dataclasses.replace(hp, focus_map_ids=np.zeros(0, np.int32)))
        _refused(ctx, 3, 2, steps=64)                   # n_focus_ids == 0
        ctx.set_params(hp)
        _check(ctx, hp, costs, (3, 2), 64)              # still usable, and right
        # out_cost may be NULL
        assert ctx._lib.lfi_focus_tiles_steps(ctx._h, 3, 2, 64, None, res) == 0
        want = _tile_sums(costs, W, H, 3, 2)
        for t in range(6):
            rect = L.focus_tile_rect(W, H, 3, 2, t % 3, t // 3)
            assert res[t].best_index == ref.first_min(want[t // 3, t % 3]) and res[t].pixels == (rect[2] - rect[0]) * (rect[3] - rect[1])
        ctx.set_row_window(0, H // 2, 0, H)
        ctx.set_params(hp)
        _refused(ctx, 3, 2, steps=64)                   # a row window
    with _ctx(gpu, case) as ctx:
        ctx.render("TEN_WM")
        ctx.release_inputs()
        _refused(ctx, 3, 2, steps=64)                   # the RGBA planes are gone
        ctx.render("TEN_WM")
        ctx.sync()


# ---- 8. the command line --------------------------------------------------------------------------------------------------------------

def _write_scene(tmp_path, lf, cols, rows):
    """the grid as files row_column.png (image id = col * rows + row)"""
    d = tmp_path / "scene"
    d.mkdir()
    for col in range(cols):
        for row in range(rows):
            L.write_png(str(d / f"{row:02d}_{col:02d}.png"), lf[col * rows + row])
    return str(d)


def test_cli_tile_steps_and_whole_frame_autofocus_on_the_two_depth_scene(gpu, tmp_path):
    P = ref.PLANTED
    hp, lf = two_depth_scene(gpu)
    W, H, V = P["W"], P["H"], 4
    scene = _write_scene(tmp_path, lf, P["cols"], P["rows"])
    common = ["-i", scene, "-t", P["traj"], "-m", "STD", "-n", str(V), "-b", "1"]
    search = ["-f", str(P["focus"]), "-r", str(P["rng"])]
    with gpu.Context(0) as ctx:
        ctx.set_grid(P["cols"], P["rows"], W, H)
        ctx.upload_grid(lf)
        ctx.set_params(gpu.build_params(P["cols"], P["rows"], W, H, P["traj"], P["focus"], P["rng"], 3.0, 1.0, V))
        _, best64, f64 = ctx.focus_tiles(4, 3, steps=64)
        _, best128, _ = ctx.focus_tiles(16, 9, steps=128)
        want_f, want_r, lo, hi = L.focus_auto_range(best128, P["focus"], P["rng"], steps=128)
        ctx.set_params(gpu.build_params(P["cols"], P["rows"], W, H, P["traj"], float(want_f), float(want_r), 3.0, 1.0, V))
        ctx.set_focus_steps(128)
        poison.focus_map(ctx)
        want_map = ctx.download_map(0)
    # --focus-tiles 4x3 --tile-steps 64: the library's indices and candidates
    res = run_cli(gpu, *common, *search, "-o", str(tmp_path / "tiles"), "--focus-tiles", "4x3", "--tile-steps", "64")
    assert res.returncode == 0, res.stderr
    assert re.search(r"^focus tiles: 4 x 3$", res.stdout, re.M), res.stdout
    lines = re.findall(r"^tile (\d+) (\d+) index (\d+) focus (\S+)$", res.stdout, re.M)
    assert [(int(a), int(b)) for a, b, _, _ in lines] == [(tx, ty) for ty in range(3) for tx in range(4)], res.stdout
    assert [int(i) for _, _, i, _ in lines] == [int(b) for b in best64.ravel()]
    assert max(int(i) for _, _, i, _ in lines) >= 32                            # indices 32 steps could not print
    for (_, _, i, f), want in zip(lines, f64.ravel()):
        assert np.float32(float(f)).view(np.uint32) == want.view(np.uint32), (i, f)
    # --auto-range --tile-steps 128 --map-steps 128: the interval of lfi_host_focus_auto_range_steps, the library's map inside it
    auto = run_cli(gpu, *common, *search, "-o", str(tmp_path / "auto"), "--auto-range", "--tile-steps", "128", "--map-steps", "128")
    assert auto.returncode == 0, auto.stderr
    m = re.search(r"^auto-range: focus (\S+) range (\S+) \(candidates (\d+)\.\.(\d+)\)$", auto.stdout, re.M)
    assert m, auto.stdout
    assert (int(m.group(3)), int(m.group(4))) == (lo, hi)
    assert np.float32(float(m.group(1))).view(np.uint32) == want_f.view(np.uint32) and np.float32(float(m.group(2))).view(np.uint32) == want_r.view(np.uint32)
    got = L.load_image(str(tmp_path / "auto" / "map0.png"))
    assert (got[..., :3] == want_map[..., :3]).all()
    # whole-frame --autofocus with explicit steps (the frame as one tile) prints what the rectangle's curve prints
    one = run_cli(gpu, *common, *search, "-o", str(tmp_path / "af_tile"), "--autofocus", "--autofocus-steps", "64")
    two = run_cli(gpu, *common, *search, "-o", str(tmp_path / "af_curve"), "--autofocus", f"0,0,{W},{H}", "--autofocus-steps", "64")
    assert one.returncode == 0 and two.returncode == 0, (one.stderr, two.stderr)
    line = [re.search(r"^autofocus: .*$", r.stdout, re.M) for r in (one, two)]
    assert line[0] and line[1] and line[0].group(0) == line[1].group(0), (one.stdout, two.stdout)
    assert re.search(r"\(candidate \d+ of 64, %d px\)" % (W * H), line[0].group(0)), line[0].group(0)
    # --tile-steps needs one of the two
    bad = run_cli(gpu, *common, *search, "-o", str(tmp_path / "bad"), "--tile-steps", "64")
    assert bad.returncode != 0 and "--tile-steps" in bad.stderr and "--focus-tiles" in bad.stderr
    assert not (tmp_path / "bad").exists()
