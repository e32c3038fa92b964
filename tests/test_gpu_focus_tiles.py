"""GPU (-m gpu): focus tiles — lfi_focus_tiles, every tile's focus curve from one factored estimate, and the CLI's --focus-tiles / --auto-range.

Every tile's cost[] is compared for u64 EQUALITY with the numpy restatement (tests/focus_curve_ref.py, anchored to the oracle by
tests/test_host_focus_curve.py) over the rectangle of lfinterpolator_amd.focus_tile_rect; best_index is the first minimum of the returned
costs, best_focus that candidate bit for bit, pixels the rectangle's area.  No tile and no candidate is skipped.  The estimate's workspace
and the curves' memory are poisoned before every call a check reads, with alternating bytes."""
import dataclasses
import re

import numpy as np
import pytest

import focus_curve_ref as ref
import focus_routes
import lfinterpolator_amd as L
import poison
from test_host_focus_tiles import two_depth_scene
from view_rows import run_cli

pytestmark = pytest.mark.gpu

# name: cols, rows, W, H, trajectory, focus, range, seed, n_focus_ids (None: what build_params selects), block radius (None: build_params')
# The trajectories' centres lie inside the grid: images on either side, shifts of both signs — flagged rows and columns exist (asserted).
CASES = {
    "g3x3": (3, 3, 300, 40, "0,0,1,1", 0.1, 0.3, 0x1F1F, None, None),                    # 9 ids, block radius 4 x 1: two pixels per lane
    "g8x8_ids5": (8, 8, 96, 24, "0.3,0.6,0.5,0.1", 0.0, 0.5, 5, 5, None),                # n_focus_ids < 32
    "g15x15": (15, 15, 131, 33, "0.071,0.071,0.93,0.93", 0.22, 0.17, 99, None, None),    # 32 of 225 images, odd sizes
    "g8x8_r2x2": (8, 8, 96, 24, "0.3,0.6,0.5,0.1", 0.0, 0.5, 5, 5, (2, 2)),              # an even radius at a width below 128
    "g8x8_r3x1": (8, 8, 96, 24, "0.3,0.6,0.5,0.1", 0.0, 0.5, 5, 5, (3, 1)),              # an odd radius_x: one pixel per lane
    "g8x8_r1x3": (8, 8, 96, 24, "0.3,0.6,0.5,0.1", 0.0, 0.5, 5, 5, (1, 3)),              # radius_x = 1 at a width below 128 (the library's smallest)
    "g15x15_r1x2": (15, 15, 131, 33, "0.071,0.071,0.93,0.93", 0.22, 0.17, 99, None, (1, 2)),
}
GRIDS = [(1, 1), (3, 2), (7, 5), "pixels"]   # "pixels": one pixel per tile (at most 256 tiles per axis: the widest grid where the image is wider)
VARIANTS = ["auto", "factored_direct", "packed_p2"]   # focus_range_t where it applies / focus_range / the fallback through focus_curve_partial


def _setup(gpu, oracle_c, case):
    cols, rows, W, H, traj, focus, rng, seed, n_ids, radius = CASES[case]
    hp = gpu.build_params(cols, rows, W, H, traj, focus, rng, 3.0, 1.783, 3)
    if n_ids is not None:
        hp = dataclasses.replace(hp, focus_map_ids=np.ascontiguousarray(hp.focus_map_ids[:n_ids]))
    if radius is not None:
        hp = dataclasses.replace(hp, block_radius=np.array(radius, np.int32))
    lf = oracle_c.synthetic_lf(cols * rows, W, H, seed)
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, W, H)
    ctx.fill_synthetic(seed)   # the same hash as the oracle's synthetic_lf
    ctx.set_params(hp)
    costs = ref.pixel_costs(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, 32)
    return ctx, hp, lf, costs


def _has_negative_shifts(hp):
    f = ref.candidates(hp.focus, hp.range, 32)
    o = hp.offsets[hp.focus_map_ids]
    return bool((np.outer(f, o[:, 0]) < 0).any() and (np.outer(f, o[:, 1]) < 0).any())


def _grid(ctx, grid):
    return (min(ctx.width, 256), min(ctx.height, 256)) if grid == "pixels" else grid


def _check(ctx, hp, costs, grid, poisoned=True):
    nx, ny = _grid(ctx, grid)
    if poisoned:
        ctx.poison(poison.FOCUS, poison._byte(None))
    cost, best, f = ctx.focus_tiles(nx, ny)
    assert cost.dtype == np.uint64 and cost.shape == (ny, nx, 32) and best.shape == (ny, nx) and f.shape == (ny, nx)
    cand = L.focus_candidates(hp.focus, hp.range, 32)
    W, H = ctx.width, ctx.height
    for ty in range(ny):
        for tx in range(nx):
            rect = L.focus_tile_rect(W, H, nx, ny, tx, ty)
            want = ref.curve(costs, *rect)
            assert (cost[ty, tx] == want).all(), (grid, tx, ty, rect, cost[ty, tx], want)
            assert best[ty, tx] == ref.first_min(want), (grid, tx, ty, best[ty, tx])
            assert f[ty, tx].view(np.uint32) == cand[best[ty, tx]].view(np.uint32), (grid, tx, ty)
            assert ctx.focus_tiles_pixels[ty, tx] == (rect[2] - rect[0]) * (rect[3] - rect[1]), (grid, tx, ty)
    return cost, best, f


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", list(CASES))
def test_every_tiles_curve_equals_the_restatement(gpu, oracle_c, case, variant):
    ctx, hp, lf, costs = _setup(gpu, oracle_c, case)
    assert _has_negative_shifts(hp)
    with ctx:
        ctx.set_variant("FOCUS", variant)
        for grid in GRIDS:
            _check(ctx, hp, costs, grid)
        focus_routes.assert_variant(ctx, variant, hp, 32, "tiles")   # the curves are the named estimate's
        if ctx.width > 256:
            _check(ctx, hp, costs, (ctx.width // 2, ctx.height))   # two pixels per tile where one per tile exceeds the limit
        if case == "g3x3":
            for grid in [(256, 1), (1, 40), (2, 3), (129, 7), (16, 9)]:
                _check(ctx, hp, costs, grid)


def test_tiles_on_the_planes_a_focus_map_left(gpu, oracle_c):
    """the map equals the oracle's, then the tiles reuse the SAME padded planes (no poison in between)"""
    ctx, hp, lf, costs = _setup(gpu, oracle_c, "g3x3")
    with ctx:
        poison.focus_map(ctx)
        want0 = oracle_c.focus_estimate(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)
        assert (ctx.download_map(0) == want0).all()
        _check(ctx, hp, costs, (7, 5), poisoned=False)
        _check(ctx, hp, costs, "pixels", poisoned=False)


def test_poison_before_the_call_changes_nothing(gpu, oracle_c):
    ctx, hp, lf, costs = _setup(gpu, oracle_c, "g15x15")
    with ctx:
        plain = ctx.focus_tiles(7, 5)
        for byte in poison.POISON:
            ctx.poison(L.LFI_POISON_FOCUS_WORKSPACE, byte)
            again = ctx.focus_tiles(7, 5)
            for a, b in zip(plain, again):
                assert (a.view(np.uint32) == b.view(np.uint32)).all() if a.dtype == np.float32 else (a == b).all()
        _check(ctx, hp, costs, (7, 5))


def test_large_frame_equals_focus_curve_per_tile_on_the_device(gpu):
    """8 x 8 @1080p, 16 x 9 tiles against a second implementation on the device: lfi_focus_curve(rect, 32) per tile on the same context"""
    cols, rows, W, H = 8, 8, 1920, 1080
    hp = gpu.build_params(cols, rows, W, H, "0,0,1,1", 0.0, 0.5, 3.0, 1.0, 4)
    assert _has_negative_shifts(hp)
    with gpu.Context(0) as ctx:
        ctx.set_grid(cols, rows, W, H)
        ctx.set_params(hp)
        ctx.fill_synthetic_scene(0x1F1F)
        ctx.poison(poison.FOCUS, poison._byte(None))
        cost, best, f = ctx.focus_tiles(16, 9)
        pixels = ctx.focus_tiles_pixels                  # of the 16 x 9 call: the next call replaces the attribute
        whole, whole_best, whole_f = ctx.focus_tiles(1, 1)
        assert ctx.focus_tiles_pixels[0, 0] == W * H
        assert (whole[0, 0] == cost.sum(axis=(0, 1), dtype=np.uint64)).all()
        for ty in range(9):
            for tx in range(16):
                rect = L.focus_tile_rect(W, H, 16, 9, tx, ty)
                c, b, bf = ctx.focus_curve(*rect, steps=32)
                assert (cost[ty, tx] == c).all(), (tx, ty, cost[ty, tx], c)
                assert best[ty, tx] == b and f[ty, tx].view(np.uint32) == np.float32(bf).view(np.uint32), (tx, ty)
                assert pixels[ty, tx] == ctx.focus_curve_pixels == (rect[2] - rect[0]) * (rect[3] - rect[1])
        c, b, bf = ctx.focus_curve(0, 0, W, H, steps=32)
        assert (whole[0, 0] == c).all() and whole_best[0, 0] == b


@pytest.mark.parametrize("variant", ["auto", "packed_p2"])
def test_the_call_leaves_maps_and_views_alone_and_keeps_the_padded_plane_cache_right(gpu, oracle_c, variant):
    ctx, hp, lf, costs = _setup(gpu, oracle_c, "g8x8_ids5")
    with ctx:
        ctx.set_variant("FOCUS", variant)
        W, H = ctx.width, ctx.height
        want0 = oracle_c.focus_estimate(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)
        poison.focus_map(ctx)
        maps = [ctx.download_map(0), ctx.download_map(1)]
        assert (maps[0] == want0).all()
        poison.render(ctx, "STD")
        views = ctx.download_views()
        mem = ctx.memory_info().workspace_bytes
        # no poison here: the estimate's padded planes and workspace are shared with the call
        _check(ctx, hp, costs, (7, 5), poisoned=False)
        assert ctx.memory_info().workspace_bytes > mem     # the tiles' memory is counted
        assert (ctx.download_map(0) == maps[0]).all() and (ctx.download_map(1) == maps[1]).all()
        assert (ctx.download_views() == views).all()
        # the maps poisoned, then the tiles: the call writes no map byte
        ctx.poison(L.LFI_POISON_MAPS, 0x77)
        _check(ctx, hp, costs, (3, 2), poisoned=False)
        assert (ctx.download_map(0) == 0x77).all() and (ctx.download_map(1) == 0x77).all()
        ctx.focus_map()   # on the planes the tiles left
        ctx.sync()
        assert (ctx.download_map(0) == maps[0]).all() and (ctx.download_map(1) == maps[1]).all()
        # one sampled image replaced, then the tiles (they re-pad that plane), then the map on the cache the tiles left
        g = int(hp.focus_map_ids[1])
        lf2 = lf.copy()
        lf2[g] = lf[g][::-1, ::-1]
        ctx.upload_image(g, lf2[g])
        costs2 = ref.pixel_costs(lf2, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, 32)
        _check(ctx, hp, costs2, (7, 5), poisoned=False)
        ctx.focus_map()
        ctx.sync()
        want2 = oracle_c.focus_estimate(lf2, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)
        assert (ctx.download_map(0) == want2).all()
        assert not (want2 == want0).all()
        # and the other way round: the map re-pads, the tiles reuse
        ctx.upload_image(g, lf[g])
        ctx.focus_map()
        _check(ctx, hp, costs, (7, 5), poisoned=False)
        assert (ctx.download_map(0) == maps[0]).all() and (ctx.download_map(1) == maps[1]).all()
        poison.render(ctx, "STD")
        assert (ctx.download_views() == views).all()


def _refused(ctx, *args):
    with pytest.raises(L.LfiError, match=r"lfi error -1:"):
        ctx.focus_tiles(*args)


def test_refusals_return_einval_and_leave_the_context_usable(gpu, oracle_c):
    with gpu.Context(0) as fresh:
        _refused(fresh, 1, 1)                           # no grid
        fresh.set_grid(3, 3, 32, 8)
        _refused(fresh, 1, 1)                           # no parameters
    ctx, hp, lf, costs = _setup(gpu, oracle_c, "g3x3")
    with ctx:
        W, H = ctx.width, ctx.height                    # 300 x 40
        for grid in [(0, 1), (1, 0), (-2, 3), (3, -2), (257, 1), (1, H + 1), (1, 257), (300, 1)]:
            _refused(ctx, *grid)
            _check(ctx, hp, costs, (3, 2))              # a following valid call succeeds
        res = (L.abi.FocusCurveResult * 6)()
        assert ctx._lib.lfi_focus_tiles(ctx._h, 3, 2, None, None) == -1        # out == NULL
        assert ctx._lib.lfi_focus_tiles(None, 3, 2, None, res) == -1
        ctx.set_params(dataclasses.replace(hp, range=0.0))
        _refused(ctx, 3, 2)                             # range <= 0
        ctx.set_params(dataclasses.replace(hp, range=-0.25))
        _refused(ctx, 3, 2)
        ctx.set_params(dataclasses.replace(hp, focus_map_ids=np.zeros(0, np.int32)))
        _refused(ctx, 3, 2)                             # n_focus_ids == 0
        ctx.set_params(hp)
        _check(ctx, hp, costs, (3, 2))                  # still usable, and right
        # out_cost may be NULL
        assert ctx._lib.lfi_focus_tiles(ctx._h, 3, 2, None, res) == 0
        for t in range(6):
            rect = L.focus_tile_rect(W, H, 3, 2, t % 3, t // 3)
            want = ref.curve(costs, *rect)
            assert res[t].best_index == ref.first_min(want) and res[t].pixels == (rect[2] - rect[0]) * (rect[3] - rect[1])
        ctx.set_row_window(0, H // 2, 0, H)
        ctx.set_params(hp)
        _refused(ctx, 3, 2)                             # a row window
    ctx, hp, lf, costs = _setup(gpu, oracle_c, "g3x3")
    with ctx:
        ctx.render("TEN_WM")
        ctx.release_inputs()
        _refused(ctx, 3, 2)                             # the RGBA planes are gone
        ctx.render("TEN_WM")
        ctx.sync()


def _write_scene(tmp_path, lf, cols, rows):
    """the grid as files row_column.png (image id = col * rows + row)"""
    d = tmp_path / "scene"
    d.mkdir()
    for col in range(cols):
        for row in range(rows):
            L.write_png(str(d / f"{row:02d}_{col:02d}.png"), lf[col * rows + row])
    return str(d)


def test_cli_focus_tiles_and_auto_range_on_the_two_depth_scene(gpu, tmp_path):
    P = ref.PLANTED
    hp, lf = two_depth_scene(gpu)
    scene = _write_scene(tmp_path, lf, P["cols"], P["rows"])
    V = 4
    common = ["-i", scene, "-t", P["traj"], "-m", "STD", "-n", str(V), "-b", "1"]
    search = ["-f", str(P["focus"]), "-r", str(P["rng"])]
    res = run_cli(gpu, *common, *search, "-o", str(tmp_path / "tiles"), "--focus-tiles", "4x1")
    assert res.returncode == 0, res.stderr
    assert re.search(r"^focus tiles: 4 x 1$", res.stdout, re.M), res.stdout
    lines = re.findall(r"^tile (\d+) (\d+) index (\d+) focus (\S+)$", res.stdout, re.M)
    assert [(int(a), int(b)) for a, b, _, _ in lines] == [(0, 0), (1, 0), (2, 0), (3, 0)], res.stdout
    cand = L.focus_candidates(P["focus"], P["rng"], 32)
    assert int(lines[0][2]) == 9 and int(lines[3][2]) == 22, lines
    for _, _, i, f in lines:
        assert np.float32(float(f)).view(np.uint32) == cand[int(i)].view(np.uint32), (i, f)
    # the same tiles through the library
    with gpu.Context(0) as ctx:
        ctx.set_grid(P["cols"], P["rows"], P["W"], P["H"])
        ctx.upload_grid(lf)
        ctx.set_params(gpu.build_params(P["cols"], P["rows"], P["W"], P["H"], P["traj"], P["focus"], P["rng"], 3.0, 1.0, V))
        cost, best, f = ctx.focus_tiles(4, 1)
    assert [int(i) for _, _, i, _ in lines] == [int(b) for b in best[0]]
    # --auto-range: candidates 8..23, then the render of that interval
    auto = run_cli(gpu, *common, *search, "-o", str(tmp_path / "auto"), "--auto-range", "4x1")
    assert auto.returncode == 0, auto.stderr
    m = re.search(r"^auto-range: focus (\S+) range (\S+) \(candidates (\d+)\.\.(\d+)\)$", auto.stdout, re.M)
    assert m, auto.stdout
    assert (int(m.group(3)), int(m.group(4))) == (8, 23)
    want_f, want_r, lo, hi = L.focus_auto_range(best, P["focus"], P["rng"])
    assert (lo, hi) == (8, 23)
    assert np.float32(float(m.group(1))).view(np.uint32) == want_f.view(np.uint32) and np.float32(float(m.group(2))).view(np.uint32) == want_r.view(np.uint32)
    hand = run_cli(gpu, *common, "-f", m.group(1), "-r", m.group(2), "-o", str(tmp_path / "hand"))
    assert hand.returncode == 0, hand.stderr
    names = sorted(p.name for p in (tmp_path / "auto").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "hand").iterdir()) == sorted([f"{v:02d}.png" for v in range(V)] + ["map0.png", "map1.png"])
    for name in names:
        assert (tmp_path / "auto" / name).read_bytes() == (tmp_path / "hand" / name).read_bytes(), name
    # the default grid
    res = run_cli(gpu, *common, *search, "-o", str(tmp_path / "auto169"), "--auto-range")
    assert res.returncode == 0, res.stderr
    assert re.search(r"^auto-range: focus \S+ range \S+ \(candidates \d+\.\.\d+\)$", res.stdout, re.M), res.stdout
