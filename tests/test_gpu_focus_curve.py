"""GPU (-m gpu): autofocus — lfi_focus_curve, the focus curve of a region reduced on the device, and the CLI's --autofocus.

cost[] is compared for u64 EQUALITY with the numpy restatement (tests/focus_curve_ref.py, anchored to the oracle by
tests/test_host_focus_curve.py); best_index is the first minimum of the returned costs and best_focus that candidate bit for bit.  The
curve's device memory (partial sums, the curve, the result) is poisoned before every call a check reads, with alternating bytes."""
import dataclasses
import re

import numpy as np
import pytest

import focus_curve_ref as ref
import lfinterpolator_amd as L
import poison
from view_rows import run_cli

pytestmark = pytest.mark.gpu

# name, cols, rows, W, H, trajectory, focus, range, seed, n_focus_ids (None: what build_params selects)
CASES = {
    "g3x3": ("g3x3", 3, 3, 300, 40, "0,0,1,1", 0.1, 0.3, 0x1F1F, None),                    # 9 ids, block radius 4 x 1
    "g8x8": ("g8x8", 8, 8, 203, 29, "0.0,0.0,1.0,1.0", -0.1, 0.4, 0x2B2B, None),           # 32 of 64 images, an odd width
    "g15x15": ("g15x15", 15, 15, 131, 33, "0.071,0.071,0.93,0.93", 0.22, 0.17, 99, None),  # 32 of 225 images
    "g8x8_ids5": ("g8x8_ids5", 8, 8, 96, 24, "0.3,0.6,0.5,0.1", 0.0, 0.5, 5, 5),           # n_focus_ids < 32
    "g4x4_far": ("g4x4_far", 4, 4, 64, 20, "0,0,1,1", 3.0, 9.0, 11, None),                 # shifts larger than the image: the outer images are clamped everywhere
}


def _setup(gpu, oracle_c, case, steps=(32,)):
    name, cols, rows, W, H, traj, focus, rng, seed, n_ids = CASES[case]
    hp = gpu.build_params(cols, rows, W, H, traj, focus, rng, 3.0, 1.783, 3)
    if n_ids is not None:
        hp = dataclasses.replace(hp, focus_map_ids=np.ascontiguousarray(hp.focus_map_ids[:n_ids]))
    lf = oracle_c.synthetic_lf(cols * rows, W, H, seed)
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, W, H)
    ctx.fill_synthetic(seed)   # the same hash as the oracle's synthetic_lf
    ctx.set_params(hp)
    costs = {s: ref.pixel_costs(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, s) for s in steps}
    return ctx, hp, lf, costs


def _curve(ctx, region, steps=32):
    """poison the curve's memory (and the rest of the focus workspace), then the call"""
    ctx.poison(poison.FOCUS, poison._byte(None))
    return ctx.focus_curve(*region, steps=steps)


def _check(ctx, hp, costs, region, steps=32):
    cost, best, f = _curve(ctx, region, steps)
    want = ref.curve(costs[steps], *region)
    assert cost.dtype == np.uint64 and (cost == want).all(), (region, steps, cost, want)
    assert best == ref.first_min(cost), (region, steps, best)
    cand = L.focus_candidates(hp.focus, hp.range, steps)
    assert np.float32(f).view(np.uint32) == cand[best].view(np.uint32), (region, steps, f, cand[best])
    assert ctx.focus_curve_pixels == (region[2] - region[0]) * (region[3] - region[1])
    return cost, best


@pytest.mark.parametrize("case", list(CASES))
def test_whole_frame_corners_and_clamping_pixels_equal_the_restatement(gpu, oracle_c, case):
    ctx, hp, lf, costs = _setup(gpu, oracle_c, case)
    with ctx:
        W, H = ctx.width, ctx.height
        _check(ctx, hp, costs, (0, 0, W, H))
        # 1 x 1 regions: the four corners, and pixels next to every edge whose taps clamp
        for x, y in [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (1, H // 2), (W - 2, H // 2), (W // 2, 1), (W // 2, H - 2), (W // 2, H // 2)]:
            _check(ctx, hp, costs, (x, y, x + 1, y + 1))
        _check(ctx, hp, costs, (0, H // 2, W, H // 2 + 1))   # one pixel high
        _check(ctx, hp, costs, (W // 3, 0, W // 3 + 1, H))   # one pixel wide
    if case == "g4x4_far":
        # shifts larger than the image at every candidate: the outer images show their clamped edge everywhere
        f = ref.candidates(hp.focus, hp.range, 32)
        assert (np.abs(hp.offsets).max(axis=0) * np.abs(f).min() > np.array([W, H])).all()


def test_region_edges_at_every_residue_mod_64(gpu, oracle_c):
    """x0 and x1 at every residue mod 64 (and so mod 4: the lanes' pixel pairs, the wave's 128 pixels); regions up to three waves wide"""
    ctx, hp, lf, costs = _setup(gpu, oracle_c, "g3x3")
    with ctx:
        seen0, seen1 = set(), set()
        for r in range(64):
            x0, x1 = (r * 29) % 64, 150 + r + (64 if r % 3 == 0 else 0)
            seen0.add(x0 % 64), seen1.add(x1 % 64)
            _check(ctx, hp, costs, (x0, 5 + r % 7, x1, 5 + r % 7 + 1 + r % 11))
        assert len(seen0) == 64 and len(seen1) == 64
        for x0 in range(4):
            for x1 in range(x0 + 1, x0 + 6):
                _check(ctx, hp, costs, (x0 + 128, 0, x1 + 128, 3))   # narrower than a lane's pixels, at a wave's seam


@pytest.mark.parametrize("case", ["g3x3", "g8x8_ids5"])
def test_steps_are_a_runtime_value(gpu, oracle_c, case):
    steps = (2, 7, 32, 256)
    ctx, hp, lf, costs = _setup(gpu, oracle_c, case, steps)
    with ctx:
        W, H = ctx.width, ctx.height
        for s in steps:
            _check(ctx, hp, costs, (0, 0, W, H), s)
            _check(ctx, hp, costs, (7, 3, W - 9, H - 2), s)
            _check(ctx, hp, costs, (W - 1, H - 1, W, H), s)


def test_a_tie_goes_to_the_first_candidate(gpu):
    """an all-equal light field: every candidate's cost is 0 (the dropped FLT_MIN terms are the only place where the float code would differ):
    candidate 0 wins"""
    cols, rows, W, H = 3, 3, 70, 9
    hp = gpu.build_params(cols, rows, W, H, "0,0,1,1", 0.0, 0.5, 3.0, 1.0, 2)
    with gpu.Context(0) as ctx:
        ctx.set_grid(cols, rows, W, H)
        for value in (0, 200):
            lf = np.full((cols * rows, H, W, 4), value, np.uint8)
            lf[..., 3] = 255
            ctx.upload_grid(lf)
            ctx.set_params(hp)
            for steps in (2, 32, 256):
                cost, best, f = _curve(ctx, (0, 0, W, H), steps)
                assert (cost == 0).all() and best == 0 and np.float32(f) == np.float32(hp.focus)


@pytest.mark.parametrize("k", ref.PLANTED["ks"])
def test_planted_scene_is_found(gpu, k):
    P = ref.PLANTED
    hp = gpu.build_params(P["cols"], P["rows"], P["W"], P["H"], P["traj"], P["focus"], P["rng"], 3.0, 1.0, 2)
    lf = ref.planted_scene(hp.offsets, k, **P)
    costs = {P["steps"]: ref.pixel_costs(lf, hp.offsets, hp.focus_map_ids, P["focus"], P["rng"], hp.block_radius, P["steps"])}
    with gpu.Context(0) as ctx:
        ctx.set_grid(P["cols"], P["rows"], P["W"], P["H"])
        ctx.upload_grid(lf)
        ctx.set_params(hp)
        for region in ref.PLANTED_REGIONS:
            cost, best = _check(ctx, hp, costs, region, P["steps"])
            assert best == k and cost[k] == 0 and (np.delete(cost, k) > 0).all(), (region, best, cost)


@pytest.mark.parametrize("case", ["g3x3", "g8x8", "g15x15"])
def test_one_pixel_curves_agree_with_the_products_own_map(gpu, oracle_c, case):
    ctx, hp, lf, costs = _setup(gpu, oracle_c, case)
    with ctx:
        poison.focus_map(ctx)
        map0 = ctx.download_map(0)
        W, H = ctx.width, ctx.height
        rs = np.random.RandomState(3)
        pixels = [(0, 0), (W - 1, H - 1)] + [(int(rs.randint(W)), int(rs.randint(H))) for _ in range(24)]
        for x, y in pixels:
            cost, best, f = _curve(ctx, (x, y, x + 1, y + 1))
            assert cost.min() >= 1      # hash noise: the FLT_MIN departure plays no part
            assert ref.map_byte(f, hp.focus, hp.range) == map0[y, x, 0], (x, y, best)


@pytest.mark.parametrize("variant", ["auto", "packed_p2"])
def test_the_call_leaves_maps_views_and_the_estimates_cache_alone(gpu, oracle_c, variant):
    ctx, hp, lf, costs = _setup(gpu, oracle_c, "g8x8")
    with ctx:
        ctx.set_variant("FOCUS", variant)
        W, H = ctx.width, ctx.height
        poison.focus_map(ctx)
        maps = [ctx.download_map(0), ctx.download_map(1)]
        want0 = oracle_c.focus_estimate(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)
        assert (maps[0] == want0).all()
        poison.render(ctx, "STD")
        views = ctx.download_views()
        mem = ctx.memory_info().workspace_bytes
        # no poison here: the estimate's padded planes and workspace are to survive the call as they are
        cost, best, f = ctx.focus_curve(0, 0, W, H)
        assert (cost == ref.curve(costs[32], 0, 0, W, H)).all()
        assert ctx.memory_info().workspace_bytes > mem     # the curve's memory is counted
        assert (ctx.download_map(0) == maps[0]).all() and (ctx.download_map(1) == maps[1]).all()
        assert (ctx.download_views() == views).all()
        ctx.focus_map()   # on the kept planes
        ctx.sync()
        assert (ctx.download_map(0) == maps[0]).all() and (ctx.download_map(1) == maps[1]).all()
        ctx.focus_curve(3, 2, 90, 20)
        poison.focus_map(ctx)
        assert (ctx.download_map(0) == maps[0]).all() and (ctx.download_map(1) == maps[1]).all()
        poison.render(ctx, "STD")
        assert (ctx.download_views() == views).all()


def test_per_view_offsets_do_not_affect_the_curve(gpu, oracle_c):
    ctx, hp, lf, costs = _setup(gpu, oracle_c, "g3x3")
    with ctx:
        rs = np.random.RandomState(1)
        ctx.set_view_float_offsets(rs.uniform(-5, 5, size=(3, 9, 2)).astype(np.float32))
        ctx.set_view_offsets(rs.randint(-5, 5, size=(3, 9, 2)).astype(np.int32))
        _check(ctx, hp, costs, (2, 1, 260, 37))


def _refused(ctx, *args, **kw):
    with pytest.raises(L.LfiError, match=r"lfi error -1:"):
        ctx.focus_curve(*args, **kw)


def test_refusals_return_einval_and_leave_the_context_usable(gpu, oracle_c):
    with gpu.Context(0) as fresh:
        _refused(fresh, 0, 0, 1, 1)                     # no grid
        fresh.set_grid(3, 3, 32, 8)
        _refused(fresh, 0, 0, 1, 1)                     # no parameters
    ctx, hp, lf, costs = _setup(gpu, oracle_c, "g3x3")
    with ctx:
        W, H = ctx.width, ctx.height
        for region in [(5, 5, 5, 9), (5, 5, 9, 5), (9, 5, 5, 9), (-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, W + 1, H), (0, 0, W, H + 1), (W, 0, W + 4, 4)]:
            _refused(ctx, *region)
        for steps in (-3, 0, 1, 257):
            _refused(ctx, 0, 0, W, H, steps=steps)
        res = L.abi.FocusCurveResult()
        assert ctx._lib.lfi_focus_curve(ctx._h, 0, 0, W, H, 32, None, None) == -1       # out == NULL
        assert ctx._lib.lfi_focus_curve(None, 0, 0, W, H, 32, None, res) == -1
        ctx.set_params(dataclasses.replace(hp, range=0.0))
        _refused(ctx, 0, 0, W, H)                       # range <= 0
        ctx.set_params(dataclasses.replace(hp, range=-0.25))
        _refused(ctx, 0, 0, W, H)
        ctx.set_params(dataclasses.replace(hp, focus_map_ids=np.zeros(0, np.int32)))
        _refused(ctx, 0, 0, W, H)                       # n_focus_ids == 0
        ctx.set_params(hp)
        _check(ctx, hp, costs, (0, 0, W, H))            # still usable, and right
        # out_cost may be NULL
        assert ctx._lib.lfi_focus_curve(ctx._h, 3, 4, 50, 9, 32, None, res) == 0
        want = ref.curve(costs[32], 3, 4, 50, 9)
        assert res.best_index == ref.first_min(want) and res.pixels == 47 * 5
        ctx.set_row_window(0, H // 2, 0, H)
        ctx.set_params(hp)
        _refused(ctx, 0, 0, W, H // 2)                  # a row window
    ctx, hp, lf, costs = _setup(gpu, oracle_c, "g3x3")
    with ctx:
        ctx.render("TEN_WM")
        ctx.release_inputs()
        _refused(ctx, 0, 0, 8, 8)                       # the RGBA planes are gone
        ctx.render("TEN_WM")
        ctx.sync()


@pytest.mark.parametrize("method,region", [("STD", "8,4,40,28"), ("TEN_WM", None)])
def test_cli_autofocus_renders_at_the_found_focus(gpu, tmp_path, method, region):
    cols, rows, W, H, seed, V = 4, 4, 64, 32, 7967, 4
    common = ["--synthetic", f"{cols},{rows},{W},{H},{seed}", "-t", "0,0,1,1", "-m", method, "-n", str(V), "-b", "1"]
    auto = ["--autofocus"] + ([region] if region else [])
    res = run_cli(gpu, *common, "-o", str(tmp_path / "auto"), "-f", "0.0", "-r", "1.0", *auto, "--autofocus-steps", "24")
    assert res.returncode == 0, res.stderr
    m = re.search(r"^autofocus: focus (\S+) \(candidate (\d+) of (\d+), (\d+) px\)$", res.stdout, re.M)
    assert m, res.stdout
    box = tuple(int(t) for t in region.split(",")) if region else (0, 0, W, H)
    with gpu.Context(0) as ctx:
        ctx.set_grid(cols, rows, W, H)
        ctx.fill_synthetic(seed)
        ctx.set_params(gpu.build_params(cols, rows, W, H, "0,0,1,1", 0.0, 1.0, 3.0, 1.0, V))
        cost, best, f = _curve(ctx, box, 24)
    assert np.float32(float(m.group(1))).view(np.uint32) == np.float32(f).view(np.uint32), (m.group(1), f)
    assert (int(m.group(2)), int(m.group(3)), int(m.group(4))) == (best, 24, (box[2] - box[0]) * (box[3] - box[1]))
    fixed = run_cli(gpu, *common, "-o", str(tmp_path / "fixed"), "-f", m.group(1))
    assert fixed.returncode == 0, fixed.stderr
    names = sorted(p.name for p in (tmp_path / "auto").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "fixed").iterdir()) == [f"{v:02d}.png" for v in range(V)]   # a fixed-focus render: no maps
    for name in names:
        assert (tmp_path / "auto" / name).read_bytes() == (tmp_path / "fixed" / name).read_bytes(), name
