"""GPU (-m gpu): fine focus maps — lfi_set_focus_steps, lfi_focus_map with 64 … 256 candidates, and the CLI's --map-steps.

Every byte of map 0 is compared with the numpy restatement (tests/focus_steps_ref.py, anchored to the oracle at 32 steps by
tests/test_host_focus_steps.py), every byte of map 1 with oracle_c.focus_filter of it.  The shapes are 33 x 17, 16 x 16, 32 x 24 and 96 x 64;
a restatement is computed once per (scene, steps) and shared by the tests and variants that need it.  The maps and the estimate's workspace
(the carry plane included) are poisoned before every call a check reads, with alternating bytes."""
import dataclasses
import functools

import numpy as np
import pytest

import focus_curve_ref as cref
import focus_routes
import focus_steps_ref as ref
import lfinterpolator_amd as L
import poison
from test_host_focus_steps import FUZZ, fuzz_case, golden_case, has_negative_shifts, planted
from view_rows import run_cli

pytestmark = pytest.mark.gpu

VARIANTS = ["auto", "factored_direct", "packed_p2"]   # focus_range_t + focus_pick_sep where they apply / focus_range + focus_pick<2> / focus_estimate_packed
STEPS = [64, 96, 256]
SCENES = ["g4x4_33x17", "g15x15_16x16", "planted37", "planted93"] + [c[0] for c in FUZZ]


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(hp, lf) of a scene by name; cached: the arrays are shared and never written"""
    from oracle import lfi_oracle_c as oc
    if name == "g4x4_33x17":
        return golden_case(L, oc, "g4x4_33x17_v5", 0.25)                # odd width
    if name == "g15x15_16x16":
        return golden_case(L, oc, "g15x15_16x16_v8", 0.4)               # 32 of 225 sampled
    if name.startswith("planted"):
        return planted(L, int(name[7:]))
    if name == "flat":
        hp, lf = golden_case(L, oc, "g4x4_33x17_v5", 0.25)
        lf = np.empty_like(lf)
        lf[...] = (200, 100, 50, 255)
        return hp, lf
    return fuzz_case(L, oc, next(c for c in FUZZ if c[0] == name))


@functools.lru_cache(maxsize=None)
def _want(name, steps):
    """(map 0, map 1) of the restatement"""
    from oracle import lfi_oracle_c as oc
    hp, lf = _scene(name)
    m0 = ref.map0(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, steps)
    m0.setflags(write=False)
    m1 = oc.focus_filter(m0, hp.block_radius)
    m1.setflags(write=False)
    return m0, m1


def _ctx(gpu, name, variant="auto", steps=None, hp=None):
    hp0, lf = _scene(name)
    hp = hp0 if hp is None else hp
    n, H, W, _ = lf.shape
    cols, rows = _grid_of(name)
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, W, H)
    ctx.upload_grid(lf)
    ctx.set_params(hp)
    ctx.set_variant("FOCUS", variant)
    if steps is not None:
        ctx.set_focus_steps(steps)
    return ctx


def _grid_of(name):
    if name in ("g4x4_33x17", "flat") or name.startswith("planted"):
        return (4, 4)
    if name == "g15x15_16x16":
        return (15, 15)
    c = next(c for c in FUZZ if c[0] == name)
    return (c[1], c[2])


def _check(ctx, name, steps, what=""):
    poison.focus_map(ctx)
    want0, want1 = _want(name, steps)
    got0, got1 = ctx.download_map(0), ctx.download_map(1)
    assert (got0 == want0).all(), (name, steps, what, "map 0", int((got0 != want0).sum()))
    assert (got1 == want1).all(), (name, steps, what, "map 1", int((got1 != want1).sum()))
    return got0, got1


# ---- 1. maps against the restatement -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("name", SCENES)
def test_maps_equal_the_restatement_in_every_variant(gpu, name, steps):
    """the three implementations against the restatement, hence byte for byte against each other"""
    for variant in VARIANTS:
        with _ctx(gpu, name, variant, steps) as ctx:
            assert ctx.focus_steps() == steps
            _check(ctx, name, steps, variant)
            focus_routes.assert_variant(ctx, variant, _scene(name)[0], steps)   # the maps are the named estimate's


def test_the_scenes_cover_what_they_claim():
    hps = [_scene(c[0])[0] for c in FUZZ]
    assert sum(has_negative_shifts(hp) for hp in hps) >= 4
    rx = [int(hp.block_radius[0]) for hp in hps]
    assert any(r % 2 == 0 and r <= 64 for r in rx) and any(r % 2 == 1 for r in rx) and any(r > 64 for r in rx)


# ---- 2. pass boundaries and ties ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
def test_all_candidates_tie_and_the_first_wins_across_seven_boundaries(gpu, variant):
    with _ctx(gpu, "flat", variant, 256) as ctx:
        for _ in range(2):                  # both poison bytes: a constant map can equal one of them
            poison.focus_map(ctx)
            m0, m1 = ctx.download_map(0), ctx.download_map(1)
            assert (m0[..., :3] == 0).all() and (m0[..., 3] == 255).all()
            assert (m1[..., :3] == 0).all() and (m1[..., 3] == 255).all()


@pytest.mark.parametrize("k", [31, 32, 33, 63, 64])
def test_planted_scenes_beside_a_pass_boundary(gpu, k):
    name = f"planted{k}"
    want0, _ = _want(name, 128)
    hp, _ = _scene(name)
    f = cref.candidates(hp.focus, hp.range, 128)
    x0, y0, x1, y1 = cref.PLANTED_REGIONS[0]
    # the restatement itself puts the region's winners at or below k (tests/test_host_focus_steps.py explains which)
    assert (want0[y0:y1, x0:x1, 0] <= cref.map_byte(f[k], hp.focus, hp.range)).all()
    for variant in VARIANTS:
        with _ctx(gpu, name, variant, 128) as ctx:
            _check(ctx, name, 128, variant)


# ---- 3. steps = 32 is today -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["g4x4_33x17", "f3_4x4_96x64_r4x2"])
def test_back_at_32_steps_the_maps_are_the_oracles_and_a_fresh_contexts(gpu, oracle_c, name, variant):
    hp, lf = _scene(name)
    want0 = oracle_c.focus_estimate(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)
    want1 = oracle_c.focus_filter(want0, hp.block_radius)
    with _ctx(gpu, name, variant) as fresh:
        assert fresh.focus_steps() == 32
        poison.focus_map(fresh)
        fresh0, fresh1 = fresh.download_map(0), fresh.download_map(1)
    with _ctx(gpu, name, variant, 128) as ctx:
        _check(ctx, name, 128, variant)
        ctx.set_focus_steps(32)
        poison.focus_map(ctx)
        got0, got1 = ctx.download_map(0), ctx.download_map(1)
    assert (got0 == want0).all() and (got1 == want1).all()
    assert (got0 == fresh0).all() and (got1 == fresh1).all()


def test_the_setting_outlives_grid_params_and_row_window(gpu):
    hp, lf = _scene("g4x4_33x17")
    with _ctx(gpu, "g4x4_33x17", "auto", 96) as ctx:
        ctx.set_params(hp)
        assert ctx.focus_steps() == 96
        ctx.set_row_window(0, 8, 0, 17)
        assert ctx.focus_steps() == 96
        ctx.set_grid(4, 4, 33, 17)
        assert ctx.focus_steps() == 96


# ---- 4. the carry plane is initialised by the call ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["auto", "factored_direct"])
def test_poison_of_the_workspace_changes_nothing(gpu, variant):
    name = "f3_4x4_96x64_r4x2"
    maps = []
    with _ctx(gpu, name, variant, 128) as ctx:
        ctx.focus_map()     # the workspace exists: the poison below reaches the carry plane
        ctx.sync()
        assert ctx.memory_info().workspace_bytes >= 4 * 96 * 64
        for byte in (0x00, 0xFF):           # 0x00: every carried word smaller than any real one; 0xFF: larger
            ctx.poison(L.LFI_POISON_FOCUS_WORKSPACE | L.LFI_POISON_MAPS, byte)
            ctx.focus_map()
            ctx.sync()
            maps.append((ctx.download_map(0), ctx.download_map(1)))
    assert (maps[0][0] == maps[1][0]).all() and (maps[0][1] == maps[1][1]).all()
    want0, want1 = _want(name, 128)
    assert (maps[0][0] == want0).all() and (maps[0][1] == want1).all()


# ---- 5. row window --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("band", [(0, 20), (23, 47)])
def test_row_window_gives_the_whole_frames_rows(gpu, band):
    name = "f3_4x4_96x64_r4x2"
    hp, lf = _scene(name)
    want0, want1 = _want(name, 64)
    n, H, W, _ = lf.shape
    with gpu.Context(0) as ctx:
        ctx.set_grid(4, 4, W, H)
        ctx.set_row_window(band[0], band[1], 0, H)
        ctx.upload_grid(lf)
        ctx.set_params(hp)
        ctx.set_focus_steps(64)
        poison.focus_map(ctx)
        got0, got1 = ctx.download_map(0), ctx.download_map(1)
    assert (got0[band[0]:band[1]] == want0[band[0]:band[1]]).all()
    assert (got1[band[0]:band[1]] == want1[band[0]:band[1]]).all()


# ---- 6. the render consumes it --------------------------------------------------------------------------------------------------------------

def test_all_focus_renders_read_the_fine_map(gpu, oracle_c):
    name = "f3_4x4_96x64_r4x2"
    hp, lf = _scene(name)
    want0, want1 = _want(name, 128)
    with _ctx(gpu, name, "auto", 128) as ctx:
        _check(ctx, name, 128)
        poison.render(ctx, "STD", all_focus=True)
        std = ctx.download_views()
        poison.render(ctx, "TEN_WM", all_focus=True)
        ten = ctx.download_views()
    want_std = oracle_c.blend_std(lf, hp.focused_offsets, hp.offsets, hp.weights, all_focus=True, map_plane=want1, focus=hp.focus, rng=hp.range)
    assert (std == want_std).all(), int((std != want_std).sum())
    # the reference's Tensors::process reads map 0 (src/kernels.cu:430); within one LSB of the fp16-accumulate model, the existing contract
    want_ten = oracle_c.blend_ten(lf, hp.focused_offsets, hp.offsets, hp.weights, model=oracle_c.TEN_M16, all_focus=True, map_plane=want0,
                                  focus=hp.focus, rng=hp.range)
    assert np.abs(ten.astype(int) - want_ten.astype(int)).max() <= 1


# ---- 7. neighbours are untouched ------------------------------------------------------------------------------------------------------------

def test_tiles_and_view_maps_keep_32_candidates(gpu):
    name = "f1_8x8_32x24"
    c = next(c for c in FUZZ if c[0] == name)
    cols, rows, W, H, traj = c[1], c[2], c[3], c[4], c[5]
    hp, lf = _scene(name)
    V = 3
    O, _ = gpu.build_view_centred_offsets(cols, rows, W, H, traj, 1.783, np.full(V, hp.focus, np.float32))
    ids = gpu.build_view_focus_ids(cols, rows, traj, V)
    out = {}
    for steps in (32, 128):
        with _ctx(gpu, name, "auto", steps) as ctx:
            ctx.set_view_float_offsets(O)
            ctx.poison(poison.FOCUS, poison._byte(None))
            tiles = ctx.focus_tiles(4, 3)
            ctx.poison(L.LFI_POISON_VIEW_MAPS | L.LFI_POISON_FOCUS_WORKSPACE, poison._byte(None))
            ctx.view_focus_maps(ids)
            ctx.sync()
            out[steps] = (tiles, [ctx.download_view_map(v, k) for v in range(V) for k in (0, 1)])
    for a, b in zip(out[32][0], out[128][0]):
        assert (a.view(np.uint32) == b.view(np.uint32)).all() if a.dtype == np.float32 else (a == b).all()
    for a, b in zip(out[32][1], out[128][1]):
        assert (a == b).all()


def test_padded_planes_survive_a_change_of_steps_and_their_bookkeeping_stays_right(gpu, oracle_c):
    """as tests/test_gpu_parity.py::test_focus_map_padded_planes_are_kept_between_calls: the MAPS are poisoned, not the workspace — the padded
    planes are what is kept — and every call must give the right bytes: more candidates on the planes a 32-step call left, 32 candidates on
    the planes a fine call left, then one sampled image replaced (that plane alone is redone) at 32 and at 128."""
    name = "f3_4x4_96x64_r4x2"
    hp, lf = _scene(name)

    def check(ctx, steps, want0, what):
        ctx.set_focus_steps(steps)
        ctx.poison(L.LFI_POISON_MAPS, poison.POISON[len(what) & 1])
        ctx.focus_map()
        ctx.sync()
        got = ctx.download_map(0)
        assert (got == want0).all(), (what, int((got != want0).sum()))
        assert (ctx.download_map(1) == oracle_c.focus_filter(want0, hp.block_radius)).all(), what

    want32 = oracle_c.focus_estimate(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)
    with _ctx(gpu, name, "factored") as ctx:
        check(ctx, 32, want32, "first call")
        mem = ctx.memory_info().workspace_bytes
        check(ctx, 128, _want(name, 128)[0], "128 on the planes of 32")
        assert ctx.memory_info().workspace_bytes == mem      # nothing reallocated: the planes cannot have been rebuilt for that
        check(ctx, 32, want32, "32 on the planes of 128")
        check(ctx, 64, _want(name, 64)[0], "64")
        g = int(hp.focus_map_ids[1])
        lf2 = lf.copy()
        lf2[g] = lf[g][::-1, ::-1]
        ctx.upload_image(g, lf2[g])
        want32b = oracle_c.focus_estimate(lf2, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)
        assert not (want32b == want32).all()
        check(ctx, 32, want32b, "a sampled image replaced")
        want128b = ref.map0(lf2, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, 128)
        check(ctx, 128, want128b, "and 128 on those planes")
        assert ctx.memory_info().workspace_bytes == mem


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------------------

def test_bad_step_counts_are_refused_and_the_setting_is_kept(gpu):
    with _ctx(gpu, "g4x4_33x17", "auto", 96) as ctx:
        for bad in (0, 31, 33, 288, -32, 100, 16):
            with pytest.raises(L.LfiError, match=r"lfi error -1:.*lfi_set_focus_steps"):
                ctx.set_focus_steps(bad)
            assert ctx.focus_steps() == 96
        assert ctx._lib.lfi_set_focus_steps(None, 64) == -1 and ctx._lib.lfi_focus_steps(ctx._h, None) == -1
        _check(ctx, "g4x4_33x17", 96)            # still usable, and right


@pytest.mark.parametrize("variant", ["lds", "plain"])
def test_variants_of_32_candidates_refuse_other_numbers_and_leave_the_maps(gpu, oracle_c, variant):
    hp, lf = _scene("g4x4_33x17")
    with _ctx(gpu, "g4x4_33x17", variant, 64) as ctx:
        ctx.poison(L.LFI_POISON_MAPS, 0x77)
        with pytest.raises(L.LfiError, match=rf"lfi error -1:.*{variant}"):
            ctx.focus_map()
        ctx.sync()
        assert (ctx.download_map(0) == 0x77).all() and (ctx.download_map(1) == 0x77).all()
        ctx.set_focus_steps(32)
        poison.focus_map(ctx)
        assert (ctx.download_map(0) == oracle_c.focus_estimate(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)).all()


# ---- 9. the command line --------------------------------------------------------------------------------------------------------------------

def test_cli_map_steps_writes_the_librarys_map(gpu, tmp_path):
    cols, rows, W, H, V, seed = 4, 4, 96, 64, 4, 0x1F1F
    traj, focus, rng = "0.071,0.071,0.93,0.93", 0.1, 0.3
    res = run_cli(gpu, "--synthetic", f"{cols},{rows},{W},{H},{seed}", "-t", traj, "-m", "STD", "-n", str(V), "-b", "1", "-f", str(focus), "-r", str(rng),
                  "--map-steps", "128", "-o", str(tmp_path / "out"))
    assert res.returncode == 0, res.stderr
    maps = {}
    for steps in (32, 128):
        with gpu.Context(0) as ctx:
            ctx.set_grid(cols, rows, W, H)
            ctx.fill_synthetic(seed)
            ctx.set_params(gpu.build_params(cols, rows, W, H, traj, focus, rng, 3.0, 1.0, V))
            ctx.set_focus_steps(steps)
            poison.focus_map(ctx)
            maps[steps] = ctx.download_map(0)
    got = L.load_image(str(tmp_path / "out" / "map0.png"))
    assert (got[..., :3] == maps[128][..., :3]).all()
    assert not (maps[32] == maps[128]).all()         # the flag changed the map
    for extra in (["--map-steps", "100"], ["--map-steps", "64", "-c", "--view-maps"]):
        bad = run_cli(gpu, "--synthetic", f"{cols},{rows},{W},{H},{seed}", "-t", traj, "-m", "STD", "-n", str(V), "-b", "1", "-f", str(focus), "-r", str(rng),
                      *extra, "-o", str(tmp_path / "bad"))
        assert bad.returncode != 0 and "--map-steps" in bad.stderr
