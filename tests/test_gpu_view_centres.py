"""GPU (-m gpu): view-centred shifts (lfi_set_view_float_offsets, csrc/hip/blend_vfocus_af.hpp) — every view of an all-focus render shifted
about its own camera instead of the trajectory's centre.

View v of an all-focus render samples image g at (int)fma(f(x,y), O[v][g], pixel); the oracle's all-focus render of weight row v with O[v] as
its float offsets, over the map the context reads, is therefore the exact answer for view v: STD byte for byte, TEN_WM within the TEN_WM
contract (≤ 1 LSB from the fp16-accumulator model M16, < 1e-3 of the bytes off the exactly-summed model, every byte inside the interval of
the exact sum: tests/ten_interval.py).  Every render goes through tests/poison.py; the family's shapes and edges are the table of
tests/view_rows.py (tests/test_gpu_view_rows_coverage.py)."""
import os

import numpy as np
import pytest

import poison
from conftest import SEED
from view_rows import TEN_TOL_LSB, check_views, random_maps as _random_maps, run_cli, ten_want  # (_random_maps: test_gpu_view_maps.py imports it from here)

pytestmark = pytest.mark.gpu

KERNEL = {"STD": "blend_vfocus_af<STD>", "TEN_WM": "blend_vfocus_af<TEN_WM>"}


def _map_index(method, unified):
    return 1 if (method == "STD" or unified) else 0


def _want(oc, lf, O, hp, method, maps, unified=False, v0=0, v1=None, focused=None):
    """[v1 - v0] expected views: view v = the oracle's all-focus render of weight row v at float offsets O[v] over the map `method` reads."""
    v1 = len(O) if v1 is None else v1
    m = maps[_map_index(method, unified)]
    foc = hp.focused_offsets if focused is None else focused
    out = []
    for v in range(v0, v1):
        kw = dict(all_focus=True, map_plane=m, focus=hp.focus, rng=hp.range)
        if method == "STD":
            out.append(oc.blend_std(lf, foc, O[v], hp.weights[v:v + 1], **kw)[0])
        else:
            out.append(ten_want(oc, lf, foc, O[v], hp.weights[v:v + 1], **kw))
    return out


def _ctx(gpu, cols, rows, W, H, hp, layout="rgba", flags=0, seed=SEED):
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, W, H)
    ctx.fill_synthetic(seed)
    ctx.set_params(hp, flags)
    ctx.set_output_layout(layout)
    return ctx


def _maps(ctx, kind, H, W):
    if kind == "own":
        poison.focus_map(ctx)
        return [ctx.download_map(0), ctx.download_map(1)]
    maps = _random_maps(H, W, 11)
    for k in (0, 1):
        ctx.upload_map(k, maps[k])
    return maps


# name, cols, rows, W, H, trajectory, focus, range, views, aspect, effect — the shapes of test_gpu_view_focus.CASES
CASES = [
    ("long_8x8", 8, 8, 64, 48, "0,0,1,1", 0.0, 0.5, 64, 1.0, 3.0),
    ("diag_3x3_oddW", 3, 3, 33, 17, "0,0,1,1", 0.1, 0.8, 5, 1.783, 3.0),
    ("diag_15x15", 15, 15, 70, 20, "0.071,0.071,0.93,0.93", 0.22, 0.17, 9, 1.0, 3.0),
    ("single_1x1", 1, 1, 16, 16, "0,0,0,0", 0.0, 0.5, 1, 1.0, 3.0),
    ("wide_5x2_v70", 5, 2, 300, 7, "0,0,1,1", -0.4, 1.0, 70, 1.0, 3.0),
    ("subnormal_w_s7", 4, 4, 40, 24, "0.2,0.2,0.8,0.8", 0.3, 0.25, 11, 1.0, 7.0),
]


@pytest.mark.parametrize("unified", [False, True], ids=["default_map", "unified_map"])
@pytest.mark.parametrize("map_kind", ["own", "random"])
@pytest.mark.parametrize("layout", ["rgba", "planar"])
@pytest.mark.parametrize("method", ["STD", "TEN_WM"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_all_focus_per_view_matches_the_oracle(gpu, oracle_c, case, method, layout, map_kind, unified):
    name, cols, rows, W, H, traj, focus, rng_, V, aspect, effect = case
    hp = gpu.build_params(cols, rows, W, H, traj, focus, rng_, effect, aspect, V)
    O, _ = gpu.build_view_centred_offsets(cols, rows, W, H, traj, aspect, np.full(V, focus, np.float32))
    lf = oracle_c.synthetic_lf(cols * rows, W, H, SEED)
    ctx = _ctx(gpu, cols, rows, W, H, hp, layout, gpu.LFI_FLAG_UNIFIED_FOCUS_MAP if unified else 0)
    maps = _maps(ctx, map_kind, H, W)
    ctx.set_view_float_offsets(O)
    poison.render(ctx, method, all_focus=True)
    assert ctx.last_kernel_name() == KERNEL[method]
    check_views(ctx.download_views(), _want(oracle_c, lf, O, hp, method, maps, unified), method)
    ctx.close()


@pytest.mark.parametrize("layout", ["rgba", "planar"])
@pytest.mark.parametrize("method", ["STD", "TEN_WM"])
def test_rows_equal_to_the_offsets_give_the_ordinary_render(gpu, oracle_c, method, layout):
    cols, rows, W, H, V = 8, 8, 96, 40, 16
    hp = gpu.build_params(cols, rows, W, H, "0,0,1,1", 0.05, 0.4, 3.0, 1.783, V)
    lf = oracle_c.synthetic_lf(cols * rows, W, H, SEED)
    ctx = _ctx(gpu, cols, rows, W, H, hp, layout)
    maps = _maps(ctx, "own", H, W)
    poison.render(ctx, method, all_focus=True)
    plain_kernel = ctx.last_kernel_name()
    plain = ctx.download_views()
    O = np.repeat(hp.offsets[None], V, 0)
    ctx.set_view_float_offsets(O)
    poison.render(ctx, method, all_focus=True)
    assert ctx.last_kernel_name() == KERNEL[method]
    got = ctx.download_views()
    if method == "STD":
        assert (got == plain).all()
    else:
        assert np.abs(got.astype(int) - plain.astype(int)).max() <= TEN_TOL_LSB
        check_views(got, _want(oracle_c, lf, O, hp, method, maps), method)
    ctx.set_params(hp)  # clears the float offsets: the ordinary kernel is back
    poison.render(ctx, method, all_focus=True)
    assert ctx.last_kernel_name() == plain_kernel
    assert (ctx.download_views() == plain).all()
    ctx.set_view_float_offsets(O)
    ctx.set_view_float_offsets(None)  # NULL clears them too
    poison.render(ctx, method, all_focus=True)
    assert ctx.last_kernel_name() == plain_kernel
    assert (ctx.download_views() == plain).all()
    ctx.close()


@pytest.mark.parametrize("method", ["STD", "TEN_WM"])
def test_fixed_focus_rows_and_both_kinds_at_once(gpu, oracle_c, method):
    # -c without -r: the integer rows through lfi_set_view_offsets (here with a focus ramp, as -c -f … -F … sets them)
    cols, rows, W, H, V, traj = 5, 5, 61, 18, 13, "0,0,1,1"
    ramp = gpu.focus_ramp(0.1, 0.6, V)
    hp = gpu.build_params(cols, rows, W, H, traj, 0.1, 0.5, 3.0, 1.0, V)
    O, D = gpu.build_view_centred_offsets(cols, rows, W, H, traj, 1.0, ramp)
    lf = oracle_c.synthetic_lf(cols * rows, W, H, SEED)
    ctx = _ctx(gpu, cols, rows, W, H, hp)
    maps = _maps(ctx, "random", H, W)
    ctx.set_view_offsets(D)
    ctx.set_view_float_offsets(O)
    poison.render(ctx, method)  # fixed focus: the integer rows
    assert ctx.last_kernel_name() == f"blend_vfocus<{method}>"
    fixed = ctx.download_views()
    for v in range(V):
        if method == "STD":
            want = oracle_c.blend_std(lf, D[v], hp.offsets, hp.weights[v:v + 1])[0]
            assert (fixed[v] == want).all(), v
        else:
            want = oracle_c.blend_ten(lf, D[v], hp.offsets, hp.weights[v:v + 1], model=oracle_c.TEN_M16)[0]
            assert np.abs(fixed[v].astype(int) - want.astype(int)).max() <= TEN_TOL_LSB, v
    poison.render(ctx, method, all_focus=True)  # all-focus: the float rows
    assert ctx.last_kernel_name() == KERNEL[method]
    check_views(ctx.download_views(), _want(oracle_c, lf, O, hp, method, maps), method)
    ctx.close()


@pytest.mark.parametrize("layout", ["rgba", "planar"])
def test_sub_ranges_match_the_full_render(gpu, oracle_c, layout):
    cols, rows, W, H, V = 5, 5, 61, 18, 21
    hp = gpu.build_params(cols, rows, W, H, "0,0,1,1", 0.05, 0.4, 3.0, 1.0, V)
    O, _ = gpu.build_view_centred_offsets(cols, rows, W, H, "0,0,1,1", 1.0, np.full(V, 0.05, np.float32))
    ctx = _ctx(gpu, cols, rows, W, H, hp, layout)
    maps = _maps(ctx, "random", H, W)
    ctx.set_view_float_offsets(O)
    for method in ("STD", "TEN_WM"):
        poison.render(ctx, method, all_focus=True)
        full = ctx.download_views()
        lf = oracle_c.synthetic_lf(cols * rows, W, H, SEED)
        check_views(full, _want(oracle_c, lf, O, hp, method, maps), method)
        for v0, v1 in [(0, 1), (3, 12), (7, 8), (13, 21), (1, 20)]:
            got = poison.render_range(ctx, method, v0, v1, all_focus=True)
            assert (got == full[v0:v1]).all(), (method, v0, v1)
    ctx.close()


def test_new_offsets_do_not_reach_renders_already_enqueued(gpu, oracle_c):
    cols, rows, W, H, V = 8, 8, 256, 96, 8
    hp = gpu.build_params(cols, rows, W, H, "0,0,1,1", 0.0, 0.5, 3.0, 1.0, V)
    O1, _ = gpu.build_view_centred_offsets(cols, rows, W, H, "0,0,1,1", 1.0, np.zeros(V, np.float32))
    O2, _ = gpu.build_view_centred_offsets(cols, rows, W, H, "1,0,0,1", 1.0, np.zeros(V, np.float32))
    ctx = _ctx(gpu, cols, rows, W, H, hp)
    maps = _maps(ctx, "random", H, W)
    ctx.set_view_float_offsets(O1)
    ctx.poison(poison.RENDER, poison.POISON[0])
    ctx.render("STD", all_focus=True, v0=0, v1=4)
    ctx.set_view_float_offsets(O2)  # no synchronisation in between
    ctx.render("STD", all_focus=True, v0=4, v1=8)
    ctx.set_view_float_offsets(O1)  # reuses the first staging buffer while the second copy may be in flight
    ctx.render("STD", all_focus=True, v0=2, v1=3)
    ctx.sync()
    got = ctx.download_views()
    lf = oracle_c.synthetic_lf(cols * rows, W, H, SEED)
    check_views(got[:4], _want(oracle_c, lf, O1, hp, "STD", maps, v0=0, v1=4), "STD")
    check_views(got[4:], _want(oracle_c, lf, O2, hp, "STD", maps, v0=4, v1=8), "STD")
    ctx.close()


@pytest.mark.parametrize("method", ["STD", "TEN_WM"])
def test_row_bands_assemble_the_full_render(gpu, oracle_c, method):
    cols, rows, W, H, V, traj = 4, 4, 72, 50, 7, "0,0,1,1"
    hp = gpu.build_params(cols, rows, W, H, traj, 0.1, 0.4, 3.0, 1.0, V)
    O, _ = gpu.build_view_centred_offsets(cols, rows, W, H, traj, 1.0, np.full(V, 0.1, np.float32))
    lf = oracle_c.synthetic_lf(cols * rows, W, H, SEED)
    maps = _random_maps(H, W, 5)
    out = np.zeros((V, H, W, 4), np.uint8)
    for band in [(0, 23), (23, 50)]:
        in_rows = gpu.input_rows_all_focus(band, O.reshape(-1, 2), [], hp.focus, hp.range, hp.block_radius, H)
        ctx = gpu.Context(0)
        ctx.set_grid(cols, rows, W, H)
        ctx.set_row_window(band[0], band[1], *in_rows)
        ctx.upload_grid(lf)
        ctx.set_params(hp)
        for k in (0, 1):
            ctx.upload_map(k, maps[k])
        ctx.set_view_float_offsets(O)
        poison.render(ctx, method, all_focus=True)
        out[:, band[0]:band[1]] = ctx.download_views()[:, band[0]:band[1]]
        ctx.close()
    check_views(out, _want(oracle_c, lf, O, hp, method, maps), method)


def test_row_window_shortfall_is_refused(gpu):
    cols, rows, W, H, V = 3, 3, 40, 60, 4
    hp = gpu.build_params(cols, rows, W, H, "0.5,0.5,0.5,0.5", 0.0, 0.1, 3.0, 1.0, V)
    O, _ = gpu.build_view_centred_offsets(cols, rows, W, H, "0,0,1,1", 1.0, np.zeros(V, np.float32))
    band = (20, 40)
    in_rows = gpu.input_rows_all_focus(band, hp.offsets, [], hp.focus, hp.range, hp.block_radius, H)
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, W, H)
    ctx.set_row_window(band[0], band[1], *in_rows)  # enough for the centre's offsets, not for the outer cameras'
    ctx.fill_synthetic(SEED)
    ctx.set_params(hp)
    ctx.render("STD", all_focus=True)  # the ordinary render is covered
    ctx.set_view_float_offsets(O)
    with pytest.raises(gpu.LfiError, match="row window"):
        ctx.render("STD", all_focus=True)
    ctx.set_view_float_offsets(np.repeat(hp.offsets[None], V, 0))  # every view at the centre: covered
    ctx.render("STD", all_focus=True)
    ctx.sync()
    ctx.close()


@pytest.mark.parametrize("method", ["STD", "TEN_WM"])
def test_shifts_beyond_the_image_clamp(gpu, oracle_c, method):
    cols, rows, W, H, V = 3, 4, 37, 21, 10
    hp = gpu.build_params(cols, rows, W, H, "0,0,1,1", 0.5, 1.0, 3.0, 1.0, V)
    rng = np.random.default_rng(5)
    O = np.stack([rng.uniform(-3 * W, 3 * W, (V, cols * rows)), rng.uniform(-3 * H, 3 * H, (V, cols * rows))], -1).astype(np.float32)
    lf = oracle_c.synthetic_lf(cols * rows, W, H, SEED)
    ctx = _ctx(gpu, cols, rows, W, H, hp)
    maps = _maps(ctx, "random", H, W)
    ctx.set_view_float_offsets(O)
    poison.render(ctx, method, all_focus=True)
    check_views(ctx.download_views(), _want(oracle_c, lf, O, hp, method, maps), method)
    ctx.close()


def test_benchmark_prepare_quilt_and_compare(gpu, oracle_c):
    cols, rows, W, H, V = 4, 4, 48, 20, 6
    hp = gpu.build_params(cols, rows, W, H, "0,0,1,1", 0.0, 0.6, 3.0, 1.0, V)
    O, _ = gpu.build_view_centred_offsets(cols, rows, W, H, "0,0,1,1", 1.0, np.zeros(V, np.float32))
    lf = oracle_c.synthetic_lf(cols * rows, W, H, SEED)
    ctx = _ctx(gpu, cols, rows, W, H, hp)
    maps = _maps(ctx, "own", H, W)
    want = _want(oracle_c, lf, O, hp, "STD", maps)
    ctx.set_view_float_offsets(O)
    ctx.prepare("STD", all_focus=True)
    ctx.poison(poison.RENDER, poison.POISON[1])
    st = ctx.benchmark("STD", all_focus=True, warmup=1, runs=3)
    assert st.runs == 3 and st.mean_ms > 0 and ctx.last_kernel_name() == KERNEL["STD"]
    check_views(ctx.download_views(), want, "STD")
    quilt = ctx.download_quilt(3, 2)
    for t in range(6):
        ty, tx = divmod(t, 3)
        assert (quilt[ty * H:(ty + 1) * H, tx * W:(tx + 1) * W] == want[t]).all()
    q = ctx.compare_view(2, want[2])
    assert q.mse[0] == 0 and q.mse[1] == 0 and q.mse[2] == 0
    ctx.close()


def test_errors(gpu):
    cols, rows, W, H, V = 3, 3, 40, 30, 4
    hp = gpu.build_params(cols, rows, W, H, "0,0,1,1", 0.2, 0.2, 3.0, 1.0, V)
    O, D = gpu.build_view_centred_offsets(cols, rows, W, H, "0,0,1,1", 1.0, np.full(V, 0.2, np.float32))
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, W, H)
    ctx.fill_synthetic(SEED)
    with pytest.raises(gpu.LfiError, match="lfi_set_params"):
        ctx.set_view_float_offsets(O)
    ctx.set_params(hp)
    with pytest.raises(gpu.LfiError, match="differs"):
        ctx.set_view_float_offsets(O[:3])
    bad = O.copy()
    bad[1, 2, 0] = np.nan
    with pytest.raises(gpu.LfiError, match="finite"):
        ctx.set_view_float_offsets(bad)
    ctx.focus_map()
    # integer rows only: all-focus renders stay refused with the existing message
    ctx.set_view_offsets(D)
    with pytest.raises(gpu.LfiError, match="all-focus"):
        ctx.render("STD", all_focus=True)
    ctx.set_view_offsets(None)
    ctx.set_view_float_offsets(O)
    with pytest.raises(gpu.LfiError, match="lfi_render_stream"):
        ctx.render_stream("STD", hp.weights, all_focus=True)
    with pytest.raises(gpu.LfiError, match="prequant"):
        ctx.download_prequant("STD", 0, all_focus=True)
    ctx.render_stream("STD", hp.weights)  # fixed focus is not governed by the float rows
    ctx.set_params(hp, gpu.LFI_FLAG_TEN_ROUND_PER_BATCH)
    ctx.set_view_float_offsets(O)
    with pytest.raises(gpu.LfiError, match="ROUND_PER_BATCH"):
        ctx.render("TEN_WM", all_focus=True)
    ctx.set_params(hp)
    ctx.set_view_float_offsets(O)
    ctx.render("STD", all_focus=True)  # the context is still usable
    ctx.sync()
    assert ctx.last_kernel_name() == KERNEL["STD"]
    ctx.release_inputs()
    with pytest.raises(gpu.LfiError, match="released"):
        ctx.render("STD", all_focus=True)
    ctx.close()


@pytest.mark.parametrize("method", ["STD", "TEN_WM"])
def test_cli_view_centred_all_focus(gpu, oracle_c, tmp_path, method):
    from PIL import Image
    cols, rows, W, H, V, traj, f, r = 4, 4, 48, 20, 6, "0,0,1,1", 0.1, 0.3
    dst = tmp_path / "out"
    res = run_cli(gpu, "--synthetic", f"{cols},{rows},{W},{H}", "-t", traj, "-f", str(f), "-r", str(r), "-c", "-n", str(V), "-m", method,
               "-b", "2", "-o", str(dst))
    assert res.returncode == 0, res.stderr
    assert sorted(os.listdir(dst)) == [f"{i:02d}.png" for i in range(V)] + ["map0.png", "map1.png"]
    hp = gpu.build_params(cols, rows, W, H, traj, f, r, 3.0, 1.0, V)
    O, _ = gpu.build_view_centred_offsets(cols, rows, W, H, traj, 1.0, np.full(V, f, np.float32))
    lf = oracle_c.synthetic_lf(cols * rows, W, H, SEED)
    map0 = oracle_c.focus_estimate(lf, hp.offsets, hp.focus_map_ids, f, r, hp.block_radius)  # the map of the trajectory's centre
    map1 = oracle_c.focus_filter(map0, hp.block_radius)
    assert (np.array(Image.open(dst / "map0.png")) == map0).all()
    got = np.stack([np.array(Image.open(dst / f"{v:02d}.png")) for v in range(V)])
    check_views(got, _want(oracle_c, lf, O, hp, method, [map0, map1]), method)
    # without -c: the centre's offsets, which differ for the outer views
    plain = oracle_c.blend_std(lf, hp.focused_offsets, hp.offsets, hp.weights[:1], all_focus=True, map_plane=map1, focus=f, rng=r)[0]
    assert method != "STD" or not (got[0] == plain).all()


@pytest.mark.parametrize("method", ["STD", "TEN_WM"])
def test_cli_view_centred_focus_ramp(gpu, oracle_c, tmp_path, method):
    from PIL import Image
    cols, rows, W, H, V, traj = 4, 4, 48, 20, 8, "0,0,1,1"
    dst = tmp_path / "out"
    res = run_cli(gpu, "--synthetic", f"{cols},{rows},{W},{H}", "-t", traj, "-c", "-f", "0.1", "-F", "0.7", "-n", str(V), "-m", method, "-b", "2",
               "-o", str(dst))
    assert res.returncode == 0, res.stderr
    hp = gpu.build_params(cols, rows, W, H, traj, 0.1, 0.0, 3.0, 1.0, V)
    _, D = gpu.build_view_centred_offsets(cols, rows, W, H, traj, 1.0, gpu.focus_ramp(0.1, 0.7, V))
    lf = oracle_c.synthetic_lf(cols * rows, W, H, SEED)
    got = np.stack([np.array(Image.open(dst / f"{v:02d}.png")) for v in range(V)])
    for v in range(V):
        if method == "STD":
            assert (got[v] == oracle_c.blend_std(lf, D[v], hp.offsets, hp.weights[v:v + 1])[0]).all(), v
        else:
            want = oracle_c.blend_ten(lf, D[v], hp.offsets, hp.weights[v:v + 1], model=oracle_c.TEN_M16)[0]
            assert np.abs(got[v].astype(int) - want.astype(int)).max() <= TEN_TOL_LSB, v


def test_cli_view_centred_with_range_and_focus_end_fails(gpu, tmp_path):
    res = run_cli(gpu, "--synthetic", "3,3,32,8", "-t", "0,0,1,1", "-c", "-f", "0.1", "-F", "0.5", "-r", "0.2", "-m", "STD", "-o", str(tmp_path / "o"))
    assert res.returncode != 0 and "-F" in res.stderr and "-r" in res.stderr
