"""GPU (-m gpu): per-view focus (lfi_set_view_offsets, csrc/hip/blend_vfocus.hpp) — focal stacks and focus pulls in one launch.

View v of a fixed-focus render samples image g at pixel + D[v][g]; the oracle's fixed-focus render of weight row v with D[v] as its
focused offsets is therefore the exact answer for view v: STD byte for byte, TEN_WM within the TEN_WM contract (≤ 1 LSB from the
fp16-accumulator model M16, < 1e-3 of the bytes off the exactly-summed model, every byte inside the interval of the exact sum:
tests/ten_interval.py).  Every render goes through tests/poison.py; the family's shapes, sources and edges are the table of
tests/view_rows.py (tests/test_gpu_view_rows_coverage.py)."""
import os

import numpy as np
import pytest

import poison
from conftest import SEED
from view_rows import check_views, run_cli, ten_want

pytestmark = pytest.mark.gpu


def _want(oc, lf, D, hp, method, v0=0, v1=None, weights=None):
    """[v1 - v0][H][W][4]: view v = the oracle's fixed-focus render of weight row v at offsets D[v]."""
    w = hp.weights if weights is None else weights
    v1 = len(D) if v1 is None else v1
    out = []
    for v in range(v0, v1):
        if method == "STD":
            out.append(oc.blend_std(lf, D[v], hp.offsets, w[v:v + 1])[0])
        else:
            out.append(ten_want(oc, lf, D[v], hp.offsets, w[v:v + 1]))
    return out


def _ctx(gpu, cols, rows, W, H, hp, D=None, layout="rgba", seed=SEED, flags=0):
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, W, H)
    ctx.fill_synthetic(seed)
    ctx.set_params(hp, flags)
    ctx.set_output_layout(layout)
    if D is not None:
        ctx.set_view_offsets(D)
    return ctx


# name, cols, rows, W, H, trajectory, focus from, focus to, views, aspect, effect
CASES = [
    ("stack_8x8", 8, 8, 64, 48, "0.5,0.5,0.5,0.5", 0.0, 0.5, 64, 1.0, 3.0),
    ("pull_3x3_oddW", 3, 3, 33, 17, "0,0,1,1", 0.1, 0.9, 5, 1.783, 3.0),
    ("pull_15x15", 15, 15, 70, 20, "0.071,0.071,0.93,0.93", 0.22, 0.39, 9, 1.0, 3.0),
    ("single_1x1", 1, 1, 16, 16, "0,0,0,0", 0.0, 0.5, 1, 1.0, 3.0),
    ("wide_5x2_v70", 5, 2, 300, 7, "0,0,1,1", -0.4, 0.6, 70, 1.0, 3.0),
    ("subnormal_w_s7", 4, 4, 40, 24, "0.2,0.2,0.8,0.8", 0.3, 0.0, 11, 1.0, 7.0),
]


@pytest.mark.parametrize("layout", ["rgba", "planar"])
@pytest.mark.parametrize("method", ["STD", "TEN_WM"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_focal_stacks_and_focus_pulls(gpu, oracle_c, case, method, layout):
    name, cols, rows, W, H, traj, f0, f1, V, aspect, effect = case
    focus = gpu.focus_ramp(f0, f1, V)
    hp = gpu.build_params(cols, rows, W, H, traj, float(focus[0]), 0.0, effect, aspect, V)
    D = gpu.build_view_offsets(cols, rows, W, H, traj, aspect, focus)
    lf = oracle_c.synthetic_lf(cols * rows, W, H, SEED)
    ctx = _ctx(gpu, cols, rows, W, H, hp, D, layout)
    poison.render(ctx, method)
    assert ctx.last_kernel_name() == f"blend_vfocus<{method}>"
    check_views(ctx.download_views(), _want(oracle_c, lf, D, hp, method), method)
    ctx.close()


@pytest.mark.parametrize("method", ["STD", "TEN_WM"])
def test_offsets_beyond_the_image_clamp(gpu, oracle_c, method):
    cols, rows, W, H, V = 3, 4, 37, 21, 10
    hp = gpu.build_params(cols, rows, W, H, "0,0,1,1", 0.2, 0.0, 3.0, 1.0, V)
    rng = np.random.default_rng(5)
    D = np.stack([rng.integers(-3 * W, 3 * W, cols * rows), rng.integers(-3 * H, 3 * H, cols * rows)], -1)[None].repeat(V, 0).astype(np.int32)
    D[1:] = rng.integers(-2 * W, 2 * W, D[1:].shape)
    D[2, 0] = (2 ** 31 - 1, -2 ** 31)  # far beyond: the same samples as ±W / ±H
    lf = oracle_c.synthetic_lf(cols * rows, W, H, SEED)
    ctx = _ctx(gpu, cols, rows, W, H, hp, D)
    poison.render(ctx, method)
    want_D = D.copy()
    want_D[..., 0] = np.clip(want_D[..., 0], -W, W)
    want_D[..., 1] = np.clip(want_D[..., 1], -H, H)
    check_views(ctx.download_views(), _want(oracle_c, lf, want_D, hp, method), method)
    ctx.close()


def test_weights_outside_0_2(gpu, oracle_c):
    cols, rows, W, H, V = 3, 3, 50, 13, 6
    hp = gpu.build_params(cols, rows, W, H, "0,0,1,1", 0.0, 0.0, 3.0, 1.0, V)
    rng = np.random.default_rng(9)
    w = rng.uniform(-0.6, 0.6, (V, cols * rows)).astype(np.float16)
    w[:, 4] = np.float16(2.25)
    hp.weights = w.view(np.uint16)
    D = gpu.build_view_offsets(cols, rows, W, H, "0,0,1,1", 1.0, gpu.focus_ramp(-0.5, 0.5, V))
    lf = oracle_c.synthetic_lf(cols * rows, W, H, SEED)
    ctx = _ctx(gpu, cols, rows, W, H, hp, D)
    poison.render(ctx, "STD")
    check_views(ctx.download_views(), _want(oracle_c, lf, D, hp, "STD"), "STD")
    # TEN_WM: one fp16 rounding of the fp32 sum, truncated — within one LSB of the exactly-summed model (M16 re-rounds per batch of 16
    # images, which for sums above 256 is not the contract of any fp32-accumulating kernel here)
    poison.render(ctx, "TEN_WM")
    got = ctx.download_views()
    exact = np.stack([oracle_c.blend_ten(lf, D[v], hp.offsets, hp.weights[v:v + 1], model=oracle_c.TEN_EXACT)[0] for v in range(V)])
    assert np.abs(got.astype(int) - exact.astype(int)).max() <= 1 and (got != exact).mean() < 1e-3
    ctx.close()


@pytest.mark.parametrize("method", ["STD", "TEN_WM"])
def test_rgba_source_through_grid_device_ptr(gpu, oracle_c, method):
    cols, rows, W, H, V = 4, 3, 45, 19, 9
    focus = gpu.focus_ramp(0.0, 0.8, V)
    hp = gpu.build_params(cols, rows, W, H, "0,0,1,1", 0.0, 0.0, 3.0, 1.0, V)
    D = gpu.build_view_offsets(cols, rows, W, H, "0,0,1,1", 1.0, focus)
    lf = oracle_c.synthetic_lf(cols * rows, W, H, SEED)
    ctx = _ctx(gpu, cols, rows, W, H, hp, D)
    ctx.grid_device_ptr()  # handed out and not marked modified: the RGBA planes are read directly
    poison.render(ctx, method)
    assert ctx.last_kernel_name() == f"blend_vfocus<{method},rgba_src>"
    want = _want(oracle_c, lf, D, hp, method)
    check_views(ctx.download_views(), want, method)
    ctx.grid_modified()
    poison.render(ctx, method)
    assert ctx.last_kernel_name() == f"blend_vfocus<{method}>"
    check_views(ctx.download_views(), want, method)
    ctx.close()


@pytest.mark.parametrize("layout", ["rgba", "planar"])
def test_sub_ranges_match_the_full_render(gpu, oracle_c, layout):
    cols, rows, W, H, V = 5, 5, 61, 18, 21
    focus = gpu.focus_ramp(0.05, 0.45, V)
    hp = gpu.build_params(cols, rows, W, H, "0.5,0.5,0.5,0.5", 0.05, 0.0, 3.0, 1.0, V)
    D = gpu.build_view_offsets(cols, rows, W, H, "0.5,0.5,0.5,0.5", 1.0, focus)
    ctx = _ctx(gpu, cols, rows, W, H, hp, D, layout)
    poison.render(ctx, "STD")
    full = ctx.download_views()
    lf = oracle_c.synthetic_lf(cols * rows, W, H, SEED)
    check_views(full, _want(oracle_c, lf, D, hp, "STD"), "STD")
    for v0, v1 in [(0, 1), (3, 12), (7, 8), (13, 21), (1, 20)]:
        got = poison.render_range(ctx, "STD", v0, v1)
        assert (got == full[v0:v1]).all(), (v0, v1)
    ctx.close()


def test_new_offsets_do_not_reach_renders_already_enqueued(gpu, oracle_c):
    cols, rows, W, H, V = 8, 8, 256, 96, 8
    hp = gpu.build_params(cols, rows, W, H, "0.5,0.5,0.5,0.5", 0.0, 0.0, 3.0, 1.0, V)
    D1 = gpu.build_view_offsets(cols, rows, W, H, "0.5,0.5,0.5,0.5", 1.0, gpu.focus_ramp(0.0, 0.5, V))
    D2 = gpu.build_view_offsets(cols, rows, W, H, "0.5,0.5,0.5,0.5", 1.0, gpu.focus_ramp(0.9, 0.2, V))
    ctx = _ctx(gpu, cols, rows, W, H, hp, D1)
    ctx.poison(poison.RENDER, poison.POISON[0])
    ctx.render("STD", v0=0, v1=4)
    ctx.set_view_offsets(D2)  # no synchronisation in between
    ctx.render("STD", v0=4, v1=8)
    ctx.sync()
    got = ctx.download_views()
    lf = oracle_c.synthetic_lf(cols * rows, W, H, SEED)
    check_views(got[:4], _want(oracle_c, lf, D1, hp, "STD", 0, 4), "STD")
    check_views(got[4:], _want(oracle_c, lf, D2, hp, "STD", 4, 8), "STD")
    ctx.close()


@pytest.mark.parametrize("layout", ["rgba", "planar"])
def test_rows_equal_to_focused_offsets_give_the_plain_render(gpu, layout):
    cols, rows, W, H, V = 8, 8, 96, 40, 16
    hp = gpu.build_params(cols, rows, W, H, "0,0,1,1", 0.23, 0.0, 3.0, 1.783, V)
    ctx = _ctx(gpu, cols, rows, W, H, hp, layout=layout)
    poison.render(ctx, "STD")
    plain_kernel = ctx.last_kernel_name()
    plain = ctx.download_views()
    ctx.set_view_offsets(np.repeat(hp.focused_offsets[None], V, 0))
    poison.render(ctx, "STD")
    assert ctx.last_kernel_name() == "blend_vfocus<STD>"
    assert (ctx.download_views() == plain).all()
    ctx.set_params(hp)  # clears the per-view offsets: the ordinary render is back
    poison.render(ctx, "STD")
    assert ctx.last_kernel_name() == plain_kernel
    assert (ctx.download_views() == plain).all()
    # NULL clears them too
    ctx.set_view_offsets(np.repeat(hp.focused_offsets[None], V, 0))
    ctx.set_view_offsets(None)
    poison.render(ctx, "STD")
    assert ctx.last_kernel_name() == plain_kernel
    ctx.close()


def test_benchmark_prepare_quilt_and_compare(gpu, oracle_c):
    cols, rows, W, H, V = 4, 4, 48, 20, 6
    focus = gpu.focus_ramp(0.0, 0.6, V)
    hp = gpu.build_params(cols, rows, W, H, "0.5,0.5,0.5,0.5", 0.0, 0.0, 3.0, 1.0, V)
    D = gpu.build_view_offsets(cols, rows, W, H, "0.5,0.5,0.5,0.5", 1.0, focus)
    lf = oracle_c.synthetic_lf(cols * rows, W, H, SEED)
    want = _want(oracle_c, lf, D, hp, "STD")
    ctx = _ctx(gpu, cols, rows, W, H, hp, D)
    ctx.prepare("STD")
    ctx.poison(poison.RENDER, poison.POISON[1])
    st = ctx.benchmark("STD", warmup=1, runs=3)
    assert st.runs == 3 and st.mean_ms > 0 and ctx.last_kernel_name() == "blend_vfocus<STD>"
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
    hp = gpu.build_params(cols, rows, W, H, "0,0,1,1", 0.2, 0.2, 3.0, 1.0, V)  # a focus range: the focus map exists
    D = gpu.build_view_offsets(cols, rows, W, H, "0,0,1,1", 1.0, gpu.focus_ramp(0.0, 0.4, V))
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, W, H)
    ctx.fill_synthetic(SEED)
    with pytest.raises(gpu.LfiError, match="lfi_set_params"):
        ctx.set_view_offsets(D)
    ctx.set_params(hp)
    with pytest.raises(gpu.LfiError, match="differs"):
        ctx.set_view_offsets(D[:3])
    ctx.set_view_offsets(D)
    ctx.focus_map()
    with pytest.raises(gpu.LfiError, match="all-focus"):
        ctx.render("STD", all_focus=True)
    with pytest.raises(gpu.LfiError, match="lfi_render_stream"):
        ctx.render_stream("STD", hp.weights)
    with pytest.raises(gpu.LfiError, match="prequant"):
        ctx.download_prequant("STD", 0)
    ctx.set_params(hp, gpu.LFI_FLAG_TEN_ROUND_PER_BATCH)
    ctx.set_view_offsets(D)
    with pytest.raises(gpu.LfiError, match="ROUND_PER_BATCH"):
        ctx.render("TEN_WM")
    ctx.set_params(hp)
    ctx.set_view_offsets(D)
    ctx.render("STD")  # the context is still usable
    ctx.sync()
    ctx.close()


def test_row_window_shortfall_is_refused(gpu):
    cols, rows, W, H, V = 3, 3, 40, 60, 4
    hp = gpu.build_params(cols, rows, W, H, "0,0,1,1", 0.0, 0.0, 3.0, 1.0, V)
    D = gpu.build_view_offsets(cols, rows, W, H, "0,0,1,1", 1.0, gpu.focus_ramp(0.0, 1.0, V))
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, W, H)
    ctx.set_row_window(20, 40, 20, 40)  # focus 0 needs these rows only; focus 1 reaches ±20 rows further
    ctx.fill_synthetic(SEED)
    ctx.set_params(hp)
    with pytest.raises(gpu.LfiError, match="row window"):
        ctx.set_view_offsets(D)
    ctx.set_view_offsets(D[:1].repeat(V, 0))  # every view at focus 0: covered
    ctx.close()


@pytest.mark.parametrize("method", ["STD", "TEN_WM"])
def test_row_bands_assemble_the_full_render(gpu, oracle_c, method):
    cols, rows, W, H, V = 4, 4, 72, 50, 7
    traj = "0,0,1,1"
    focus = gpu.focus_ramp(0.0, 0.5, V)
    hp = gpu.build_params(cols, rows, W, H, traj, 0.0, 0.0, 3.0, 1.0, V)
    D = gpu.build_view_offsets(cols, rows, W, H, traj, 1.0, focus)
    lf = oracle_c.synthetic_lf(cols * rows, W, H, SEED)
    out = np.zeros((V, H, W, 4), np.uint8)
    for band in [(0, 23), (23, 50)]:
        in_rows = gpu.input_rows(band, D.reshape(-1, 2), H)
        ctx = gpu.Context(0)
        ctx.set_grid(cols, rows, W, H)
        ctx.set_row_window(band[0], band[1], *in_rows)
        ctx.upload_grid(lf)
        ctx.set_params(hp)
        ctx.set_view_offsets(D)
        poison.render(ctx, method)
        out[:, band[0]:band[1]] = ctx.download_views()[:, band[0]:band[1]]
        ctx.close()
    check_views(out, _want(oracle_c, lf, D, hp, method), method)


def test_released_inputs(gpu, oracle_c):
    cols, rows, W, H, V = 4, 4, 64, 32, 8
    traj = "0.5,0.5,0.5,0.5"
    hp = gpu.build_params(cols, rows, W, H, traj, 0.5, 0.0, 3.0, 1.0, V)
    lf = oracle_c.synthetic_lf(cols * rows, W, H, SEED)
    ctx = _ctx(gpu, cols, rows, W, H, hp)
    ctx.release_inputs()  # the planar copy is padded for the offsets of focus 0.5
    D = gpu.build_view_offsets(cols, rows, W, H, traj, 1.0, gpu.focus_ramp(0.0, 0.5, V))
    ctx.set_view_offsets(D)  # covered: every |shift| within focus 0.5's
    poison.render(ctx, "STD")
    assert ctx.last_kernel_name() == "blend_vfocus<STD>"
    check_views(ctx.download_views(), _want(oracle_c, lf, D, hp, "STD"), "STD")
    far = gpu.build_view_offsets(cols, rows, W, H, traj, 1.0, gpu.focus_ramp(0.0, 3.0, V))
    ctx.set_view_offsets(far)  # shifts of focus 3: beyond the copy's padding, and the RGBA planes are gone
    with pytest.raises(gpu.LfiError, match="released"):
        ctx.render("STD")
    ctx.close()


@pytest.mark.parametrize("method", ["STD", "TEN_WM"])
def test_cli_focal_stack(gpu, oracle_c, tmp_path, method):
    from PIL import Image
    cols, rows, W, H, V = 4, 4, 48, 20, 12
    traj = "0.5,0.5,0.5,0.5"
    dst = tmp_path / "out"
    res = run_cli(gpu, "--synthetic", f"{cols},{rows},{W},{H}", "-t", traj, "-f", "0", "-F", "0.6", "-n", str(V), "-m", method, "-b", "2",
               "-o", str(dst))
    assert res.returncode == 0, res.stderr
    assert sorted(os.listdir(dst)) == [f"{i:02d}.png" for i in range(V)]
    hp = gpu.build_params(cols, rows, W, H, traj, 0.0, 0.0, 3.0, 1.0, V)
    D = gpu.build_view_offsets(cols, rows, W, H, traj, 1.0, gpu.focus_ramp(0.0, 0.6, V))
    lf = oracle_c.synthetic_lf(cols * rows, W, H, SEED)
    got = np.stack([np.array(Image.open(dst / f"{v:02d}.png")) for v in range(V)])
    check_views(got, _want(oracle_c, lf, D, hp, method), method)


def test_cli_focus_end_with_range_fails(gpu, tmp_path):
    res = run_cli(gpu, "--synthetic", "3,3,32,8", "-t", "0,0,1,1", "-f", "0.1", "-F", "0.5", "-r", "0.2", "-m", "STD", "-o", str(tmp_path / "o"))
    assert res.returncode != 0 and "-F" in res.stderr and "-r" in res.stderr
