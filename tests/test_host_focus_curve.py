"""CPU: the host side of autofocus (lfi_focus_curve) — the numpy restatement of the focus curve (tests/focus_curve_ref.py) anchored to the
committed oracle, the candidate list of lfi_host_focus_candidates, the planted scene the GPU test uploads, the CLI's checks of --autofocus,
and the new kernels' code objects."""

import numpy as np
import pytest

import code_object
import focus_curve_ref as ref
from view_rows import run_cli

# name, cols, rows, W, H, trajectory, focus, range, seed — hash-noise light fields (oracle synthetic_lf).  Small images have block radius 1
# (width / 100 rounded up to even, at least 1); the last shape has 2.
ANCHOR_CASES = [
    ("g3x3_16x16", 3, 3, 16, 16, "0,0,1,1", 0.1, 0.3, 0x1F1F),
    ("g4x4_33x17", 4, 4, 33, 17, "0.071,0.071,0.93,0.93", 0.43, 0.25, 0x2B2B),
    ("g8x8_32x24", 8, 8, 32, 24, "0.0,0.0,1.0,1.0", -0.2, 0.5, 77),
    ("g3x3_208x104_r2", 3, 3, 208, 104, "0.2,0.1,0.9,0.8", 0.05, 0.2, 4242),
]


@pytest.mark.parametrize("case", ANCHOR_CASES, ids=[c[0] for c in ANCHOR_CASES])
def test_restatement_argmin_is_the_oracles_map_byte_for_every_pixel(native, oracle_c, case):
    """Every pixel as a 1 x 1 region, 32 steps: round((f_argmin - focus) / range * 255) is oracle_c.focus_estimate's map byte.  Every
    per-pixel cost is >= 1 on these inputs (asserted first), so the dropped FLT_MIN terms cannot be what makes the two agree."""
    _, cols, rows, W, H, traj, focus, rng, seed = case
    hp = native.build_params(cols, rows, W, H, traj, focus, rng, 3.0, 1.783, 2)
    if case[0].endswith("_r2"):
        assert tuple(hp.block_radius) == (2, 2)
    else:
        assert tuple(hp.block_radius) == (1, 1)
    lf = oracle_c.synthetic_lf(cols * rows, W, H, seed)
    costs = ref.pixel_costs(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, 32)
    assert costs.min() >= 1, int(costs.min())
    f = ref.candidates(hp.focus, hp.range, 32)
    got = ref.map_byte(f[np.argmin(costs, axis=0)], hp.focus, hp.range)   # np.argmin: the first minimum
    want = oracle_c.focus_estimate(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)
    assert (got == want[..., 0]).all(), int((got != want[..., 0]).sum())
    # a 1 x 1 region's curve is that pixel's column of costs
    assert (ref.curve(costs, 5, 3, 6, 4) == costs[:, 3, 5].astype(np.uint64)).all()


@pytest.mark.parametrize("steps", [2, 32, 255, 256])
@pytest.mark.parametrize("focus,rng", [(0.0, 1.0), (0.23, 0.17), (-0.75, 0.3), (1e-3, 2.5)])
def test_host_focus_candidates_are_fmaf_bit_for_bit(native, steps, focus, rng):
    got = native.focus_candidates(focus, rng, steps)
    assert got.dtype == np.float32 and got.shape == (steps,)
    step = np.float32(np.float32(rng) / np.float32(steps - 1))
    want = np.array([np.float32(np.float64(step) * np.float64(i) + np.float64(np.float32(focus))) for i in range(steps)], np.float32)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    assert (got.view(np.uint32) == ref.candidates(focus, rng, steps).view(np.uint32)).all()
    if steps == 32:
        # the estimate's own candidates (src/kernels.cu:245-250): step = range / 31
        assert step == np.float32(np.float32(rng) / np.float32(31))


def test_host_focus_candidates_refuse_fewer_than_two_steps(native):
    with pytest.raises(ValueError):
        native.focus_candidates(0.0, 1.0, 1)


@pytest.mark.parametrize("k", ref.PLANTED["ks"])
def test_planted_scene_has_its_strict_minimum_at_the_planted_candidate(native, k):
    P = ref.PLANTED
    hp = native.build_params(P["cols"], P["rows"], P["W"], P["H"], P["traj"], P["focus"], P["rng"], 3.0, 1.0, 2)
    assert (hp.offsets >= 0).all() and len(hp.focus_map_ids) == P["cols"] * P["rows"]
    lf = ref.planted_scene(hp.offsets, k, **P)
    costs = ref.pixel_costs(lf, hp.offsets, hp.focus_map_ids, P["focus"], P["rng"], hp.block_radius, P["steps"])
    for region in ref.PLANTED_REGIONS:
        cost = ref.curve(costs, *region)
        assert ref.first_min(cost) == k, (region, cost)
        assert (np.delete(cost, k) > cost[k]).all(), (region, cost)


AUTOFOCUS_ARGS = ["--synthetic", "4,4,32,16", "-t", "0,0,1,1", "-m", "STD", "-n", "4", "-b", "1", "-f", "0.0", "-r", "0.5", "--autofocus", "4,4,20,12"]


@pytest.mark.parametrize("extra", [["-F", "0.3"], ["-c"], ["-c", "--view-maps"]], ids=["-F", "-c", "--view-maps"])
def test_cli_refuses_autofocus_with_per_view_flags(native, tmp_path, extra):
    res = run_cli(native, *AUTOFOCUS_ARGS, "-o", str(tmp_path / "out"), *extra)
    assert res.returncode != 0
    assert "--autofocus" in res.stderr
    assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("r", [None, "0", "-0.5"])
def test_cli_refuses_autofocus_without_a_search_interval(native, tmp_path, r):
    args = list(AUTOFOCUS_ARGS)
    i = args.index("-r")
    args[i:i + 2] = [] if r is None else ["-r", r]
    res = run_cli(native, *args, "-o", str(tmp_path / "out"))
    assert res.returncode != 0
    assert "--autofocus" in res.stderr and "-r" in res.stderr
    assert not (tmp_path / "out").exists()


def test_cli_refuses_autofocus_steps_alone(native, tmp_path):
    args = [a for a in AUTOFOCUS_ARGS[:-2]] + ["--autofocus-steps", "16"]
    res = run_cli(native, *args, "-o", str(tmp_path / "out"))
    assert res.returncode != 0 and "--autofocus" in res.stderr


@pytest.mark.skipif(not code_object.have_tools(), reason="ROCm LLVM tools not installed")
def test_focus_curve_kernels_use_no_scratch_and_do_not_spill(native):
    """From the code object's metadata: the three kernels of csrc/hip/focus_curve.hpp exist, use no scratch and spill nothing; the partial-sum
    kernel keeps focus_estimate_packed<2, 4>'s five waves per SIMD (at most 96 registers per lane)."""
    kernels = code_object.kernels(native.build.HIP_LIB)
    curve = {k: v for k, v in kernels.items() if "focus_curve_" in k}
    assert sorted(k.split("focus_curve_")[1].split("I")[0].split("E")[0] for k in curve) == ["partial", "pick", "sum"], sorted(curve)
    for k, v in curve.items():
        assert v[".private_segment_fixed_size"] == 0 and v[".vgpr_spill_count"] == 0 and v[".sgpr_spill_count"] == 0, (k, v)
        if "partial" in k:
            assert v[".vgpr_count"] <= 96, (k, v)
