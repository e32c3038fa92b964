"""CPU: what fine focus tiles (lfi_focus_tiles_steps) need on the host — the interval of --auto-range at any number of tile candidates
(lfi_host_focus_auto_range_steps), the exported symbols, the planted scenes of the GPU test's pass-boundary cases on the numpy restatement,
the command line's checks of --tile-steps (made before any device is opened)."""
import ctypes as C

import numpy as np
import pytest

import focus_curve_ref as ref
from test_host_focus_tiles import TILE_ARGS
from view_rows import run_cli

STEPS = [32, 64, 96, 128, 256]


def _want(idx, focus, rng, steps):
    lo, hi = max(int(np.min(idx)) - 1, 0), min(int(np.max(idx)) + 1, steps - 1)
    cand = ref.candidates(focus, rng, steps)
    return cand[lo], np.float32(cand[hi] - cand[lo]), lo, hi


def _bits(v):
    return np.float32(v).view(np.uint32)


# ---- the interval ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("focus,rng", [(0.0, 0.5), (-0.75, 0.3), (0.23, 0.17), (1e-3, 2.5)])
@pytest.mark.parametrize("idx", [[9, 22], [0], [31], [0, 31], [17, 17, 17], [[1, 30], [30, 1]]], ids=lambda v: "i" + "_".join(str(x) for x in np.ravel(v)))
def test_at_32_steps_it_is_the_existing_function(native, idx, focus, rng):
    old = native.focus_auto_range(np.array(idx, np.int32), focus, rng)
    host = native.load_host_library()
    flat = np.ascontiguousarray(idx, np.int32).reshape(-1)
    f, r, lo_hi = C.c_float(), C.c_float(), np.zeros(2, np.int32)
    assert host.lfi_host_focus_auto_range_steps(flat.ctypes.data, len(flat), 32, focus, rng, C.byref(f), C.byref(r), lo_hi.ctypes.data) == 0
    assert (int(lo_hi[0]), int(lo_hi[1])) == old[2:]
    assert _bits(f.value) == _bits(old[0]) and _bits(r.value) == _bits(old[1])
    # and the Python default is that call
    assert native.focus_auto_range(np.array(idx, np.int32), focus, rng, steps=32)[2:] == old[2:]


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("focus,rng", [(0.0, 0.5), (-0.75, 0.3), (0.23, 0.17), (1e-3, 2.5)])
def test_interval_is_one_candidate_either_side_bit_equal_to_the_candidates(native, steps, focus, rng):
    last = steps - 1
    cand = native.focus_candidates(focus, rng, steps)
    assert (cand.view(np.uint32) == ref.candidates(focus, rng, steps).view(np.uint32)).all()
    for idx in ([0], [last], [0, last], [1, last - 1], [steps // 2], [last - 1, last], [steps // 3, steps // 2, last - 2], [[last, 5], [7, last]]):
        f, r, lo, hi = native.focus_auto_range(np.array(idx, np.int32), focus, rng, steps=steps)
        want = _want(idx, focus, rng, steps)
        assert (lo, hi) == want[2:], (idx, lo, hi)
        assert 0 <= lo <= int(np.min(idx)) and int(np.max(idx)) <= hi <= last      # clamped, and no tile's minimum is cut off
        assert _bits(f) == _bits(cand[lo]) and _bits(r) == _bits(np.float32(cand[hi] - cand[lo])), (idx, f, r)
        assert r > 0 and hi > lo


def test_hand_made_cases_clamp_at_either_end(native):
    assert native.focus_auto_range([0, 0], 0.0, 0.5, steps=128)[2:] == (0, 1)
    assert native.focus_auto_range([127], 0.0, 0.5, steps=128)[2:] == (126, 127)
    assert native.focus_auto_range([255], 0.0, 0.5, steps=256)[2:] == (254, 255)
    assert native.focus_auto_range([0, 255], 0.0, 0.5, steps=256)[2:] == (0, 255)
    assert native.focus_auto_range([36, 88], 0.0, 0.5, steps=128)[2:] == (35, 89)
    assert native.focus_auto_range([32], 0.0, 0.5, steps=64)[2:] == (31, 33)         # an index 32 steps could not have


@pytest.mark.parametrize("idx,steps,rng", [([], 64, 0.5), ([-1, 3], 64, 0.5), ([3, 64], 64, 0.5), ([3, 128], 128, 0.5), ([256], 256, 0.5), ([32], 32, 0.5),
                                           ([3], 64, 0.0), ([3], 64, -1.0),
                                           ([3], 0, 0.5), ([3], 31, 0.5), ([3], 33, 0.5), ([3], 48, 0.5), ([3], 288, 0.5), ([3], -32, 0.5), ([3], 2, 0.5)])
def test_refuses_indices_outside_the_steps_and_steps_the_tiles_do_not_take(native, idx, steps, rng):
    with pytest.raises(ValueError):
        native.focus_auto_range(np.array(idx, np.int32), 0.0, rng, steps=steps)
    host = native.load_host_library()
    flat = np.ascontiguousarray(idx, np.int32).reshape(-1)
    f, r, lo_hi = C.c_float(7.0), C.c_float(7.0), np.full(2, 7, np.int32)
    assert host.lfi_host_focus_auto_range_steps(flat.ctypes.data, len(flat), steps, 0.0, rng, C.byref(f), C.byref(r), lo_hi.ctypes.data) == -1
    assert f.value == 7.0 and r.value == 7.0 and (lo_hi == 7).all()                   # nothing written


# ---- symbols --------------------------------------------------------------------------------------------------------------------------

def test_libraries_export_the_new_entry_points(native):
    hip = native.load_hip_library()
    assert hasattr(hip, "lfi_focus_tiles_steps") and hasattr(hip, "lfi_focus_tiles_passes") and hasattr(hip, "lfi_focus_tiles")
    host = C.CDLL(native.build.HOST_LIB)
    assert hasattr(host, "lfi_host_focus_auto_range_steps") and hasattr(host, "lfi_host_focus_auto_range")
    assert "lfi_focus_tiles_steps" in native.ABI_SYMBOLS and "lfi_focus_tiles_passes" in native.ABI_SYMBOLS


# ---- the planted scenes beside a pass boundary ----------------------------------------------------------------------------------------
# focus_curve_ref.PLANTED over [0, 1.5] with 96 candidates.  Over PLANTED's own [0, 0.5] neighbouring candidates of 96 give every image the
# same integer shifts (the offsets are 0, 24, 48, 72: a step of 0.5 / 95 moves the largest by 0.38 pixels), and the first of such a run wins —
# 30 for a scene planted at 31, 61 for 63.  Over [0, 1.5] every candidate moves the images at 72 by more than a pixel: the planted candidate
# is the only one with cost 0 wherever no tap clamps.

BOUNDARY = dict(ref.PLANTED, rng=1.5, steps=96)
BOUNDARY_KS = (31, 32, 33, 63, 64)          # the last of pass 0, the first two of pass 1, the last of pass 1, the first of pass 2
BOUNDARY_GRID = (6, 8)                      # tiles of 16 x 8 pixels
BOUNDARY_TILES = [(1, 1), (2, 2), (0, 0)]   # two inside PLANTED_REGIONS[0], and the corner tile


def boundary_scene(native, k):
    P = BOUNDARY
    hp = native.build_params(P["cols"], P["rows"], P["W"], P["H"], P["traj"], P["focus"], P["rng"], 3.0, 1.0, 2)
    return hp, ref.planted_scene(hp.offsets, k, **P)


@pytest.mark.parametrize("k", BOUNDARY_KS)
def test_boundary_scenes_have_a_strict_minimum_at_the_planted_candidate(native, k):
    P = BOUNDARY
    hp, lf = boundary_scene(native, k)
    costs = ref.pixel_costs(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, P["steps"])
    for tx, ty in BOUNDARY_TILES:
        cost = ref.curve(costs, *native.focus_tile_rect(P["W"], P["H"], *BOUNDARY_GRID, tx, ty))
        assert ref.first_min(cost) == k, (tx, ty, cost)
        assert (np.delete(cost, k) > cost[k]).all(), (tx, ty, cost)


# ---- the command line -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra,words", [
    (["--tile-steps", "64"], ["--tile-steps", "--focus-tiles", "--auto-range"]),                       # neither of the two it needs
    (["--tile-steps", "64", "--autofocus"], ["--tile-steps", "--focus-tiles", "--auto-range"]),
    (["--focus-tiles", "4x2", "--tile-steps", "48"], ["--tile-steps", "32"]),
    (["--focus-tiles", "4x2", "--tile-steps", "0"], ["--tile-steps", "32"]),
    (["--auto-range", "--tile-steps", "288"], ["--tile-steps", "256"]),
    (["--auto-range", "4x2", "--tile-steps", "-32"], ["--tile-steps", "32"]),
], ids=["alone", "with_autofocus", "48", "0", "288", "neg"])
def test_cli_refuses_tile_steps_it_cannot_serve(native, tmp_path, extra, words):
    res = run_cli(native, *TILE_ARGS, "-r", "0.5", "-o", str(tmp_path / "out"), *extra)
    assert res.returncode != 0
    for w in words:
        assert w in res.stderr, res.stderr
    assert not (tmp_path / "out").exists()
