"""CPU: the host side of focus tiles (lfi_focus_tiles) — the tile rule of lfi_host_focus_tile_rect, the interval arithmetic of
lfi_host_focus_auto_range (--auto-range), the exported symbols, the two-depth planted scene the GPU test uploads, the CLI's checks of
--focus-tiles / --auto-range, and the new kernel's code object."""
import ctypes as C

import numpy as np
import pytest

import code_object
import focus_curve_ref as ref
from view_rows import run_cli


# ---- the tile rule --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H,nx,ny", [(96, 64, 7, 5), (96, 64, 96, 1), (96, 64, 1, 64), (96, 64, 96, 64), (203, 29, 16, 9), (1920, 1080, 16, 9),
                                       (3840, 2160, 256, 256), (131, 33, 3, 2), (5, 3, 5, 3), (1, 1, 1, 1)])
def test_tiles_cover_the_frame_exactly_once(native, W, H, nx, ny):
    seen = np.zeros((H, W), np.int32)
    widths, heights = set(), set()
    for ty in range(ny):
        for tx in range(nx):
            x0, y0, x1, y1 = native.focus_tile_rect(W, H, nx, ny, tx, ty)
            assert (x0, x1) == (tx * W // nx, (tx + 1) * W // nx) and (y0, y1) == (ty * H // ny, (ty + 1) * H // ny)
            assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H     # no tile is empty
            seen[y0:y1, x0:x1] += 1
            widths.add(x1 - x0), heights.add(y1 - y0)
    assert (seen == 1).all()
    assert max(widths) - min(widths) <= 1 and max(heights) - min(heights) <= 1


def test_tile_rule_uses_64_bit_products(native):
    # tx * W overflows 32 bits: 65535 * 65536
    assert native.focus_tile_rect(65536, 4, 65536, 1, 65535, 0) == (65535, 0, 65536, 4)
    assert native.focus_tile_rect(2 ** 31 - 1, 2, 2 ** 16, 2, 2 ** 16 - 1, 1) == ((2 ** 16 - 1) * (2 ** 31 - 1) // 2 ** 16, 1, 2 ** 31 - 1, 2)


@pytest.mark.parametrize("args", [(96, 64, 0, 1, 0, 0), (96, 64, 1, 0, 0, 0), (96, 64, 97, 1, 0, 0), (96, 64, 1, 65, 0, 0), (96, 64, 4, 4, 4, 0),
                                  (96, 64, 4, 4, 0, 4), (96, 64, 4, 4, -1, 0), (96, 64, 4, 4, 0, -1)])
def test_tile_rule_refuses_what_is_not_a_tile(native, args):
    with pytest.raises(ValueError):
        native.focus_tile_rect(*args)


# ---- the interval of --auto-range -----------------------------------------------------------------------------------------------------

def _auto_range_want(idx, focus, rng):
    lo, hi = max(int(np.min(idx)) - 1, 0), min(int(np.max(idx)) + 1, 31)
    cand = ref.candidates(focus, rng, 32)
    return cand[lo], np.float32(cand[hi] - cand[lo]), lo, hi


@pytest.mark.parametrize("focus,rng", [(0.0, 0.5), (-0.75, 0.3), (0.23, 0.17), (1e-3, 2.5)])
@pytest.mark.parametrize("idx", [[9, 22], [[9, 9, 15, 22]], [0, 12], [0], [31], [5, 31], [0, 31], [17], [17, 17, 17], [[1, 30], [30, 1]], [30, 31, 30]],
                         ids=lambda v: "i" + "_".join(str(x) for x in np.ravel(v)))
def test_auto_range_is_one_candidate_either_side_of_the_tiles_minima(native, idx, focus, rng):
    f, r, lo, hi = native.focus_auto_range(np.array(idx, np.int32), focus, rng)
    want = _auto_range_want(idx, focus, rng)
    assert (lo, hi) == want[2:]
    assert np.float32(f).view(np.uint32) == want[0].view(np.uint32) and np.float32(r).view(np.uint32) == want[1].view(np.uint32)
    assert r > 0 and hi > lo                                  # also for lo == hi, at either end of the interval
    assert lo <= int(np.min(idx)) and hi >= int(np.max(idx))  # no tile's minimum is cut off


def test_auto_range_of_hand_made_cases(native):
    assert native.focus_auto_range([9, 22], 0.0, 0.5)[2:] == (8, 23)
    assert native.focus_auto_range([0, 0, 0], 0.0, 0.5)[2:] == (0, 1)
    assert native.focus_auto_range([31], 0.0, 0.5)[2:] == (30, 31)
    assert native.focus_auto_range([0, 31], 0.0, 0.5)[2:] == (0, 31)
    f, r, lo, hi = native.focus_auto_range([0, 31], 0.25, 0.5)
    assert f == np.float32(0.25) and r == np.float32(ref.candidates(0.25, 0.5, 32)[31] - np.float32(0.25))
    assert native.focus_auto_range([16], 0.0, 0.5)[2:] == (15, 17)


@pytest.mark.parametrize("idx,rng", [([], 0.5), ([-1, 3], 0.5), ([3, 32], 0.5), ([3], 0.0), ([3], -1.0)])
def test_auto_range_refuses_bad_input(native, idx, rng):
    with pytest.raises(ValueError):
        native.focus_auto_range(np.array(idx, np.int32), 0.0, rng)


# ---- symbols --------------------------------------------------------------------------------------------------------------------------

def test_libraries_export_the_new_entry_points(native):
    hip = native.load_hip_library()
    assert hasattr(hip, "lfi_focus_tiles")
    host = C.CDLL(native.build.HOST_LIB)
    assert hasattr(host, "lfi_host_focus_tile_rect") and hasattr(host, "lfi_host_focus_auto_range")
    assert "lfi_focus_tiles" in native.ABI_SYMBOLS


# ---- the two-depth planted scene ------------------------------------------------------------------------------------------------------

def two_depth_scene(native):
    """left half ref.planted_scene(k = 9), right half k = 22 (one random texture, shown at two depths): (hp, lf)"""
    P = ref.PLANTED
    hp = native.build_params(P["cols"], P["rows"], P["W"], P["H"], P["traj"], P["focus"], P["rng"], 3.0, 1.0, 2)
    near, far = (ref.planted_scene(hp.offsets, k, **P) for k in P["ks"])
    lf = near.copy()
    lf[:, :, P["W"] // 2:] = far[:, :, P["W"] // 2:]
    return hp, lf


def test_two_depth_scene_has_its_minima_at_9_and_22_in_the_outer_tiles(native):
    """4 x 1 tiles of the 96 x 64 two-depth scene on the numpy restatement: the first strict minimum is candidate 9 in the leftmost tile and 22
    in the rightmost — what --focus-tiles 4x1 has to print and what gives --auto-range 4x1 the candidates 8..23."""
    P = ref.PLANTED
    hp, lf = two_depth_scene(native)
    costs = ref.pixel_costs(lf, hp.offsets, hp.focus_map_ids, P["focus"], P["rng"], hp.block_radius, P["steps"])
    best = []
    for tx in range(4):
        cost = ref.curve(costs, *native.focus_tile_rect(P["W"], P["H"], 4, 1, tx, 0))
        best.append(ref.first_min(cost))
        if tx in (0, 3):
            assert (np.delete(cost, best[-1]) > cost[best[-1]]).all(), (tx, cost)   # strict
    assert best[0] == 9 and best[3] == 22, best
    assert 9 <= min(best) and max(best) <= 22, best       # the inner tiles lie between: the interval is 8..23
    assert native.focus_auto_range(best, P["focus"], P["rng"])[2:] == (8, 23)


# ---- the command line -----------------------------------------------------------------------------------------------------------------

TILE_ARGS = ["--synthetic", "4,4,32,16", "-t", "0,0,1,1", "-m", "STD", "-n", "4", "-b", "1", "-f", "0.0"]


@pytest.mark.parametrize("flag", [["--focus-tiles", "4x2"], ["--auto-range"], ["--auto-range", "4x2"]], ids=["tiles", "auto", "auto_grid"])
@pytest.mark.parametrize("r", [None, "0", "-0.5"])
def test_cli_refuses_tiles_without_a_search_interval(native, tmp_path, flag, r):
    res = run_cli(native, *TILE_ARGS, *([] if r is None else ["-r", r]), "-o", str(tmp_path / "out"), *flag)
    assert res.returncode != 0
    assert flag[0] in res.stderr and "-r" in res.stderr
    assert not (tmp_path / "out").exists()


def test_cli_refuses_auto_range_with_autofocus(native, tmp_path):
    res = run_cli(native, *TILE_ARGS, "-r", "0.5", "-o", str(tmp_path / "out"), "--auto-range", "--autofocus")
    assert res.returncode != 0
    assert "--auto-range" in res.stderr and "--autofocus" in res.stderr
    assert not (tmp_path / "out").exists()


# ---- the code object ------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not code_object.have_tools(), reason="ROCm LLVM tools not installed")
def test_focus_tile_costs_uses_no_scratch_and_keeps_eight_waves_per_simd(native):
    """From the code object's metadata: both instantiations of focus_tile_costs (csrc/hip/focus_tiles.hpp) exist, use no scratch, spill nothing
    and stay at or below 64 registers per lane (eight waves per SIMD; its 32 KiB of LDS per workgroup allow five workgroups per CU)."""
    kernels = code_object.kernels(native.build.HIP_LIB)
    tiles = code_object.named(kernels, "focus_tile_costs")
    assert len(tiles) == 2, sorted(tiles)
    for k, v in tiles.items():
        assert v[".private_segment_fixed_size"] == 0 and v[".vgpr_spill_count"] == 0 and v[".sgpr_spill_count"] == 0, (k, v)
        assert v[".vgpr_count"] <= 64 and v[".group_segment_fixed_size"] <= 32 * 1024, (k, v)
