"""CPU: the host side of per-view focus (lfi_set_view_offsets) — the focus ramp, the per-view offset rows against the oracle's
parameterisation, and the new symbol in the header, the library and the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest


@pytest.mark.parametrize("f0,f1,views", [(0.0, 0.6, 12), (0.0, 0.5, 64), (0.2, 0.25, 64), (0.22, 0.39, 32), (-0.3, 0.45, 7),
                                         (0.5, -0.5, 5), (0.7, 0.1, 1), (1.25, 3.0, 9)])
def test_focus_ramp_is_float32_arithmetic(native, f0, f1, views):
    got = native.focus_ramp(f0, f1, views)
    f0_, f1_ = np.float32(f0), np.float32(f1)
    if views == 1:
        want = np.array([f0_], np.float32)
    else:
        step = np.float32((f1_ - f0_) / np.float32(views - 1))
        want = np.array([np.float32(f0_ + np.float32(step * np.float32(i))) for i in range(views)], np.float32)
    assert got.dtype == np.float32 and got.shape == (views,)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()


def test_focus_ramp_rejects_no_views(native):
    with pytest.raises(ValueError):
        native.focus_ramp(0.0, 1.0, 0)


CASES = [  # cols, rows, W, H, trajectory, aspect, focus values
    (8, 8, 64, 48, "0.5,0.5,0.5,0.5", 1.0, np.linspace(0.0, 0.5, 17)),
    (3, 3, 33, 17, "0,0,1,1", 1.783, [0.0, 0.1, 0.23, 0.5, 1.0, 1.5, 2.75]),
    (4, 4, 40, 40, "0,0.5,1,0.5", 1.0, [-0.6, -0.2, 0.0, 0.125, 0.25]),
    (15, 15, 64, 36, "0.071,0.071,0.93,0.93", 1.0, [0.22, 0.3, 0.39]),
    (1, 1, 16, 16, "0,0,0,0", 1.0, [0.0, 0.5]),
    (5, 2, 100, 30, "0.2,0.1,0.8,0.9", 0.5, [3.0, 0.75]),
]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}x{c[1]}@{c[2]}x{c[3]}" for c in CASES])
def test_view_offsets_equal_oracle_rows(native, oracle_c, case):
    cols, rows, W, H, traj, aspect, focus = case
    focus = np.asarray(focus, np.float32)
    d = native.build_view_offsets(cols, rows, W, H, traj, aspect, focus)
    assert d.shape == (len(focus), cols * rows, 2) and d.dtype == np.int32
    se = oracle_c.interpret_trajectory(traj, cols, rows)
    for v, f in enumerate(focus):
        _, want = oracle_c.offsets(se, cols, rows, W, H, aspect, float(f))
        assert (d[v] == want).all(), (v, float(f))
    # the row of the focus the ordinary parameters use is their focused_offsets
    hp = native.build_params(cols, rows, W, H, traj, float(focus[-1]), 0.0, 3.0, aspect, 2)
    assert (d[-1] == hp.focused_offsets).all()


def test_view_offsets_half_way_ties_round_away_from_zero(native, oracle_c):
    # 2 columns, width 8: shift x of the two images at the centre 0.5 is ±(0.5/2)·8 = ±2 pixels; focus 0.25 makes it ±0.5 exactly
    d = native.build_view_offsets(2, 1, 8, 8, "0.5,0,0.5,0", 1.0, [0.25, 0.75])
    assert sorted(d[0, :, 0].tolist()) == [-1, 1] and sorted(d[1, :, 0].tolist()) == [-2, 2]
    se = oracle_c.interpret_trajectory("0.5,0,0.5,0", 2, 1)
    for v, f in enumerate([0.25, 0.75]):
        assert (d[v] == oracle_c.offsets(se, 2, 1, 8, 8, 1.0, f)[1]).all()


def test_focus_ramp_rows_are_a_focus_pull(native, oracle_c):
    # what the command line's -f 0 -F 0.6 -n 12 sets: row v at the ramp's v-th value
    ramp = native.focus_ramp(0.0, 0.6, 12)
    d = native.build_view_offsets(4, 4, 48, 20, "0.5,0.5,0.5,0.5", 1.0, ramp)
    se = oracle_c.interpret_trajectory("0.5,0.5,0.5,0.5", 4, 4)
    for v in range(12):
        assert (d[v] == oracle_c.offsets(se, 4, 4, 48, 20, 1.0, float(ramp[v]))[1]).all()


def test_build_view_offsets_rejects_bad_trajectory(native):
    with pytest.raises(RuntimeError):
        native.build_view_offsets(3, 3, 32, 32, "0,0,1", 1.0, [0.1])


def test_set_view_offsets_declared_exported_and_bound(native):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "lfi.h")).read()
    assert re.search(r"int\s+lfi_set_view_offsets\s*\(\s*lfi_ctx\s*\*\s*ctx\s*,\s*const\s+lfi_int2\s*\*\s*\w+\s*,\s*int\s+views\s*\)", header)
    assert "lfi_set_view_offsets" in native.ABI_SYMBOLS
    lib = native.load_hip_library()
    fn = lib.lfi_set_view_offsets  # exported
    assert fn.restype == C.c_int and len(fn.argtypes) == 3
    assert lib.lfi_abi_version() == 1
    # without a context the call is refused, not a crash
    assert fn(None, None, 0) == -1
    assert hasattr(native.Context, "set_view_offsets")
    host = native.load_host_library()
    assert host.lfi_host_focus_ramp and host.lfi_host_build_view_offsets
