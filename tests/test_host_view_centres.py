"""CPU: the host side of view-centred shifts (lfi_set_view_float_offsets) — each view's offsets about its own camera against the oracle's
parameterisation of the trajectory collapsed onto that camera, and the new symbols in the header, the libraries and the bindings."""
import ctypes as C
import os
import re

import numpy as np
import pytest

CASES = [  # cols, rows, W, H, trajectory, aspect, views, focus
    (8, 8, 64, 48, "0,0,1,1", 1.0, 64, 0.0),
    (8, 8, 1920, 1080, "0,0,1,1", 1.783, 64, 0.23),
    (3, 3, 33, 17, "0,0,1,1", 1.783, 5, 0.5),
    (4, 4, 40, 40, "0,0.5,1,0.5", 1.0, 7, -0.6),
    (15, 15, 70, 20, "0.071,0.071,0.93,0.93", 2.02, 9, 0.3),
    (1, 1, 16, 16, "0,0,0,0", 1.0, 1, 0.5),
    (5, 2, 300, 7, "0,0,1,1", 0.5, 70, 1.25),
    (2, 1, 8, 8, "0,0,1,0", 1.0, 5, 0.25),   # half-way ties: shifts of ±0.5, ±1.5 … pixels
]


def _want(oc, cols, rows, W, H, traj, aspect, focus_v):
    se = oc.interpret_trajectory(traj, cols, rows)
    V = len(focus_v)
    O, D = [], []
    for v in range(V):
        cam = oc.trajectory_point(se, V, v)
        o, d = oc.offsets((cam[0], cam[1], cam[0], cam[1]), cols, rows, W, H, aspect, float(focus_v[v]))
        O.append(o)
        D.append(d)
    return np.stack(O), np.stack(D)


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}x{c[1]}@{c[2]}x{c[3]}_{c[4]}_v{c[6]}" for c in CASES])
def test_rows_equal_the_oracles_collapsed_trajectory(native, oracle_c, case):
    cols, rows, W, H, traj, aspect, V, f = case
    focus_v = np.full(V, f, np.float32)
    O, D = native.build_view_centred_offsets(cols, rows, W, H, traj, aspect, focus_v)
    assert O.shape == (V, cols * rows, 2) and O.dtype == np.float32
    assert D.shape == (V, cols * rows, 2) and D.dtype == np.int32
    want_O, want_D = _want(oracle_c, cols, rows, W, H, traj, aspect, focus_v)
    assert (O.view(np.uint32) == want_O.view(np.uint32)).all()
    assert (D == want_D).all()


def test_half_way_ties_round_away_from_zero(native, oracle_c):
    # 2×1 grid, width 8, trajectory along the row: camera v of 5 sits at column v/4; image 1's shift x is (v/4 − 1)/2·8 pixels, at focus 0.25
    # ±0.5 for v = 1, 3 exactly — rounded half away from zero like the reference's round()
    O, D = native.build_view_centred_offsets(2, 1, 8, 8, "0,0,1,0", 1.0, [0.25] * 5)
    assert O[:, 1, 0].tolist() == [-4.0, -3.0, -2.0, -1.0, 0.0]
    assert D[:, 1, 0].tolist() == [-1, -1, -1, 0, 0]   # −1, −0.75 → −1, −0.5 → −1, −0.25 → 0, 0
    assert D[:, 0, 0].tolist() == [0, 0, 1, 1, 1]      # 0, 0.25 → 0, 0.5 → 1, 0.75 → 1, 1


def test_zero_length_trajectory_gives_the_ordinary_parameters(native):
    # every camera is the trajectory's centre: every row is lfi_params.offsets and focused_offsets
    for cols, rows, W, H, traj, aspect, f in [(8, 8, 64, 48, "0.5,0.5,0.5,0.5", 1.0, 0.23), (15, 15, 70, 20, "0.3,0.8,0.3,0.8", 1.783, -0.4),
                                              (3, 5, 33, 17, "0,1,0,1", 0.5, 1.1)]:
        V = 6
        O, D = native.build_view_centred_offsets(cols, rows, W, H, traj, aspect, np.full(V, f, np.float32))
        hp = native.build_params(cols, rows, W, H, traj, f, 0.0, 3.0, aspect, V)
        for v in range(V):
            assert (O[v].view(np.uint32) == hp.offsets.view(np.uint32)).all()
            assert (D[v] == hp.focused_offsets).all()


def test_centre_view_of_an_odd_trajectory_is_the_ordinary_row(native):
    # 9 views on 0,0 → 1,1: camera 4 is the centre (both computed in float; the centre equals camera 4 for this grid)
    O, D = native.build_view_centred_offsets(5, 5, 40, 40, "0,0,1,1", 1.0, np.full(9, 0.3, np.float32))
    hp = native.build_params(5, 5, 40, 40, "0,0,1,1", 0.3, 0.0, 3.0, 1.0, 9)
    assert (O[4] == hp.offsets).all() and (D[4] == hp.focused_offsets).all()
    assert not (O[0] == hp.offsets).all()


def test_focus_ramp_composes(native, oracle_c):
    # what -c -f 0.1 -F 0.7 sets: view v at its own camera and the ramp's v-th focus
    cols, rows, W, H, traj, V = 4, 4, 48, 20, "0,0,1,1", 12
    ramp = native.focus_ramp(0.1, 0.7, V)
    O, D = native.build_view_centred_offsets(cols, rows, W, H, traj, 1.0, ramp)
    want_O, want_D = _want(oracle_c, cols, rows, W, H, traj, 1.0, ramp)
    assert (O == want_O).all() and (D == want_D).all()
    # the float rows do not depend on the focus; the integer rows are round(O * f_v)
    O0, _ = native.build_view_centred_offsets(cols, rows, W, H, traj, 1.0, np.zeros(V, np.float32))
    assert (O == O0).all()


@pytest.mark.parametrize("traj", ["0,0,1", "0,0,1,1,1", "a,b,c,d", ""])
def test_bad_trajectories_are_rejected(native, traj):
    with pytest.raises(RuntimeError):
        native.build_view_centred_offsets(3, 3, 32, 32, traj, 1.0, [0.1, 0.2])


def test_no_views_is_rejected(native):
    with pytest.raises(RuntimeError):
        native.build_view_centred_offsets(3, 3, 32, 32, "0,0,1,1", 1.0, np.zeros(0, np.float32))


def test_either_output_may_be_null(native):
    lib = native.load_host_library()
    f = np.full(3, 0.4, np.float32)
    O, D = native.build_view_centred_offsets(3, 3, 32, 32, "0,0,1,1", 1.0, f)
    o = np.zeros_like(O)
    d = np.zeros_like(D)
    err = C.create_string_buffer(256)
    assert lib.lfi_host_build_view_centred_offsets(3, 3, 32, 32, b"0,0,1,1", 1.0, f.ctypes.data, 3, o.ctypes.data, None, err, len(err)) == 0
    assert lib.lfi_host_build_view_centred_offsets(3, 3, 32, 32, b"0,0,1,1", 1.0, f.ctypes.data, 3, None, d.ctypes.data, err, len(err)) == 0
    assert (o == O).all() and (d == D).all()


def test_new_symbols_declared_exported_and_bound(native):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "lfi.h")).read()
    assert re.search(r"int\s+lfi_set_view_float_offsets\s*\(\s*lfi_ctx\s*\*\s*ctx\s*,\s*const\s+lfi_float2\s*\*\s*\w+\s*,\s*int\s+views\s*\)", header)
    assert "lfi_set_view_float_offsets" in native.ABI_SYMBOLS
    lib = native.load_hip_library()
    fn = lib.lfi_set_view_float_offsets  # exported
    assert fn.restype == C.c_int and len(fn.argtypes) == 3
    assert fn(None, None, 0) == -1       # without a context the call is refused, not a crash
    assert hasattr(native.Context, "set_view_float_offsets")
    assert native.load_host_library().lfi_host_build_view_centred_offsets
    assert "build_view_centred_offsets" in native.__all__
