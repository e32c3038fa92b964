"""CPU: the host side of per-view focus maps — lfinterpolator_amd.build_view_focus_ids (lfi_host_build_view_focus_ids,
Parameterizer::viewFocusMapIDs) against the oracle, and the CLI's checks of --view-maps."""
import numpy as np
import pytest

from view_rows import run_cli

# name, cols, rows, trajectory, views
CASES = [
    ("g1x1", 1, 1, "0,0,0,0", 3),
    ("g3x3", 3, 3, "0,0,1,1", 5),
    ("g8x8", 8, 8, "0,0,1,1", 64),
    ("g8x8_v97", 8, 8, "0.0,0.0,1.0,1.0", 97),
    ("g15x15", 15, 15, "0.071,0.071,0.93,0.93", 32),
    ("g5x2", 5, 2, "0,0,1,1", 70),
    ("g8x8_point", 8, 8, "0.5,0.5,0.5,0.5", 4),
    ("g15x15_row", 15, 15, "0,0.5,1,0.5", 9),
]


def _oracle_rows(oc, cols, rows, traj, V):
    se = oc.interpret_trajectory(traj, cols, rows)
    out = []
    for v in range(V):
        p = oc.trajectory_point(se, V, v)
        out.append(oc.focus_map_ids(np.array([p[0], p[1], p[0], p[1]], np.float32), cols, rows))
    return out


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_view_focus_ids_match_the_oracle_per_camera(native, oracle_c, case):
    _, cols, rows, traj, V = case
    got = native.build_view_focus_ids(cols, rows, traj, V)
    assert got.dtype == np.int32 and got.shape == (V, min(32, cols * rows))
    for v, want in enumerate(_oracle_rows(oracle_c, cols, rows, traj, V)):
        assert (got[v] == want).all(), (v, got[v], want)


def test_view_focus_ids_cover_ties_at_the_32nd_distance(native, oracle_c):
    """An 8x8 grid seen from a camera on a grid point: images at equal distances straddle the 32nd place, and the ids keep the
    reference's stable (id) order among them."""
    cols = rows = 8
    traj, V = "0,0,1,1", 8
    se = oracle_c.interpret_trajectory(traj, cols, rows)
    ties = 0
    for v in range(V):
        p = oracle_c.trajectory_point(se, V, v)
        d = np.array([np.float32(np.hypot(np.float32(g // rows) - p[0], np.float32(g % rows) - p[1])) for g in range(cols * rows)])
        s = np.sort(d, kind="stable")
        ties += int(s[31] == s[32])
    assert ties > 0
    got = native.build_view_focus_ids(cols, rows, traj, V)
    for v, want in enumerate(_oracle_rows(oracle_c, cols, rows, traj, V)):
        assert (got[v] == want).all(), v


def test_view_focus_ids_of_one_view_are_the_centre_ids(native):
    """One view: the camera is the trajectory's start, so a single-point trajectory's one row is build_params' focus_map_ids."""
    hp = native.build_params(8, 8, 64, 48, "0.3,0.6,0.3,0.6", 0.0, 0.5, 3.0, 1.0, 1)
    got = native.build_view_focus_ids(8, 8, "0.3,0.6,0.3,0.6", 1)
    assert (got[0] == hp.focus_map_ids).all()


def test_view_focus_ids_refuse_no_views(native):
    with pytest.raises(RuntimeError):
        native.build_view_focus_ids(8, 8, "0,0,1,1", 0)


@pytest.mark.parametrize("missing", ["-c", "-r"])
def test_cli_refuses_view_maps_without_view_centres_or_all_focus(native, tmp_path, missing):
    args = ["--synthetic", "4,4,32,16", "-t", "0,0,1,1", "-o", str(tmp_path / "out"), "-m", "STD", "-n", "4", "-b", "1",
            "-r", "0.5", "-c", "--view-maps"]
    i = args.index(missing)
    del args[i:i + (2 if missing == "-r" else 1)]
    res = run_cli(native, *args)
    assert res.returncode != 0
    assert "--view-maps" in res.stderr
    assert not (tmp_path / "out").exists()
