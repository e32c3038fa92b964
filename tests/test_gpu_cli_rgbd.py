"""GPU (-m gpu): the command line's --rgbd-y4m — the Y4M file's header carries twice the tile's width and the frame rate, its one frame is the
restatement (tests/rgbd_yuv_ref.py) of the NN.png and mapK.png files the same run wrote, --rgbd-invert changes the depth half only, with
--view-maps the view's own map is stored, and two time steps of a light-field video give two frames in step order: an RGB-D video."""
import numpy as np
import pytest
from PIL import Image

import rgbd_yuv_ref as ref
import yuv_in_ref as in_ref
import yuv_ref
from test_host_yuv import parse_y4m
from view_rows import run_cli

pytestmark = pytest.mark.gpu

RUN = ["--synthetic", "4,4,32,16", "-t", "0,0,1,1", "-f", "0.0", "-r", "0.5", "-m", "STD", "-n", "6", "-b", "1"]


def _png(path):
    return np.array(Image.open(path))


def _y_halves(frame, tw, th):
    y = frame[:2 * tw * th].reshape(th, 2 * tw)
    return y[:, :tw], y[:, tw:]


def test_the_frame_is_the_restatement_of_the_written_view_and_map(gpu, tmp_path):
    """the defaults: the middle view (3 of 6), the views' size, map 1, BT.709 limited, 30 fps — and --rgbd-invert next to them"""
    dst, y4m = tmp_path / "out", tmp_path / "rgbd.y4m"
    res = run_cli(gpu, *RUN, "-o", str(dst), "--rgbd-y4m", str(y4m))
    assert res.returncode == 0, res.stderr
    tags, frames = parse_y4m(y4m.read_bytes())
    assert (int(tags["W"]), int(tags["H"]), tags["F"]) == (64, 16, "30:1") and "COLORRANGE=LIMITED" in tags["X"], tags
    assert len(frames) == 1
    view, depth = _png(dst / "03.png"), _png(dst / "map1.png")
    assert (frames[0] == ref.frame(view, depth, 32, 16, False, yuv_ref.BT709, yuv_ref.LIMITED)).all()
    # inverted: the colour half is the same, the depth half is not
    dst2, y4m2 = tmp_path / "out2", tmp_path / "inverted.y4m"
    res = run_cli(gpu, *RUN, "-o", str(dst2), "--rgbd-y4m", str(y4m2), "--rgbd-invert")
    assert res.returncode == 0, res.stderr
    _, inverted = parse_y4m(y4m2.read_bytes())
    assert (_png(dst2 / "03.png") == view).all() and (_png(dst2 / "map1.png") == depth).all()
    assert (inverted[0] == ref.frame(view, depth, 32, 16, True, yuv_ref.BT709, yuv_ref.LIMITED)).all()
    colour, grey = _y_halves(frames[0], 32, 16)
    colour_i, grey_i = _y_halves(inverted[0], 32, 16)
    assert (colour == colour_i).all() and not (grey == grey_i).all()
    assert (frames[0][64 * 16:] == inverted[0][64 * 16:]).all()   # the chroma of the depth half is 128 either way


def test_view_tile_map_and_the_video_options(gpu, tmp_path):
    dst, y4m = tmp_path / "out", tmp_path / "rgbd.y4m"
    res = run_cli(gpu, *RUN, "-o", str(dst), "--rgbd-y4m", str(y4m), "--rgbd-view", "5", "--rgbd-tile", "18x10", "--rgbd-map", "0", "--fps", "30000:1001",
                  "--yuv-matrix", "601", "--yuv-range", "full")
    assert res.returncode == 0, res.stderr
    tags, frames = parse_y4m(y4m.read_bytes())
    assert (int(tags["W"]), int(tags["H"]), tags["F"]) == (36, 10, "30000:1001") and "COLORRANGE=FULL" in tags["X"], tags
    assert len(frames) == 1
    assert (frames[0] == ref.frame(_png(dst / "05.png"), _png(dst / "map0.png"), 18, 10, False, yuv_ref.BT601, yuv_ref.FULL)).all()


def test_with_view_maps_the_views_own_map_is_stored(gpu, tmp_path):
    dst, y4m = tmp_path / "out", tmp_path / "rgbd.y4m"
    res = run_cli(gpu, *RUN, "-c", "--view-maps", "-o", str(dst), "--rgbd-y4m", str(y4m), "--rgbd-view", "1")
    assert res.returncode == 0, res.stderr
    _, frames = parse_y4m(y4m.read_bytes())
    assert len(frames) == 1
    assert (frames[0] == ref.frame(_png(dst / "01.png"), _png(dst / "map1_01.png"), 32, 16, False, yuv_ref.BT709, yuv_ref.LIMITED)).all()
    assert not (_png(dst / "map1_01.png") == _png(dst / "map1_04.png")).all()


def test_an_odd_view_size_needs_a_tile_size(gpu, tmp_path):
    """the default tile is the views' size: 33 x 16 is refused before anything is rendered or written"""
    dst, y4m = tmp_path / "out", tmp_path / "rgbd.y4m"
    res = run_cli(gpu, "--synthetic", "4,4,33,16", *RUN[2:], "-o", str(dst), "--rgbd-y4m", str(y4m))
    assert res.returncode != 0 and "--rgbd-tile" in res.stderr and "even" in res.stderr, res.stderr
    assert not dst.exists() and not y4m.exists()


def test_two_time_steps_give_two_frames_in_step_order(gpu, native, tmp_path):
    cols = rows = 2
    w, h, steps, views = 18, 6, 2, 4
    d = tmp_path / "lf"
    d.mkdir()
    for c in range(cols):
        for r in range(rows):
            native.write_y4m(str(d / f"{r}_{c}.y4m"), np.random.default_rng(10 * c + r).integers(0, 256, (steps, in_ref.sizes(w, h)[2]), dtype=np.uint8), w, h)
    dst, y4m = tmp_path / "out", tmp_path / "rgbd.y4m"
    res = run_cli(gpu, "-i", str(d), "--frames", "0:2", "-o", str(dst), "-t", "0,0.5,1,0.5", "-f", "0.0", "-r", "0.5", "-b", "1", "-m", "STD", "-n", str(views),
                  "--rgbd-tile", "10x4", "--rgbd-y4m", str(y4m), "--fps", "24")
    assert res.returncode == 0, res.stderr
    tags, frames = parse_y4m(y4m.read_bytes())
    assert (int(tags["W"]), int(tags["H"]), tags["F"]) == (20, 4, "24:1") and len(frames) == steps
    want = [ref.frame(_png(dst / f"f{t:04d}" / "02.png"), _png(dst / f"f{t:04d}" / "map1.png"), 10, 4, False, yuv_ref.BT709, yuv_ref.LIMITED) for t in range(steps)]
    assert not (want[0] == want[1]).all()
    for t in range(steps):
        assert (frames[t] == want[t]).all(), t
