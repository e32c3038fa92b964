"""GPU (-m gpu): the command line's --quilt-y4m — the Y4M file's header carries the quilt's size and the frame rate, its one frame is the
restatement (tests/quilt_yuv_ref.py) of the NN.png files the same run wrote, and two time steps of a light-field video give two frames in
step order: a quilt video."""
import numpy as np
import pytest
from PIL import Image

import quilt_yuv_ref as ref
import yuv_in_ref as in_ref
import yuv_ref
from test_host_yuv import parse_y4m
from view_rows import run_cli

pytestmark = pytest.mark.gpu

RENDER = ["-t", "0,0.5,1,0.5", "-f", "0.1", "-b", "1"]


def _views(directory, n):
    return np.stack([np.array(Image.open(directory / f"{v:02d}.png")) for v in range(n)])


@pytest.mark.parametrize("tile,extra,conv,rate,colour", [((24, 10), [], (yuv_ref.BT709, yuv_ref.LIMITED), "30:1", "LIMITED"),
                                                        ((17, 9), ["--fps", "30000:1001", "--yuv-matrix", "601", "--yuv-range", "full"],
                                                         (yuv_ref.BT601, yuv_ref.FULL), "30000:1001", "FULL")], ids=["fused-24x10", "staged-17x9-601-full"])
def test_the_frame_is_the_restatement_of_the_written_views(gpu, tmp_path, tile, extra, conv, rate, colour):
    tw, th = tile
    dst, y4m = tmp_path / "out", tmp_path / "quilt.y4m"
    res = run_cli(gpu, "--synthetic", "4,4,48,20", "-o", str(dst), *RENDER, "-m", "TEN_WM", "-n", "6", "-q", "3,2", "--quilt-tile", f"{tw}x{th}",
                  "--quilt-y4m", str(y4m), *extra)
    assert res.returncode == 0, res.stderr
    tags, frames = parse_y4m(y4m.read_bytes())
    assert (int(tags["W"]), int(tags["H"]), tags["F"]) == (3 * tw, 2 * th, rate) and f"COLORRANGE={colour}" in tags["X"], tags
    assert len(frames) == 1
    views = _views(dst, 6)
    assert (frames[0] == ref.frame(views, 3, 2, tw, th, *conv)).all()
    assert np.array(Image.open(dst / "quilt.png")).shape == (2 * th, 3 * tw, 4)   # next to quilt.png, which is written as before


def test_without_a_tile_size_the_views_are_the_tiles(gpu, tmp_path):
    dst, y4m = tmp_path / "out", tmp_path / "quilt.y4m"
    res = run_cli(gpu, "--synthetic", "3,3,18,6", "-o", str(dst), *RENDER, "-m", "STD", "-n", "4", "-q", "2,2", "--quilt-y4m", str(y4m))
    assert res.returncode == 0, res.stderr
    tags, frames = parse_y4m(y4m.read_bytes())
    assert (int(tags["W"]), int(tags["H"])) == (36, 12) and len(frames) == 1
    assert (frames[0] == ref.frame(_views(dst, 4), 2, 2, 18, 6, yuv_ref.BT709, yuv_ref.LIMITED)).all()


def test_two_time_steps_give_two_frames_in_step_order(gpu, native, tmp_path):
    cols = rows = 2
    w, h, steps, views = 18, 6, 2, 4
    d = tmp_path / "lf"
    d.mkdir()
    for c in range(cols):
        for r in range(rows):
            native.write_y4m(str(d / f"{r}_{c}.y4m"), np.random.default_rng(10 * c + r).integers(0, 256, (steps, in_ref.sizes(w, h)[2]), dtype=np.uint8), w, h)
    dst, y4m = tmp_path / "out", tmp_path / "quilt.y4m"
    res = run_cli(gpu, "-i", str(d), "--frames", "0:2", "-o", str(dst), *RENDER, "-m", "STD", "-n", str(views), "-q", "2,2", "--quilt-tile", "10x4",
                  "--quilt-y4m", str(y4m), "--fps", "24")
    assert res.returncode == 0, res.stderr
    tags, frames = parse_y4m(y4m.read_bytes())
    assert (int(tags["W"]), int(tags["H"]), tags["F"]) == (20, 8, "24:1") and len(frames) == steps
    want = [ref.frame(_views(dst / f"f{t:04d}", views), 2, 2, 10, 4, yuv_ref.BT709, yuv_ref.LIMITED) for t in range(steps)]
    assert not (want[0] == want[1]).all()
    for t in range(steps):
        assert (frames[t] == want[t]).all(), t
