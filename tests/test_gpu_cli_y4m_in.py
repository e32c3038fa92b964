"""GPU (-m gpu): the command line's light-field video input — a directory of per-camera Y4M files and --frames FIRST:COUNT.  Every time step's
files equal those of a run from a directory of PNGs holding the numpy restatement's RGBA (tests/yuv_in_ref.py) of that step's frames, and the
one --y4m file holds the steps' views in step order."""
import numpy as np
import pytest
from PIL import Image

import yuv_in_ref as ref
from test_host_yuv import parse_y4m
from view_rows import run_cli

pytestmark = pytest.mark.gpu

COLS = ROWS = 2
W, H, STEPS, VIEWS = 32, 24, 3, 4
RENDER = ["-t", "0,0.5,1,0.5", "-m", "STD", "-f", "0.1", "-n", str(VIEWS), "-b", "1"]


@pytest.fixture(scope="module")
def video_dir(native, tmp_path_factory):
    """(directory, {(col, row): [STEPS][frame_bytes]})"""
    d = tmp_path_factory.mktemp("lfvideo")
    cams = {}
    for c in range(COLS):
        for r in range(ROWS):
            cams[(c, r)] = np.random.default_rng(100 * c + r).integers(0, 256, (STEPS, ref.sizes(W, H)[2]), dtype=np.uint8)
            native.write_y4m(str(d / f"{r}_{c}.y4m"), cams[(c, r)], W, H)
    return d, cams


def test_time_steps_equal_runs_from_images(gpu, tmp_path, video_dir):
    d, cams = video_dir
    out, video = tmp_path / "out", tmp_path / "out.y4m"
    res = run_cli(gpu, "-i", str(d), "--frames", "1:2", *RENDER, "--y4m", str(video), "-o", str(out))
    assert res.returncode == 0, res.stderr
    assert sorted(p.name for p in out.iterdir()) == ["f0001", "f0002"]
    tags, frames = parse_y4m(video.read_bytes())
    assert (tags["W"], tags["H"], tags["C"]) == (str(W), str(H), "420jpeg") and len(frames) == 2 * VIEWS
    for k, t in enumerate((1, 2)):
        # the same step from images: the restatement's RGBA (the defaults: BT.709, the files' limited range, bilinear) as <row>_<col>.png
        images = tmp_path / f"images{t}"
        images.mkdir()
        for (c, r), cam in cams.items():
            gpu.write_png(str(images / f"{r}_{c}.png"), ref.rgba(cam[t], W, H, ref.BT709, ref.LIMITED, ref.BILINEAR))
        want, want_video = tmp_path / f"want{t}", tmp_path / f"want{t}.y4m"
        res = run_cli(gpu, "-i", str(images), *RENDER, "--y4m", str(want_video), "-o", str(want))
        assert res.returncode == 0, res.stderr
        names = sorted(p.name for p in want.iterdir())
        assert names == [f"{v:02d}.png" for v in range(VIEWS)] == sorted(p.name for p in (out / f"f{t:04d}").iterdir())
        for name in names:
            assert (np.array(Image.open(out / f"f{t:04d}" / name)) == np.array(Image.open(want / name))).all(), (t, name)
        _, want_frames = parse_y4m(want_video.read_bytes())
        assert len(want_frames) == VIEWS
        for v in range(VIEWS):
            assert (frames[k * VIEWS + v] == want_frames[v]).all(), (t, v)


def test_one_step_goes_to_the_output_directory(gpu, tmp_path, video_dir):
    """COUNT 1: as with image inputs, into -o itself; --in-range / --in-matrix / --in-chroma reach the conversion"""
    d, cams = video_dir
    res = run_cli(gpu, "-i", str(d), "--frames", "2", "--in-matrix", "601", "--in-range", "full", "--in-chroma", "nearest", *RENDER, "-o", str(tmp_path / "out"))
    assert res.returncode == 0, res.stderr
    images = tmp_path / "images"
    images.mkdir()
    for (c, r), cam in cams.items():
        gpu.write_png(str(images / f"{r}_{c}.png"), ref.rgba(cam[2], W, H, ref.BT601, ref.FULL, ref.NEAREST))
    assert run_cli(gpu, "-i", str(images), *RENDER, "-o", str(tmp_path / "want")).returncode == 0
    for v in range(VIEWS):
        assert (np.array(Image.open(tmp_path / "out" / f"{v:02d}.png")) == np.array(Image.open(tmp_path / "want" / f"{v:02d}.png"))).all(), v


def test_refusals(gpu, tmp_path, video_dir):
    d, _ = video_dir
    res = run_cli(gpu, "-i", str(d), "--frames", "5", *RENDER, "-o", str(tmp_path / "out"))
    assert res.returncode != 0 and "--frames" in res.stderr and "3 frames" in res.stderr, res.stderr
    res = run_cli(gpu, "-i", str(d), "--frames", "2:2", *RENDER, "-o", str(tmp_path / "out"))
    assert res.returncode != 0 and "--frames" in res.stderr, res.stderr
    res = run_cli(gpu, "-i", str(d), "--frames", "0:2", "--compare-methods", *RENDER, "-o", str(tmp_path / "out"))
    assert res.returncode != 0 and "--frames" in res.stderr and "--compare-methods" in res.stderr, res.stderr
    assert not (tmp_path / "out").exists()
