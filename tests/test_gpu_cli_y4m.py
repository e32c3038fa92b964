"""GPU (-m gpu): the command line's --y4m — the video file of a run parses, has as many frames as views, and every frame is the numpy restatement
(tests/yuv_ref.py) of the NN.png the same run wrote."""
import numpy as np
import pytest
from PIL import Image

import yuv_ref as ref
from test_host_yuv import parse_y4m
from view_rows import run_cli

pytestmark = pytest.mark.gpu


def _check(gpu, tmp_path, synthetic, method, extra, fps, fmt, views=6, gpus=1):
    dst = tmp_path / f"out_{method}_{gpus}"
    video = tmp_path / f"{method}_{gpus}.y4m"
    res = run_cli(gpu, "--synthetic", synthetic, "-o", str(dst), "-t", "0,0.5,1,0.5", "-m", method, "-f", "0.1", "-n", str(views), "-b", "1", "-g", str(gpus),
                  "--y4m", str(video), *extra)
    assert res.returncode == 0, res.stderr
    w, h = (int(v) for v in synthetic.split(",")[2:4])
    tags, frames = parse_y4m(video.read_bytes())
    assert (tags["W"], tags["H"], tags["F"], tags["I"], tags["A"], tags["C"]) == (str(w), str(h), fps, "p", "1:1", "420jpeg")
    assert tags["X"] == ["COLORRANGE=" + ("FULL" if fmt[1] == ref.FULL else "LIMITED")]
    assert len(frames) == views
    for v, frame in enumerate(frames):
        png = np.array(Image.open(dst / f"{v:02d}.png"))
        assert png.shape == (h, w, 4)
        assert (frame == ref.frame(png, *fmt)).all(), (method, v)


def test_cli_writes_the_views_as_one_video(gpu, tmp_path):
    # the defaults: 30:1, BT.709, limited range; TEN_WM at a fixed focus renders into the planar view layout, STD into RGBA planes
    _check(gpu, tmp_path, "4,4,48,20", "TEN_WM", [], "30:1", (ref.BT709, ref.LIMITED))
    _check(gpu, tmp_path, "3,3,17,9", "STD", ["--fps", "30000:1001", "--yuv-matrix", "601", "--yuv-range", "full"], "30000:1001", (ref.BT601, ref.FULL))
    _check(gpu, tmp_path, "3,3,17,9", "TEN_WM", ["--fps", "25", "--yuv-range", "full"], "25:1", (ref.BT709, ref.FULL))
    if gpu.load_hip_library().lfi_device_count() >= 2:
        # every GPU converts and downloads its own views into its part of the one buffer
        _check(gpu, tmp_path, "4,4,48,20", "TEN_WM", ["--yuv-matrix", "601"], "30:1", (ref.BT601, ref.LIMITED), views=7, gpus=2)
