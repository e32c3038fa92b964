"""GPU (-m gpu): the command line's --nv12 — the raw NV12 file of a run equals the frames of the --y4m file of the same run, re-interleaved
(tests/yuv_surfaces_ref.py), also for a run of two time steps of a light-field video, which go into the one file in step order."""
import numpy as np
import pytest

import yuv_in_ref as in_ref
import yuv_surfaces_ref as sref
from test_host_yuv import parse_y4m
from view_rows import run_cli

pytestmark = pytest.mark.gpu

RENDER = ["-t", "0,0.5,1,0.5", "-f", "0.1", "-b", "1"]


def _check(res, y4m, nv12, w, h, frames, rate):
    assert res.returncode == 0, res.stderr
    assert f"-f rawvideo -pix_fmt nv12 -s {w}x{h} -r {rate}" in res.stdout, res.stdout   # how ffmpeg opens the file
    _, want = parse_y4m(y4m.read_bytes())
    assert len(want) == frames
    lay = sref.tight(sref.NV12, w, h)
    assert nv12.stat().st_size == frames * lay.frame_stride
    got = np.frombuffer(nv12.read_bytes(), np.uint8).reshape(frames, lay.frame_stride)
    assert (got == sref.scatter(np.stack(want), lay, 0)).all()


@pytest.mark.parametrize("method,size,extra,rate", [("STD", (33, 17), [], "30"), ("TEN_WM", (48, 16), ["--fps", "30000:1001", "--yuv-matrix", "601", "--yuv-range", "full"], "30000/1001")],
                         ids=["STD-33x17", "TEN_WM-48x16-601-full"])
def test_the_file_is_the_y4m_frames_re_interleaved(gpu, tmp_path, method, size, extra, rate):
    w, h = size
    y4m, nv12 = tmp_path / "v.y4m", tmp_path / "v.nv12"
    res = run_cli(gpu, "--synthetic", f"3,3,{w},{h}", "-o", str(tmp_path / "out"), *RENDER, "-m", method, "-n", "5", "--y4m", str(y4m), "--nv12", str(nv12), *extra)
    _check(res, y4m, nv12, w, h, 5, rate)


def test_alone_and_over_two_time_steps(gpu, native, tmp_path):
    cols = rows = 2
    w, h, steps, views = 18, 6, 2, 3
    d = tmp_path / "lf"
    d.mkdir()
    for c in range(cols):
        for r in range(rows):
            native.write_y4m(str(d / f"{r}_{c}.y4m"), np.random.default_rng(10 * c + r).integers(0, 256, (steps, in_ref.sizes(w, h)[2]), dtype=np.uint8), w, h)
    y4m, nv12, alone = tmp_path / "v.y4m", tmp_path / "v.nv12", tmp_path / "alone.nv12"
    res = run_cli(gpu, "-i", str(d), "--frames", "0:2", "-o", str(tmp_path / "out"), *RENDER, "-m", "STD", "-n", str(views), "--y4m", str(y4m), "--nv12", str(nv12))
    _check(res, y4m, nv12, w, h, steps * views, "30")
    # without --y4m the file is the same
    res = run_cli(gpu, "-i", str(d), "--frames", "0:2", "-o", str(tmp_path / "out2"), *RENDER, "-m", "STD", "-n", str(views), "--nv12", str(alone))
    assert res.returncode == 0, res.stderr
    assert alone.read_bytes() == nv12.read_bytes()
