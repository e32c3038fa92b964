"""GPU (-m gpu): the command line's --lean-inputs — a light-field video whose later time steps go straight into the planar copy of the inputs
(lfi_release_inputs after the first step, lfi_upload_images_yuv_derived from then on).  Every file written equals the run without the flag,
byte for byte."""
import numpy as np
import pytest

import yuv_in_ref as ref
from view_rows import run_cli

pytestmark = pytest.mark.gpu

COLS = ROWS = 2
W, H, STEPS, VIEWS = 18, 6, 3, 4


@pytest.fixture(scope="module")
def video_dir(native, tmp_path_factory):
    d = tmp_path_factory.mktemp("lfvideo_lean")
    for c in range(COLS):
        for r in range(ROWS):
            frames = np.random.default_rng(300 + 10 * c + r).integers(0, 256, (STEPS, ref.sizes(W, H)[2]), dtype=np.uint8)
            native.write_y4m(str(d / f"{r}_{c}.y4m"), frames, W, H)
    return d


@pytest.mark.parametrize("method", ["STD", "TEN_WM"])
def test_files_equal_the_run_without_the_flag(method, gpu, tmp_path, video_dir):
    render = ["-i", str(video_dir), "--frames", f"0:{STEPS}", "-t", "0,0.5,1,0.5", "-m", method, "-f", "2.0", "-n", str(VIEWS), "-b", "1"]
    runs = {}
    for name, flag in (("plain", []), ("lean", ["--lean-inputs"])):
        out, video = tmp_path / name, tmp_path / f"{name}.y4m"
        res = run_cli(gpu, *render, *flag, "--y4m", str(video), "-o", str(out))
        assert res.returncode == 0, res.stderr
        runs[name] = (out, video)
    steps = [f"f{t:04d}" for t in range(STEPS)]
    for name in runs:
        assert sorted(p.name for p in runs[name][0].iterdir()) == steps
    differing_steps = 0
    for step in steps:
        names = [f"{v:02d}.png" for v in range(VIEWS)]
        assert sorted(p.name for p in (runs["lean"][0] / step).iterdir()) == names == sorted(p.name for p in (runs["plain"][0] / step).iterdir())
        for png in names:
            assert (runs["lean"][0] / step / png).read_bytes() == (runs["plain"][0] / step / png).read_bytes(), (step, png)
        differing_steps += (runs["plain"][0] / step / "00.png").read_bytes() != (runs["plain"][0] / steps[0] / "00.png").read_bytes()
    assert differing_steps == STEPS - 1   # the steps show different frames: a step that kept the first one's would not pass
    assert runs["lean"][1].read_bytes() == runs["plain"][1].read_bytes()
