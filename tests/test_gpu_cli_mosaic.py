"""GPU (-m gpu): the command line's mosaic input (-i FILE --mosaic CxR).  A Y4M mosaic is a light-field video in one file: it gives the files
the equivalent directory of per-camera <row>_<col>.y4m files gives, byte for byte.  A PNG quilt gives the views of the directory of its tiles."""
import numpy as np
import pytest
from PIL import Image

import yuv_in_ref as ref
from view_rows import run_cli

pytestmark = pytest.mark.gpu

COLS, ROWS = 3, 2
W, H, STEPS, VIEWS = 32, 16, 2, 4          # --synthetic-sized tiles
RENDER = ["-t", "0,0.5,1,0.5", "-m", "STD", "-f", "0.1", "-n", str(VIEWS), "-b", "1"]


def _same_files(a, b):
    names = sorted(str(p.relative_to(a)) for p in a.rglob("*") if p.is_file())
    assert names and names == sorted(str(p.relative_to(b)) for p in b.rglob("*") if p.is_file())
    for name in names:
        if name.endswith(".png"):
            assert (np.array(Image.open(a / name)) == np.array(Image.open(b / name))).all(), name
        else:
            assert (a / name).read_bytes() == (b / name).read_bytes(), name
    return names


@pytest.mark.parametrize("site", ["420jpeg", "420mpeg2"])
def test_y4m_mosaic_equals_the_directory_of_camera_videos(gpu, tmp_path, site):
    rng = np.random.default_rng(40)
    cams = {(c, r): rng.integers(0, 256, (STEPS, ref.sizes(W, H)[2]), dtype=np.uint8) for c in range(COLS) for r in range(ROWS)}
    d = tmp_path / "cams"
    d.mkdir()
    mosaic = np.empty((STEPS, ref.sizes(COLS * W, ROWS * H)[2]), np.uint8)
    for t in range(STEPS):
        y, cb, cr = (np.empty(s, np.int64) for s in ((ROWS * H, COLS * W), (ROWS * H // 2, COLS * W // 2), (ROWS * H // 2, COLS * W // 2)))
        for (c, r), frames in cams.items():
            ty, tcb, tcr = ref.split(frames[t], W, H)
            y[r * H:(r + 1) * H, c * W:(c + 1) * W] = ty
            cb[r * H // 2:(r + 1) * H // 2, c * W // 2:(c + 1) * W // 2] = tcb
            cr[r * H // 2:(r + 1) * H // 2, c * W // 2:(c + 1) * W // 2] = tcr
        mosaic[t] = ref.pack(y, cb, cr)
    left = site == "420mpeg2"
    for (c, r), frames in cams.items():
        gpu.write_y4m(str(d / f"{r}_{c}.y4m"), frames, W, H, left_sited=left)
    gpu.write_y4m(str(tmp_path / "mosaic.y4m"), mosaic, COLS * W, ROWS * H, left_sited=left)
    extra = ["--frames", "0:2", "--in-matrix", "601", "--in-chroma-site", "auto"]
    got, want = tmp_path / "got", tmp_path / "want"
    res = run_cli(gpu, "-i", str(tmp_path / "mosaic.y4m"), "--mosaic", f"{COLS}x{ROWS}", *extra, *RENDER, "--y4m", str(got / "v.y4m"), "-o", str(got / "out"))
    assert res.returncode == 0, res.stderr
    res = run_cli(gpu, "-i", str(d), *extra, *RENDER, "--y4m", str(want / "v.y4m"), "-o", str(want / "out"))
    assert res.returncode == 0, res.stderr
    names = _same_files(got, want)
    assert "v.y4m" in names and sum(n.endswith(".png") for n in names) == STEPS * VIEWS
    # --frames beyond the file's
    res = run_cli(gpu, "-i", str(tmp_path / "mosaic.y4m"), "--mosaic", f"{COLS}x{ROWS}", "--frames", "1:2", *RENDER, "-o", str(tmp_path / "none"))
    assert res.returncode != 0 and "--frames" in res.stderr and not (tmp_path / "none").exists()


def test_png_quilt_equals_the_directory_of_its_tiles(gpu, tmp_path):
    """--mosaic 3x2 --mosaic-order rows --mosaic-bottom-up: tile t counts from the bottom left and is the image of file 0_<t>; an odd size"""
    w, h = 15, 7
    rng = np.random.default_rng(41)
    tiles = rng.integers(0, 256, (6, h, w, 3), dtype=np.uint8)
    d = tmp_path / "tiles"
    d.mkdir()
    quilt = np.empty((2 * h, 3 * w, 3), np.uint8)
    for t in range(6):
        Image.fromarray(tiles[t]).save(d / f"0_{t}.png")
        tx, ty = t % 3, 1 - t // 3
        quilt[ty * h:(ty + 1) * h, tx * w:(tx + 1) * w] = tiles[t]
    Image.fromarray(quilt).save(tmp_path / "quilt.png")
    render = ["-t", "0,0,1,0", "-m", "STD", "-f", "0.1", "-n", str(VIEWS), "-b", "1"]
    res = run_cli(gpu, "-i", str(tmp_path / "quilt.png"), "--mosaic", "3x2", "--mosaic-order", "rows", "--mosaic-bottom-up", *render, "-o", str(tmp_path / "got"))
    assert res.returncode == 0, res.stderr
    res = run_cli(gpu, "-i", str(d), *render, "-o", str(tmp_path / "want"))
    assert res.returncode == 0, res.stderr
    assert len(_same_files(tmp_path / "got", tmp_path / "want")) == VIEWS
    # the same quilt read top-down is another light field
    res = run_cli(gpu, "-i", str(tmp_path / "quilt.png"), "--mosaic", "3x2", "--mosaic-order", "rows", *render, "-o", str(tmp_path / "down"))
    assert res.returncode == 0, res.stderr
    assert any((np.array(Image.open(tmp_path / "down" / f"{v:02d}.png")) != np.array(Image.open(tmp_path / "want" / f"{v:02d}.png"))).any() for v in range(VIEWS))
