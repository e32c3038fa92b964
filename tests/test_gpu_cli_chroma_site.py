"""GPU (-m gpu): the command line's chroma siting — --chroma-site left writes left-sited frames tagged C420mpeg2, --in-chroma-site auto reads
a directory of C420mpeg2 videos left-sited, and the default reads it as before, with its note."""
import numpy as np
import pytest
from PIL import Image

import yuv_in_ref as in_ref
import yuv_left_ref as left
import yuv_ref as out_ref
from test_host_yuv import parse_y4m
from view_rows import run_cli

pytestmark = pytest.mark.gpu

COLS = ROWS = 2
W, H, VIEWS = 34, 22, 3
RENDER = ["-t", "0,0.5,1,0.5", "-m", "STD", "-f", "0.1", "-n", str(VIEWS), "-b", "1"]


def _views(d):
    return np.stack([np.array(Image.open(d / f"{v:02d}.png")) for v in range(VIEWS)])


@pytest.fixture(scope="module")
def mpeg2_dir(native, tmp_path_factory):
    """(directory of C420mpeg2 files of two frames, {(col, row): frames})"""
    d = tmp_path_factory.mktemp("lfvideo_mpeg2")
    cams = {}
    for c in range(COLS):
        for r in range(ROWS):
            cams[(c, r)] = np.random.default_rng(100 * c + r + 7).integers(0, 256, (2, in_ref.sizes(W, H)[2]), dtype=np.uint8)
            native.write_y4m(str(d / f"{r}_{c}.y4m"), cams[(c, r)], W, H, left_sited=True)
    return d, cams


def test_chroma_site_left_writes_left_sited_frames(gpu, tmp_path):
    out = tmp_path / "out"
    video, nv12, centre = tmp_path / "left.y4m", tmp_path / "left.nv12", tmp_path / "centre.y4m"
    args = ["--synthetic", f"3,3,{W},{H}", *RENDER, "--yuv-matrix", "601"]
    res = run_cli(gpu, *args, "--chroma-site", "left", "--y4m", str(video), "--nv12", str(nv12), "-o", str(out))
    assert res.returncode == 0, res.stderr
    views = _views(out)
    tags, frames = parse_y4m(video.read_bytes())
    assert (tags["W"], tags["H"], tags["C"]) == (str(W), str(H), "420mpeg2") and len(frames) == VIEWS
    want = left.frames(views, out_ref.BT601, out_ref.LIMITED)
    assert all((frames[v] == want[v]).all() for v in range(VIEWS))
    # the raw NV12 file: the same planes, chroma interleaved
    raw = np.frombuffer(nv12.read_bytes(), np.uint8).reshape(VIEWS, -1)
    cw, ch, fb = out_ref.sizes(W, H)
    assert raw.shape[1] == fb and (raw[:, :W * H] == want[:, :W * H]).all()
    assert (raw[:, W * H::2] == want[:, W * H:W * H + cw * ch]).all() and (raw[:, W * H + 1::2] == want[:, W * H + cw * ch:]).all()
    # the default, and --chroma-site centre: today's file
    res = run_cli(gpu, *args, "--chroma-site", "centre", "--y4m", str(centre), "-o", str(tmp_path / "out2"))
    assert res.returncode == 0, res.stderr
    tags, frames = parse_y4m(centre.read_bytes())
    assert tags["C"] == "420jpeg" and all((frames[v] == out_ref.frame(views[v], out_ref.BT601, out_ref.LIMITED)).all() for v in range(VIEWS))


def _from_images(gpu, tmp_path, cams, rgba, name):
    images = tmp_path / f"images_{name}"
    images.mkdir()
    for (c, r), cam in cams.items():
        gpu.write_png(str(images / f"{r}_{c}.png"), rgba(cam[0]))
    res = run_cli(gpu, "-i", str(images), *RENDER, "-o", str(tmp_path / f"want_{name}"))
    assert res.returncode == 0, res.stderr
    return _views(tmp_path / f"want_{name}")


def test_in_chroma_site_auto_and_the_default(gpu, tmp_path, mpeg2_dir):
    d, cams = mpeg2_dir
    want_left = _from_images(gpu, tmp_path, cams, lambda f: left.rgba(f, W, H, in_ref.BT709, in_ref.LIMITED), "left")
    want_centre = _from_images(gpu, tmp_path, cams, lambda f: in_ref.rgba(f, W, H, in_ref.BT709, in_ref.LIMITED), "centre")
    assert not (want_left == want_centre).all()
    for flags, want in ((["--in-chroma-site", "auto"], want_left), (["--in-chroma-site", "left"], want_left), ([], want_centre),
                        (["--in-chroma-site", "centre"], want_centre)):
        out = tmp_path / ("out_" + "_".join(f.strip("-") for f in flags))
        res = run_cli(gpu, "-i", str(d), *flags, *RENDER, "-o", str(out))
        assert res.returncode == 0, res.stderr
        assert (_views(out) == want).all(), flags
        if want is want_left:
            assert "left-sited" in res.stdout and "Note: the videos are" not in res.stdout, res.stdout
        else:
            # today's note, with its half sentence that names the flag
            assert "Note: the videos are C420mpeg2; their chroma is read as centre-sited (C420jpeg), at most a quarter pixel from where it was sampled" in res.stdout
            assert "--in-chroma-site" in res.stdout
    # two time steps, the second one straight into the planar copy (--lean-inputs): the setting reaches lfi_upload_images_yuv_derived
    runs = {}
    for name, flags in (("rgba", []), ("lean", ["--lean-inputs"])):
        res = run_cli(gpu, "-i", str(d), "--in-chroma-site", "auto", "--frames", "0:2", *flags, *RENDER, "-o", str(tmp_path / name))
        assert res.returncode == 0, res.stderr
        runs[name] = [_views(tmp_path / name / f"f{t:04d}") for t in (0, 1)]
    assert (runs["rgba"][0] == want_left).all() and not (runs["rgba"][1] == want_left).all()
    assert all((runs["lean"][t] == runs["rgba"][t]).all() for t in (0, 1))
    # cameras that disagree are an error under auto
    mixed = tmp_path / "mixed"
    mixed.mkdir()
    for (c, r), cam in cams.items():
        gpu.write_y4m(str(mixed / f"{r}_{c}.y4m"), cam, W, H, left_sited=(c, r) != (1, 1))
    res = run_cli(gpu, "-i", str(mixed), "--in-chroma-site", "auto", *RENDER, "-o", str(tmp_path / "out_mixed"))
    assert res.returncode != 0 and "--in-chroma-site auto" in res.stderr and not (tmp_path / "out_mixed").exists()
