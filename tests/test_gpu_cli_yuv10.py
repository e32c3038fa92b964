"""GPU (-m gpu): the command line's 10-bit video — --yuv-depth 10 with --y4m and --quilt-y4m (C420p10 files of I010 frames), --p010 (raw P010
frames), a light-field video of C420p10 files as input, and the two combinations that are refused.  Every frame is the numpy restatement
(tests/yuv10_ref.py) of the PNG views the same run wrote."""
import numpy as np
import pytest
from PIL import Image

import yuv10_ref as ref
from view_rows import run_cli

pytestmark = pytest.mark.gpu

RENDER = ["-t", "0,0.5,1,0.5", "-f", "0.1", "-b", "1"]


def parse_y4m10(data, w, h):
    """(tags, [codes]) of a C420p10 file: the header's tokens by their letter and every frame's samples as uint16 in the order Y, Cb, Cr"""
    line, _, rest = data.partition(b"\n")
    tokens = line.decode().split(" ")
    assert tokens[0] == "YUV4MPEG2"
    tags = {}
    for t in tokens[1:]:
        tags.setdefault(t[0], []).append(t[1:])
    nbytes = 2 * ref.sizes(w, h)[2]
    frames = []
    while rest:
        assert rest.startswith(b"FRAME\n") and len(rest) >= 6 + nbytes
        frames.append(np.frombuffer(rest[6:6 + nbytes], "<u2"))
        rest = rest[6 + nbytes:]
    return tags, frames


def _views(dst, n, w, h):
    out = np.stack([np.array(Image.open(dst / f"{v:02d}.png")) for v in range(n)])
    assert out.shape == (n, h, w, 4)
    return out


@pytest.mark.parametrize("method,size,extra,fmt,siting", [
    ("STD", (33, 17), [], (ref.BT709, ref.LIMITED), ref.CENTRE),
    ("TEN_WM", (48, 16), ["--fps", "25", "--yuv-matrix", "601", "--yuv-range", "full", "--chroma-site", "left"], (ref.BT601, ref.FULL), ref.LEFT),
], ids=["STD-33x17", "TEN_WM-48x16-601-full-left"])
def test_y4m_and_p010_hold_the_restatement_of_the_png_views(gpu, tmp_path, method, size, extra, fmt, siting):
    w, h = size
    views = 5
    dst, y4m, p010 = tmp_path / "out", tmp_path / "v.y4m", tmp_path / "v.p010"
    res = run_cli(gpu, "--synthetic", f"3,3,{w},{h}", "-o", str(dst), *RENDER, "-m", method, "-n", str(views), "--yuv-depth", "10", "--y4m", str(y4m),
                  "--p010", str(p010), *extra)
    assert res.returncode == 0, res.stderr
    rate = "25" if extra else "30"
    assert f"-f rawvideo -pix_fmt p010le -s {w}x{h} -r {rate}" in res.stdout, res.stdout   # how ffmpeg opens the raw file
    # Y4M has no siting tag for 10-bit frames: the run says which one it used and how to tell ffmpeg
    assert f"-chroma_sample_location {'left' if siting == ref.LEFT else 'center'}" in res.stdout, res.stdout
    tags, frames = parse_y4m10(y4m.read_bytes(), w, h)
    assert (tags["W"], tags["H"], tags["F"], tags["I"], tags["A"], tags["C"]) == ([str(w)], [str(h)], [rate + ":1"], ["p"], ["1:1"], ["420p10"])
    assert tags["X"] == ["COLORRANGE=" + ("FULL" if fmt[1] == ref.FULL else "LIMITED")]
    want = ref.frames(_views(dst, views, w, h), *fmt, siting)
    assert len(frames) == views and (np.stack(frames) == want).all()
    lay = ref.tight(ref.P010, w, h)
    assert p010.stat().st_size == views * lay.frame_stride
    got = np.frombuffer(p010.read_bytes(), np.uint8).reshape(views, lay.frame_stride)
    assert (got == ref.scatter(want, lay, 0)).all()


def test_quilt_y4m_at_ten_bits(gpu, tmp_path):
    """-q 3,2 with tiles of 18 x 10: one C420p10 frame, the restatement of quilt.png"""
    w, h = 50, 22
    dst, video = tmp_path / "out", tmp_path / "q.y4m"
    res = run_cli(gpu, "--synthetic", f"3,3,{w},{h}", "-o", str(dst), *RENDER, "-m", "STD", "-n", "6", "-q", "3,2", "--quilt-tile", "18x10", "--quilt-y4m", str(video),
                  "--yuv-depth", "10")
    assert res.returncode == 0, res.stderr
    tags, frames = parse_y4m10(video.read_bytes(), 54, 20)
    assert tags["C"] == ["420p10"] and len(frames) == 1
    quilt = np.array(Image.open(dst / "quilt.png"))
    assert quilt.shape == (20, 54, 4)
    assert (frames[0] == ref.codes(quilt, ref.BT709, ref.LIMITED)).all()


@pytest.mark.parametrize("site,siting", [([], ref.CENTRE), (["--in-chroma-site", "auto"], ref.LEFT)], ids=["centre", "auto-left"])
def test_a_directory_of_c420p10_videos_renders_what_its_rgba_images_render(gpu, native, tmp_path, site, siting):
    cols = rows = 2
    w, h, steps, views = 18, 6, 2, 3
    d, png = tmp_path / "lf", tmp_path / "png"
    d.mkdir()
    png.mkdir()
    lay = ref.tight(ref.I010, w, h)
    for c in range(cols):
        for r in range(rows):
            codes = np.random.default_rng(10 * c + r).integers(0, 1024, (steps, ref.sizes(w, h)[2]), dtype=np.uint16)
            native.write_y4m(str(d / f"{r}_{c}.y4m"), ref.scatter(codes, lay, 0), w, h, full_range=True, depth=10)
            # time step 1 as the RGBA image the definition makes of it (the files' XCOLORRANGE tag gives the range, BT.601 is asked for)
            native.write_png(str(png / f"{r}_{c}.png"), ref.rgba(codes[1], w, h, ref.BT601, ref.FULL, ref.BILINEAR, siting))
    render = [*RENDER, "-m", "STD", "-n", str(views)]
    res = run_cli(gpu, "-i", str(d), "--frames", "1:1", "--in-matrix", "601", *site, "-o", str(tmp_path / "out"), *render)
    assert res.returncode == 0, res.stderr
    assert "10-bit" in res.stdout and ("left-sited" if siting == ref.LEFT else "centre-sited") in res.stdout, res.stdout
    res = run_cli(gpu, "-i", str(png), "-o", str(tmp_path / "want"), *render)
    assert res.returncode == 0, res.stderr
    assert (_views(tmp_path / "out", views, w, h) == _views(tmp_path / "want", views, w, h)).all()
    # mixed depths in one directory are an error
    native.write_y4m(str(d / "0_0.y4m"), np.zeros((steps, ref.sizes(w, h)[2]), np.uint8), w, h)
    res = run_cli(gpu, "-i", str(d), "-o", str(tmp_path / "mixed"), *render)
    assert res.returncode != 0 and "10-bit" in res.stderr, res.stderr


def test_refused_combinations(gpu, native, tmp_path):
    """--lean-inputs with 10-bit videos and --rgbd-y4m with --yuv-depth 10 end with a message that names the limitation, and write no video"""
    w, h = 18, 6
    d = tmp_path / "lf"
    d.mkdir()
    lay = ref.tight(ref.I010, w, h)
    for c in range(2):
        for r in range(2):
            codes = np.random.default_rng(c + 2 * r).integers(0, 1024, (2, ref.sizes(w, h)[2]), dtype=np.uint16)
            native.write_y4m(str(d / f"{r}_{c}.y4m"), ref.scatter(codes, lay, 0), w, h, depth=10)
    res = run_cli(gpu, "-i", str(d), "--frames", "0:2", "--lean-inputs", "-o", str(tmp_path / "lean"), *RENDER, "-m", "STD", "-n", "3", "--y4m", str(tmp_path / "lean.y4m"))
    assert res.returncode != 0 and "--lean-inputs" in res.stderr and "10-bit" in res.stderr and "planar copy" in res.stderr, res.stderr
    assert not (tmp_path / "lean.y4m").exists()
    res = run_cli(gpu, "--synthetic", "3,3,16,8", "-o", str(tmp_path / "rgbd"), "-t", "0,0.5,1,0.5", "-f", "0.1", "-r", "0.3", "-b", "1", "-m", "STD", "-n", "3",
                  "--rgbd-y4m", str(tmp_path / "d.y4m"), "--yuv-depth", "10")
    assert res.returncode != 0 and "--rgbd-y4m" in res.stderr and "10-bit RGB-D frames are not supported" in res.stderr, res.stderr
    assert not (tmp_path / "d.y4m").exists()
