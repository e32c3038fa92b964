"""CPU: the host side of the YUV 4:2:0 input (lfi_upload_images_yuv420, --frames) — the coefficient table against its derivation from the
matrix constants, the properties include/lfi.h states about the conversion (the bracket's bound, greys, the limited end points, the round
trip through the output's definition of tests/yuv_ref.py), the numpy restatement (tests/yuv_in_ref.py) on cases worked out by hand, the Y4M
reader (csrc/host/y4m.cpp through lfi_host_y4m_info / lfi_host_y4m_read), the loader of light-field videos (lfi_host_load_grid_y4m), the
exported symbols, the CLI's usage errors and the new kernel's code object."""
import math
import os
import re

import numpy as np
import pytest

import code_object
import yuv_in_ref as ref
import yuv_ref as out_ref
from view_rows import run_cli

# (Kr, Kb) of Y = Kr·R + (1 − Kr − Kb)·G + Kb·B:  ITU-R BT.709 / BT.601
LUMA = {ref.BT709: (0.2126, 0.0722), ref.BT601: (0.299, 0.114)}
# |colour − round trip| per channel over all colours: the header's figures
ROUND_TRIP = {ref.LIMITED: 2, ref.FULL: 1}


def _round(x):
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


# ---- the table ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("matrix,rng", ref.FORMATS)
def test_table_is_derived_from_the_matrix_constants(matrix, rng):
    """each entry round(c · scale · 2¹⁶)"""
    kr, kb = LUMA[matrix]
    kg = 1.0 - kr - kb
    ys, cs = (255.0 / 219.0, 255.0 / 224.0) if rng == ref.LIMITED else (1.0, 1.0)
    want = (_round(ys * 65536), _round(2 * (1 - kr) * cs * 65536), _round(-2 * kb * (1 - kb) / kg * cs * 65536),
            _round(-2 * kr * (1 - kr) / kg * cs * 65536), _round(2 * (1 - kb) * cs * 65536), 16 if rng == ref.LIMITED else 0)
    assert ref.TABLE[(matrix, rng)] == want


def test_header_and_kernel_carry_the_table():
    """the literals of include/lfi.h's comment and of csrc/hip/yuv420_upload.hpp's one table are those of the restatement"""
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "lfi.h")).read()
    header = header[header.index("cY       rV"):header.index("enum { LFI_CHROMA_BILINEAR")]
    kernel = open(os.path.join(ROOT, "lfinterpolator_amd", "csrc", "hip", "yuv420_upload.hpp")).read()
    table = kernel[kernel.index("constexpr YuvInCoeffs YUV_IN_COEFFS[4]"):]
    table = table[:table.index("};")]
    rows = [tuple(int(v) for v in re.findall(r"-?\d+", line.split("//")[0])) for line in table.splitlines() if line.strip().startswith("{")]
    assert rows == [ref.TABLE[f] for f in ref.FORMATS]
    names = {(ref.BT709, ref.LIMITED): "BT.709 limited", (ref.BT709, ref.FULL): "BT.709 full", (ref.BT601, ref.LIMITED): "BT.601 limited",
             (ref.BT601, ref.FULL): "BT.601 full"}
    for fmt, name in names.items():
        line = next(l for l in header.splitlines() if name in l)
        assert tuple(int(v) for v in re.findall(r"-?\d+", line.split(name)[1])) == ref.TABLE[fmt]
    assert "573,111,632" in header and ref.BRACKET_BOUND == 573111632


# ---- the properties the header states ---------------------------------------------------------------------------------------------------------

def test_bracket_bound_over_all_byte_triples():
    """every bracket of every (Y, 16·U, 16·V) stays within the header's figure, which one of them reaches: int32 suffices"""
    y, u, v = np.arange(256)[:, None, None], 16 * np.arange(256)[None, :, None], 16 * np.arange(256)[None, None, :]
    worst = 0
    for fmt in ref.FORMATS:
        for b in ref.brackets(y, u, v, *fmt):
            worst = max(worst, int(np.abs(np.broadcast_to(b, (256, 256, 256))).max()))
    assert worst == ref.BRACKET_BOUND and worst + (1 << 19) < 1 << 31


@pytest.mark.parametrize("matrix,rng", ref.FORMATS)
def test_greys_and_end_points(matrix, rng):
    y = np.arange(256)
    grey = ref.convert(y, np.full(256, 2048), np.full(256, 2048), matrix, rng)
    assert (grey[:, 0] == grey[:, 1]).all() and (grey[:, 1] == grey[:, 2]).all() and (grey[:, 3] == 255).all()
    assert (np.diff(grey[:, 0].astype(int)) >= 0).all()
    if rng == ref.LIMITED:
        assert grey[16, 0] == 0 and grey[235, 0] == 255 and grey[0, 0] == 0 and grey[255, 0] == 255   # codes outside [16, 235] are clamped
        assert grey[17, 0] > 0 and grey[234, 0] < 255
    else:
        assert (grey[:, 0] == y).all()


def _blocks_image(colours):
    """[2·bh][2·bw][3] uint8: block (j, i) uniformly colours[j][i]"""
    return np.repeat(np.repeat(np.asarray(colours, np.uint8), 2, axis=0), 2, axis=1)


def _round_trip_worst(colours, matrix, rng):
    """colours [bh][bw][3] as uniform 2x2 blocks: forward by the output's definition (tests/yuv_ref.py), back by this one; the largest
    difference per channel"""
    img = _blocks_image(colours)
    h, w = img.shape[:2]
    back = ref.rgba(out_ref.frame(img, matrix, rng), w, h, matrix, rng, ref.NEAREST)
    assert (back[..., 3] == 255).all()
    return int(np.abs(back[..., :3].astype(int) - img).max())


def test_round_trip_of_all_colours():
    """all 2²⁴ uniform colours, BT.709 limited (the format with the wider bound)"""
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    worst = 0
    for r in range(256):
        worst = max(worst, _round_trip_worst(np.stack([np.full_like(g, r), g, b], axis=-1), ref.BT709, ref.LIMITED))
    assert worst <= ROUND_TRIP[ref.LIMITED], worst


@pytest.mark.parametrize("matrix,rng", ref.FORMATS[1:])
def test_round_trip_of_a_lattice(matrix, rng):
    """the other formats over the 16³ lattice {0, 17, …, 255}³, which holds the cube's corners"""
    v = np.arange(0, 256, 17)
    assert v[0] == 0 and v[-1] == 255
    r, g, b = np.meshgrid(v, v, v, indexing="ij")
    colours = np.stack([r, g, b], axis=-1).reshape(64, 64, 3)
    assert _round_trip_worst(colours, matrix, rng) <= ROUND_TRIP[rng]


@pytest.mark.parametrize("size", [(16, 8), (33, 17), (1, 1), (7, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_nearest_inverts_frames_of_uniform_blocks(size):
    """nearest on the output's frames of images made of uniform 2x2 blocks (odd sizes cut the last blocks) stays within the round-trip bound"""
    w, h = size
    rng_ = np.random.default_rng(w * 100 + h)
    img = _blocks_image(rng_.integers(0, 256, ((h + 1) // 2, (w + 1) // 2, 3)))[:h, :w]
    for matrix, rng in ref.FORMATS:
        back = ref.rgba(out_ref.frame(img, matrix, rng), w, h, matrix, rng, ref.NEAREST)
        assert np.abs(back[..., :3].astype(int) - img).max() <= ROUND_TRIP[rng]


@pytest.mark.parametrize("size", [(16, 8), (33, 17), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_bilinear_weights_sum_to_sixteen(size):
    """a frame of constant chroma: bilinear equals nearest"""
    w, h = size
    cw, ch, _ = ref.sizes(w, h)
    y = np.random.default_rng(7).integers(0, 256, (h, w))
    for u, v in ((128, 128), (0, 255), (240, 16), (77, 201)):
        frame = ref.pack(y, np.full((ch, cw), u), np.full((ch, cw), v))
        for fmt in ref.FORMATS:
            assert (ref.rgba(frame, w, h, *fmt, ref.BILINEAR) == ref.rgba(frame, w, h, *fmt, ref.NEAREST)).all()


def test_bilinear_corners_and_edges_by_hand():
    """4x4 pixels over the 2x2 chroma plane [[0, 64], [128, 255]], worked out from the definition:
      (0,0): both neighbours clamp onto the sample itself: 16·0
      (1,0): nx = 1, ny clamps to 0: 9·0 + 3·64 + 3·0 + 64 = 256          (3,0): nx clamps to 1: 12·64 + 4·64 = 1024
      (1,1): nx = 1, ny = 1: 9·0 + 3·64 + 3·128 + 255 = 831               (2,1): cx = 1, nx = 0, ny = 1: 9·64 + 3·0 + 3·255 + 128 = 1469
      (0,3): nx clamps to 0, ny clamps to 1: 16·128 = 2048                (3,3): 16·255 = 4080
      (0,1): nx clamps to 0, ny = 1: 12·0 + 4·128 = 512                   (2,3): cx = 1, nx = 0, cy = ny = 1: 12·255 + 4·128 = 3572"""
    plane = np.array([[0, 64], [128, 255]])
    s = ref.chroma16(plane, 4, 4, ref.BILINEAR)
    by_hand = {(0, 0): 0, (1, 0): 256, (3, 0): 1024, (1, 1): 831, (2, 1): 1469, (0, 3): 2048, (3, 3): 4080, (0, 1): 512, (2, 3): 3572}
    for (x, y), want in by_hand.items():
        assert s[y, x] == want, (x, y)
    assert (ref.chroma16(plane, 4, 4, ref.NEAREST) == 16 * np.repeat(np.repeat(plane, 2, axis=0), 2, axis=1)).all()
    # one pixel, BT.709 full, Y = 100, SU = 1469, SV = 831: l = 16·65536·100 = 104857600, u = −579, v = −1217
    #   R: 104857600 − 103206·1217 = −20744102 → + 2¹⁹ → floor(/2²⁰) = −20 → 0
    #   G: 104857600 + 12276·579 + 30679·1217 = 149301747 → 142          B: 104857600 − 121609·579 = 34445989 → 33
    assert ref.convert(np.array(100), np.array(1469), np.array(831), ref.BT709, ref.FULL).tolist() == [0, 142, 33, 255]
    # an odd size: the last column and row have one pixel per chroma sample, their outward neighbours clamp
    s = ref.chroma16(np.array([[10, 20], [30, 40]]), 3, 3, ref.BILINEAR)
    assert s[2, 2] == 9 * 40 + 3 * 20 + 3 * 30 + 10 and s[0, 2] == 12 * 20 + 4 * 10 and s[2, 0] == 12 * 30 + 4 * 10


def test_extremes_frame_holds_every_combination():
    w, h = 40, 10   # 20 x 5 = 100 blocks
    y, cb, cr = ref.split(ref.extremes_frame(w, h), w, h)
    seen = {(int(y[2 * j, 2 * i]), int(cb[j, i]), int(cr[j, i])) for j in range(5) for i in range(20)}
    assert seen == {(a, b, c) for a in (0, 16, 235, 255) for b in (0, 16, 128, 240, 255) for c in (0, 16, 128, 240, 255)}
    for fmt in ref.FORMATS:   # both clamps are hit
        img = ref.rgba(ref.extremes_frame(w, h), w, h, *fmt)
        assert img[..., :3].min() == 0 and img[..., :3].max() == 255


# ---- the Y4M reader ---------------------------------------------------------------------------------------------------------------------------

def _frames(w, h, n, seed=0):
    return np.random.default_rng(seed + w * 100 + h).integers(0, 256, (n, ref.sizes(w, h)[2]), dtype=np.uint8)


@pytest.mark.parametrize("w,h,n", [(16, 8, 3), (17, 9, 2), (1, 1, 4), (16, 8, 0)])
@pytest.mark.parametrize("full", [False, True])
def test_reader_round_trips_the_writer(native, tmp_path, w, h, n, full):
    frames = _frames(w, h, n)
    path = str(tmp_path / "v.y4m")
    native.write_y4m(path, frames, w, h, fps=(30000, 1001), full_range=full)
    info = native.read_y4m_info(path)
    assert info == dict(width=w, height=h, fps=(30000, 1001), frames=n, full_range=full, centre_sited=True, chroma="420jpeg")
    assert (native.read_y4m(path) == frames).all()
    for t in range(n):   # frame for frame
        assert (native.read_y4m(path, t, 1)[0] == frames[t]).all()
    with pytest.raises(ValueError, match="no frame"):
        native.read_y4m(path, n, 1)
    with pytest.raises(ValueError, match="no frame"):
        native.read_y4m(path, -1, 1)


def _write(path, header, frames, frame_line=b"FRAME\n"):
    with open(path, "wb") as f:
        f.write(header)
        for k, fr in enumerate(frames):
            f.write(frame_line if isinstance(frame_line, bytes) else frame_line[k])
            f.write(fr.tobytes())
    return str(path)


def test_reader_parses_reordered_and_extra_tokens(native, tmp_path):
    w, h = 6, 4
    frames = _frames(w, h, 3)
    path = _write(tmp_path / "a.y4m", b"YUV4MPEG2 XYSCSS=420JPEG C420mpeg2 A128:117 H4 XCOLORRANGE=FULL Ip F25:1 W6 XFOO\n", frames)
    assert native.read_y4m_info(path) == dict(width=6, height=4, fps=(25, 1), frames=3, full_range=True, centre_sited=False, chroma="420mpeg2")
    assert (native.read_y4m(path) == frames).all()
    # nothing but the size: Y4M's defaults
    path = _write(tmp_path / "b.y4m", b"YUV4MPEG2 W6 H4\n", frames)
    assert native.read_y4m_info(path) == dict(width=6, height=4, fps=(0, 0), frames=3, full_range=None, centre_sited=True, chroma="420jpeg")
    for tag, centre in (("420paldv", False), ("420", False), ("420jpeg", True)):
        path = _write(tmp_path / "c.y4m", f"YUV4MPEG2 W6 H4 F30:1 I? C{tag}\n".encode(), frames)
        info = native.read_y4m_info(path)
        assert (info["chroma"], info["centre_sited"], info["frames"]) == (tag, centre, 3)


def test_reader_walks_frame_lines_with_parameters(native, tmp_path):
    w, h = 6, 4
    frames = _frames(w, h, 3)
    lines = [b"FRAME Ip\n", b"FRAME\n", b"FRAME XLONGER=1 Ip\n"]
    path = _write(tmp_path / "p.y4m", b"YUV4MPEG2 W6 H4 F30:1\n", frames, lines)
    assert native.read_y4m_info(path)["frames"] == 3
    assert (native.read_y4m(path) == frames).all() and (native.read_y4m(path, 2, 1)[0] == frames[2]).all()
    # parameters on a later line only: the size is no whole number of plain frames, so the lines are walked
    path = _write(tmp_path / "q.y4m", b"YUV4MPEG2 W6 H4 F30:1\n", frames, [b"FRAME\n", b"FRAME Ip\n", b"FRAME\n"])
    assert (native.read_y4m(path) == frames).all()


@pytest.mark.parametrize("header,word", [
    (b"YUV4MPEG2 W6 H4 C422\n", "4:2:0"),
    (b"YUV4MPEG2 W6 H4 C444\n", "4:2:0"),
    (b"YUV4MPEG2 W6 H4 C420p10\n", "4:2:0"),
    (b"YUV4MPEG2 W6 H4 Cmono\n", "4:2:0"),
    (b"YUV4MPEG2 W6 H4 C411\n", "4:2:0"),
    (b"YUV4MPEG2 W6 H4 It\n", "interlaced"),
    (b"YUV4MPEG2 W6 H4 Ib\n", "interlaced"),
    (b"YUV4MPEG2 W6 H4 Im\n", "interlaced"),
    (b"YUV4MPEG2 W0 H4\n", "size"),
    (b"YUV4MPEG2 W6 H0\n", "size"),
    (b"YUV4MPEG2 H4\n", "size"),
    (b"YUV4MPEG2 W-6 H4\n", "width"),
    (b"YUV4MPEG2 W6 H4 F30\n", "frame rate"),
    (b"YUV4MPEG W6 H4\n", "not a YUV4MPEG2"),
    (b"RIFF....AVI \n", "not a YUV4MPEG2"),
])
def test_reader_refuses(native, tmp_path, header, word):
    path = _write(tmp_path / "bad.y4m", header, _frames(6, 4, 2))
    with pytest.raises(ValueError, match=word):
        native.read_y4m_info(path)
    with pytest.raises(ValueError, match=word):
        native.read_y4m(path, 0, 1)


def test_reader_refuses_a_truncated_last_frame(native, tmp_path):
    frames = _frames(6, 4, 3)
    good = open(_write(tmp_path / "good.y4m", b"YUV4MPEG2 W6 H4 F30:1\n", frames), "rb").read()
    for cut in (1, 5, 36, 37):   # inside the last frame's bytes, and inside its FRAME line
        (tmp_path / "cut.y4m").write_bytes(good[:-cut])
        with pytest.raises(ValueError, match="truncated|FRAME|header line"):
            native.read_y4m_info(str(tmp_path / "cut.y4m"))
    (tmp_path / "cut.y4m").write_bytes(good[:-(6 + 36)])   # a whole frame less is a shorter video
    assert native.read_y4m_info(str(tmp_path / "cut.y4m"))["frames"] == 2
    with pytest.raises(ValueError, match="Cannot read"):
        native.read_y4m_info(str(tmp_path / "missing.y4m"))
    (tmp_path / "junk.y4m").write_bytes(good[:22] + b"JUNK!\n" + good[28:])
    with pytest.raises(ValueError, match="FRAME"):
        native.read_y4m_info(str(tmp_path / "junk.y4m"))


# ---- the loader of light-field videos -----------------------------------------------------------------------------------------------------------

def _video_dir(native, d, cols, rows, w, h, n, name=lambda r, c: f"{r}_{c}.y4m", full=False):
    """rows x cols cameras of n frames; returns {(col, row): [n][frame_bytes]}"""
    d.mkdir()
    cams = {}
    for c in range(cols):
        for r in range(rows):
            cams[(c, r)] = _frames(w, h, n, seed=1000 * c + 10 * r)
            native.write_y4m(str(d / name(r, c)), cams[(c, r)], w, h, full_range=full)
    return cams


def test_loader_reads_a_grid_of_videos(native, tmp_path):
    cols, rows, w, h, n = 3, 2, 6, 4, 3
    # unpadded and padded names side by side
    cams = _video_dir(native, tmp_path / "lf", cols, rows, w, h, n, name=lambda r, c: f"{r:02d}_{c}.y4m" if c == 1 else f"{r}_{c}.y4m", full=True)
    for t in range(n):
        got = native.load_grid_y4m(str(tmp_path / "lf"), t)
        assert got[:6] == (cols, rows, w, h, n, True)
        for (c, r), frames in cams.items():
            assert (got[6][c * rows + r] == frames[t]).all(), (t, c, r)   # image id = col*rows + row
    with pytest.raises(RuntimeError, match="no frame 3"):
        native.load_grid_y4m(str(tmp_path / "lf"), n)
    # an image directory is not a video, and image directories load as before
    (tmp_path / "img").mkdir()
    native.write_png(str(tmp_path / "img" / "0_0.png"), np.full((4, 6, 4), 255, np.uint8))
    with pytest.raises(RuntimeError, match="images"):
        native.load_grid_y4m(str(tmp_path / "img"))
    assert native.load_grid(str(tmp_path / "img"))[:2] == (1, 1)


def test_loader_takes_the_shortest_video(native, tmp_path):
    cams = _video_dir(native, tmp_path / "lf", 2, 2, 6, 4, 3)
    native.write_y4m(str(tmp_path / "lf" / "1_0.y4m"), cams[(0, 1)][:2], 6, 4)
    got = native.load_grid_y4m(str(tmp_path / "lf"), 1)
    assert got[4] == 2 and (got[6][1] == cams[(0, 1)][1]).all()
    with pytest.raises(RuntimeError, match="no frame 2"):
        native.load_grid_y4m(str(tmp_path / "lf"), 2)


def test_loader_refuses(native, tmp_path):
    _video_dir(native, tmp_path / "missing", 2, 2, 6, 4, 2)
    os.remove(tmp_path / "missing" / "1_0.y4m")
    with pytest.raises(RuntimeError, match="1_0 is missing"):
        native.load_grid_y4m(str(tmp_path / "missing"))
    cams = _video_dir(native, tmp_path / "sizes", 2, 2, 6, 4, 2)
    native.write_y4m(str(tmp_path / "sizes" / "0_1.y4m"), _frames(8, 4, 2), 8, 4)
    with pytest.raises(RuntimeError, match="same resolution"):
        native.load_grid_y4m(str(tmp_path / "sizes"))
    _video_dir(native, tmp_path / "ranges", 2, 2, 6, 4, 2)
    native.write_y4m(str(tmp_path / "ranges" / "0_1.y4m"), cams[(1, 0)], 6, 4, full_range=True)
    with pytest.raises(RuntimeError, match="XCOLORRANGE"):
        native.load_grid_y4m(str(tmp_path / "ranges"))
    _video_dir(native, tmp_path / "mixed", 2, 2, 6, 4, 2)
    os.remove(tmp_path / "mixed" / "1_1.y4m")
    native.write_png(str(tmp_path / "mixed" / "1_1.png"), np.full((4, 6, 4), 255, np.uint8))
    for load in (native.load_grid_y4m, native.load_grid):
        with pytest.raises(RuntimeError, match="mixes"):
            load(str(tmp_path / "mixed"))
    _video_dir(native, tmp_path / "bad", 1, 1, 6, 4, 2)
    (tmp_path / "bad" / "0_0.y4m").write_bytes(b"YUV4MPEG2 W6 H4 C444\n")
    with pytest.raises(RuntimeError, match="4:2:0"):
        native.load_grid_y4m(str(tmp_path / "bad"))


# ---- the library and the command line -----------------------------------------------------------------------------------------------------

def test_symbols_are_exported_and_bound(native):
    lib = native.load_hip_library()
    assert "lfi_upload_images_yuv420" in native.ABI_SYMBOLS and hasattr(lib, "lfi_upload_images_yuv420")
    host = native.load_host_library()
    for name in ("lfi_host_y4m_info", "lfi_host_y4m_read", "lfi_host_load_grid_y4m"):
        assert hasattr(host, name)
    assert hasattr(native.Context, "upload_images_yuv420")
    assert (native.LFI_CHROMA_BILINEAR, native.LFI_CHROMA_NEAREST) == (ref.BILINEAR, ref.NEAREST) == (0, 1)
    assert lib.lfi_abi_version() == 1


IN_ARGS = ["-t", "0,0,1,1", "-m", "STD", "-n", "4", "-b", "1", "-f", "0.0"]


@pytest.mark.parametrize("extra,words", [
    (["--frames", "0:2", "--compare-methods"], ("--frames", "--compare-methods")),
    (["--frames", "0:2", "--compare", "dir"], ("--frames", "--compare")),
    (["--frames", "0:2", "-g", "2"], ("--frames", "-g")),
    (["--frames", "1:0"], ("--frames", "FIRST", "COUNT")),
    (["--frames", "a"], ("--frames", "FIRST")),
    (["--frames", "1:"], ("--frames", "FIRST")),
    (["--frames", "-1"], ("--frames", "FIRST")),
    (["--frames"], ("--frames", "FIRST")),
    (["--in-matrix", "2020"], ("--in-matrix", "709", "601")),
    (["--in-range", "tv"], ("--in-range", "limited", "full")),
    (["--in-chroma", "bicubic"], ("--in-chroma", "bilinear", "nearest")),
])
def test_cli_refuses_before_anything_runs(native, tmp_path, extra, words):
    (tmp_path / "lf").mkdir()
    res = run_cli(native, "-i", str(tmp_path / "lf"), *IN_ARGS, "-o", str(tmp_path / "out"), *extra)
    assert res.returncode != 0
    for word in words:
        assert word in res.stderr, res.stderr
    assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("flag", [["--frames", "0"], ["--in-matrix", "601"], ["--in-range", "full"], ["--in-chroma", "nearest"]])
def test_cli_refuses_video_flags_without_a_video(native, tmp_path, flag):
    res = run_cli(native, "--synthetic", "3,3,16,8", *IN_ARGS, "-o", str(tmp_path / "out"), *flag)
    assert res.returncode != 0 and ".y4m" in res.stderr and flag[0] in res.stderr, res.stderr
    assert not (tmp_path / "out").exists()


def test_cli_help_names_the_flags(native):
    res = run_cli(native, "-h")
    assert res.returncode == 0
    for flag in ("--frames FIRST[:COUNT]", "--in-matrix 709|601", "--in-range limited|full", "--in-chroma bilinear|nearest"):
        assert flag in res.stdout


# ---- the code object --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not code_object.have_tools(), reason="ROCm LLVM tools not installed")
def test_yuv420_expand_uses_no_scratch_no_spills_and_no_lds(native):
    """From the code object's notes: both I420 instantiations of yuvs_expand (csrc/hip/yuv_surfaces.hpp), the kernel behind
    lfi_upload_images_yuv420, exist, use no scratch and no LDS and spill nothing; from its code: no atomics, no byte or short stores — a lane's two runs of 32 bytes leave as four 16-byte stores (ragged
    blocks: dwords) — Y arrives as two 8-byte loads, chroma as dwords: one per plane (nearest), nine per plane (bilinear)."""
    kernels = code_object.kernels(native.build.HIP_LIB)
    expand = {k: v for k, v in code_object.named(kernels, "yuvs_expand").items() if "yuvs_expandILi0E" in k}   # <YUVS_I420, NEAREST>
    assert len(expand) == 2, sorted(expand)
    for k, v in expand.items():
        assert v[".private_segment_fixed_size"] == 0 and v[".vgpr_spill_count"] == 0 and v[".sgpr_spill_count"] == 0, (k, v)
        assert v[".group_segment_fixed_size"] == 0 and v[".vgpr_count"] <= 128, (k, v)   # at least four waves per SIMD
    bodies = {k: v for k, v in code_object.bodies(native.build.HIP_LIB).items() if k in expand}
    assert set(bodies) == set(expand)
    for k, text in bodies.items():
        assert "atomic" not in text and "scratch_" not in text and "ds_" not in text, k
        assert "global_store_byte" not in text and "global_store_short" not in text, k
        # the channels are clamped before their shift: clamp(v >> 20, 0, 255) compiled to v_ashr_pk_u8_i32 for two channels with the third
        # ORed beside it, and on the MI355X the blue channel came out with stray bits (csrc/hip/yuv420_upload.hpp, yuv_in_clamp)
        assert "v_ashr_pk_u8_i32" not in text, k
        assert text.count("global_store_dwordx4") == 4 and len(re.findall(r"global_store_dword ", text)) == 16, k
        assert text.count("global_load_dwordx2") == 2 and "global_load_ubyte" not in text, k
        assert len(re.findall(r"global_load_dword ", text)) == (2 if "ELb1E" in k else 18), k   # NEAREST / bilinear
