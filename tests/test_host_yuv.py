"""CPU: the host side of the YUV 4:2:0 video output (lfi_download_views_yuv420, lfi_render_stream_yuv420, --y4m) — the coefficient table against
its derivation from the matrix constants, the properties include/lfi.h states about it, the numpy restatement (tests/yuv_ref.py) on hand-made
cases, the Y4M writer (csrc/host/y4m.cpp through lfi_host_y4m_write) through a small parser, the exported symbols, the CLI's usage errors and
the new kernel's code object."""
import math
import os
import re

import numpy as np
import pytest

import code_object
import yuv_ref as ref
from view_rows import run_cli

# (Kr, Kb) of Y = Kr·R + (1 − Kr − Kb)·G + Kb·B:  ITU-R BT.709 / BT.601
LUMA = {ref.BT709: (0.2126, 0.0722), ref.BT601: (0.299, 0.114)}


def _round(x):
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


# ---- the table ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("matrix,rng", ref.FORMATS)
def test_table_is_derived_from_the_matrix_constants(matrix, rng):
    """each entry round(c · scale · 2¹⁶); G then adjusted for the row sums"""
    kr, kb = LUMA[matrix]
    kg = 1.0 - kr - kb
    ys, cs = (219.0 / 255.0, 224.0 / 255.0) if rng == ref.LIMITED else (1.0, 1.0)
    y_sum = 56284 if rng == ref.LIMITED else 65536
    assert y_sum == _round(ys * 65536)
    y_r, y_b = _round(kr * ys * 65536), _round(kb * ys * 65536)
    half = _round(0.5 * cs * 65536)
    cb_r = _round(-kr / (2 * (1 - kb)) * cs * 65536)
    cr_b = _round(-kb / (2 * (1 - kr)) * cs * 65536)
    want = ((y_r, y_sum - y_r - y_b, y_b), (cb_r, -(cb_r + half), half), (half, -(half + cr_b), cr_b), 16 if rng == ref.LIMITED else 0)
    assert ref.TABLE[(matrix, rng)] == want
    # the adjusted G is the rounded one, or its neighbour
    ky, kcb, kcr, _ = ref.TABLE[(matrix, rng)]
    assert abs(ky[1] - kg * ys * 65536) < 1.5
    assert abs(kcb[1] + kg / (2 * (1 - kb)) * cs * 65536) < 1.5 and abs(kcr[1] + kg / (2 * (1 - kr)) * cs * 65536) < 1.5


@pytest.mark.parametrize("matrix,rng", ref.FORMATS)
def test_row_sums(matrix, rng):
    ky, kcb, kcr, y_off = ref.TABLE[(matrix, rng)]
    assert sum(ky) == (56284 if rng == ref.LIMITED else 65536) and sum(kcb) == 0 and sum(kcr) == 0
    assert y_off == (16 if rng == ref.LIMITED else 0)


def test_header_and_kernel_carry_the_table():
    """the literals of include/lfi.h's comment and of csrc/hip/yuv420.hpp's one table are those of the restatement"""
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "lfi.h")).read()
    kernel = open(os.path.join(ROOT, "lfinterpolator_amd", "csrc", "hip", "yuv420.hpp")).read()
    table = kernel[kernel.index("constexpr YuvCoeffs YUV_COEFFS[4]"):]
    table = table[:table.index("};")]
    rows = re.findall(r"\{\{(-?\d+), (-?\d+), (-?\d+)\}, \{(-?\d+), (-?\d+), (-?\d+)\}, \{(-?\d+), (-?\d+), (-?\d+)\}, (\d+)\}", table)
    assert len(rows) == 4
    for (matrix, rng), row in zip(ref.FORMATS, rows):   # row = matrix·2 + range
        ky, kcb, kcr, y_off = ref.TABLE[(matrix, rng)]
        assert tuple(int(v) for v in row) == ky + kcb + kcr + (y_off,)
        name = ("709" if matrix == ref.BT709 else "601") + (" limited" if rng == ref.LIMITED else " full")
        line = next(ln for ln in header.splitlines() if re.match(r"\*\s+" + name + r"\s", ln.strip()))
        assert [int(v) for v in re.findall(r"-?\d+", line.split(name, 1)[1])] == list(ky + kcb + kcr + (y_off,))
    for text in ("LFI_YUV_BT709 = 0", "LFI_YUV_BT601 = 1", "LFI_YUV_LIMITED = 0", "LFI_YUV_FULL = 1"):
        assert text in header


# ---- the restatement's properties --------------------------------------------------------------------------------------------------------------

SAMPLE = ref.corner_views(128, 66, 3)


def test_sample_holds_every_arrangement_every_corner_and_every_grey():
    blocks = SAMPLE.reshape(3, 33, 2, 64, 2, 4)[..., :3].transpose(0, 1, 3, 2, 4, 5).reshape(-1, 4, 3)   # [block][pixel of the block][rgb]
    corner = (blocks[..., 0] // 255) + 2 * (blocks[..., 1] // 255) + 4 * (blocks[..., 2] // 255)         # of corner pixels
    is_corner = ((blocks == 0) | (blocks == 255)).all(axis=(1, 2))
    codes = (corner[is_corner] * np.array([1, 8, 64, 512])).sum(axis=1)
    assert len(np.unique(codes)) == 4096                                                                    # every 2x2 arrangement of the 8 corners
    uniform = (blocks == blocks[:, :1]).all(axis=(1, 2))
    greys = blocks[uniform & (blocks[:, 0, 0] == blocks[:, 0, 1]) & (blocks[:, 0, 1] == blocks[:, 0, 2])][:, 0, 0]
    assert len(np.unique(greys)) == 256
    assert len(np.unique(corner[uniform & is_corner][:, 0])) == 8


@pytest.mark.parametrize("matrix,rng", ref.FORMATS)
def test_extremes(matrix, rng):
    """limited range: Y in [16, 235], chroma in [16, 240], all four reached; full range: Y in [0, 255] and chroma reaches 256 before the clamp,
    255 after it; every grey has chroma exactly 128; white is 235 / 255"""
    ys, cbs, crs = zip(*[ref.planes(v, matrix, rng, clamp=False) for v in SAMPLE])
    y, cb, cr = np.stack(ys), np.stack(cbs), np.stack(crs)
    if rng == ref.LIMITED:
        assert (y.min(), y.max()) == (16, 235)
        assert (cb.min(), cb.max()) == (16, 240) and (cr.min(), cr.max()) == (16, 240)
    else:
        assert (y.min(), y.max()) == (0, 255)
        assert cb.max() == 256 and cr.max() == 256 and cb.min() >= 0 and cr.min() >= 0
        clamped = np.stack([ref.planes(v, matrix, rng)[1] for v in SAMPLE])
        assert clamped.max() == 255 and (clamped[cb == 256] == 255).all()
    for level in range(256):
        grey = np.full((2, 2, 4), level, np.uint8)
        gy, gcb, gcr = ref.planes(grey, matrix, rng)
        assert gcb[0, 0] == 128 and gcr[0, 0] == 128
        if rng == ref.FULL:
            assert (gy == level).all()
    white = ref.planes(np.full((2, 2, 4), 255, np.uint8), matrix, rng)[0]
    assert (white == (235 if rng == ref.LIMITED else 255)).all()


def test_frame_by_hand():
    """3 x 3, BT.601 full: the planes' sizes, the replicated last column and row, one value of each plane from the formula"""
    img = np.zeros((3, 3, 4), np.uint8)
    img[..., 3] = 255
    img[0, 0, :3] = (255, 0, 0)
    img[2, 2, :3] = (0, 0, 255)
    assert ref.sizes(3, 3) == (2, 2, 9 + 8)
    f = ref.frame(img, ref.BT601, ref.FULL)
    assert f.shape == (17,)
    y, cb, cr = f[:9].reshape(3, 3), f[9:13].reshape(2, 2), f[13:].reshape(2, 2)
    assert y[0, 0] == (19595 * 255 + 32768) >> 16 and y[2, 2] == (7471 * 255 + 32768) >> 16 and y[1, 1] == 0
    assert cr[0, 0] == ((1 << 25) + (1 << 17) + 32768 * 255) >> 18       # one red pixel of four
    assert cb[1, 1] == min(255, ((1 << 25) + (1 << 17) + 32768 * 4 * 255) >> 18) == 255   # the blue corner, replicated to all four: 256 clamped
    assert cr[1, 1] == ((1 << 25) + (1 << 17) - 5329 * 4 * 255) >> 18
    assert cb[0, 1] == 128 and cb[1, 0] == 128


# ---- the Y4M writer --------------------------------------------------------------------------------------------------------------------------

def parse_y4m(data):
    """(header fields, [frames]) of a Y4M file's bytes"""
    head, rest = data.split(b"\n", 1)
    fields = head.decode().split(" ")
    assert fields[0] == "YUV4MPEG2"
    tags = {f[0]: f[1:] for f in fields[1:] if not f.startswith("X")}
    tags["X"] = [f[1:] for f in fields[1:] if f.startswith("X")]
    size = ref.sizes(int(tags["W"]), int(tags["H"]))[2]
    frames = []
    while rest:
        assert rest[:6] == b"FRAME\n" and len(rest) >= 6 + size
        frames.append(np.frombuffer(rest[6:6 + size], np.uint8))
        rest = rest[6 + size:]
    return tags, frames


@pytest.mark.parametrize("w,h,n", [(16, 8, 3), (17, 9, 2), (7, 3, 4), (1, 1, 5), (24, 6, 0)])
@pytest.mark.parametrize("full", [False, True])
def test_y4m_round_trip(native, tmp_path, w, h, n, full):
    size = ref.sizes(w, h)[2]
    frames = np.random.default_rng(w * 100 + h).integers(0, 256, (n, size + 5), dtype=np.uint8)   # a frame stride above the frame's bytes
    path = tmp_path / "v.y4m"
    native.write_y4m(str(path), frames, w, h, fps=(30000, 1001), full_range=full)
    data = path.read_bytes()
    assert data.startswith(f"YUV4MPEG2 W{w} H{h} F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE={'FULL' if full else 'LIMITED'}\n".encode())
    tags, got = parse_y4m(data)
    assert (tags["W"], tags["H"], tags["F"], tags["I"], tags["A"], tags["C"]) == (str(w), str(h), "30000:1001", "p", "1:1", "420jpeg")
    assert tags["X"] == ["COLORRANGE=" + ("FULL" if full else "LIMITED")]
    assert len(got) == n and all((g == frames[k, :size]).all() for k, g in enumerate(got))
    assert len(data) == len(data.split(b"\n", 1)[0]) + 1 + n * (6 + size)
    # the default rate, tight frames
    native.write_y4m(str(path), np.ascontiguousarray(frames[:, :size]), w, h)
    assert path.read_bytes().startswith(f"YUV4MPEG2 W{w} H{h} F30:1 ".encode())


def test_y4m_refusals(native, tmp_path):
    path = tmp_path / "v.y4m"
    frames = np.zeros((2, 16 * 8 * 3 // 2), np.uint8)
    for bad in (lambda: native.write_y4m(str(path), frames[:, :-1], 16, 8), lambda: native.write_y4m(str(path), frames, 0, 8),
                lambda: native.write_y4m(str(path), frames, 16, 8, fps=(0, 1)), lambda: native.write_y4m(str(path), frames, 16, 8, fps=(30, 0)),
                lambda: native.write_y4m(str(path), frames.astype(np.uint16), 16, 8),
                lambda: native.write_y4m(str(tmp_path / "missing" / "v.y4m"), frames, 16, 8)):
        with pytest.raises(ValueError):
            bad()
    assert not path.exists()


# ---- the library and the command line -----------------------------------------------------------------------------------------------------

def test_symbols_are_exported_and_bound(native):
    lib = native.load_hip_library()
    for name in ("lfi_download_views_yuv420", "lfi_render_stream_yuv420"):
        assert name in native.ABI_SYMBOLS and hasattr(lib, name)
    host = native.load_host_library()
    assert hasattr(host, "lfi_host_y4m_write") and hasattr(host, "lfi_host_y4m_frame_bytes")
    assert hasattr(native.Context, "download_views_yuv420") and hasattr(native.Context, "render_stream_yuv420")
    assert (native.LFI_YUV_BT709, native.LFI_YUV_BT601, native.LFI_YUV_LIMITED, native.LFI_YUV_FULL) == (ref.BT709, ref.BT601, ref.LIMITED, ref.FULL)
    for w, h in ((16, 8), (17, 9), (1, 1), (3840, 2160)):
        assert host.lfi_host_y4m_frame_bytes(w, h) == ref.sizes(w, h)[2]


Y4M_ARGS = ["--synthetic", "4,4,32,16", "-t", "0,0,1,1", "-m", "STD", "-n", "6", "-b", "1", "-f", "0.0"]


@pytest.mark.parametrize("extra,words", [
    (["--fps", "25"], ("--fps", "--y4m")),
    (["--yuv-matrix", "601"], ("--yuv-matrix", "--y4m")),
    (["--yuv-range", "full"], ("--yuv-range", "--y4m")),
    (["--y4m"], ("--y4m", "file")),
    (["--y4m", "v.y4m", "--fps", "0"], ("--fps", "N:D")),
    (["--y4m", "v.y4m", "--fps", "30:"], ("--fps", "N:D")),
    (["--y4m", "v.y4m", "--fps", "30:0"], ("--fps", "N:D")),
    (["--y4m", "v.y4m", "--fps", "29.97"], ("--fps", "N:D")),
    (["--y4m", "v.y4m", "--fps", "30:1:1"], ("--fps", "N:D")),
    (["--y4m", "v.y4m", "--fps"], ("--fps", "N:D")),
    (["--y4m", "v.y4m", "--yuv-matrix", "2020"], ("--yuv-matrix", "709", "601")),
    (["--y4m", "v.y4m", "--yuv-matrix"], ("--yuv-matrix", "709", "601")),
    (["--y4m", "v.y4m", "--yuv-range", "tv"], ("--yuv-range", "limited", "full")),
    (["--y4m", "v.y4m", "--yuv-range", "Full"], ("--yuv-range", "limited", "full")),
])
def test_cli_refuses_before_anything_runs(native, tmp_path, extra, words):
    extra = [str(tmp_path / e) if e == "v.y4m" else e for e in extra]
    res = run_cli(native, *Y4M_ARGS, "-o", str(tmp_path / "out"), *extra)
    assert res.returncode != 0
    for word in words:
        assert word in res.stderr, res.stderr
    assert not (tmp_path / "out").exists() and not (tmp_path / "v.y4m").exists()


def test_cli_help_names_the_flags(native):
    res = run_cli(native, "-h")
    assert res.returncode == 0
    for flag in ("--y4m FILE", "--fps N[:D]", "--yuv-matrix 709|601", "--yuv-range limited|full"):
        assert flag in res.stdout


# ---- the code object --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not code_object.have_tools(), reason="ROCm LLVM tools not installed")
def test_yuv420_convert_uses_no_scratch_no_spills_and_no_lds(native):
    """From the code object's notes: both I420 instantiations of yuvs_convert (csrc/hip/yuv_surfaces.hpp), the kernel behind
    lfi_download_views_yuv420 and lfi_render_stream_yuv420, exist, use no scratch and no LDS and spill nothing; from its code: no atomics, no
    short stores — Y leaves as 8-byte pieces, chroma as dwords — and the aligned RGBA path reads 16 bytes per load, the planar path 8.

    The kernel took over from one of these calls' own that wrote every byte of padded planes and so had no byte stores at all, which this test
    asserted.  yuvs_convert also writes the caller's surfaces in place, where pitch padding must keep its value: a ragged last block of a row
    stores its own bytes one by one.  The assertion is now the exact count of those: at most 7 Y columns × 2 rows + 3 chroma columns × 2
    planes = 20 byte stores, and every whole block still leaves as words."""
    kernels = code_object.kernels(native.build.HIP_LIB)
    convert = {k: v for k, v in kernels.items() if re.search(r"yuvs_convertILb[01]ELi0E", k)}   # <PLANAR, YUVS_I420>
    assert len(convert) == 2, sorted(convert)
    for k, v in convert.items():
        assert v[".private_segment_fixed_size"] == 0 and v[".vgpr_spill_count"] == 0 and v[".sgpr_spill_count"] == 0, (k, v)
        assert v[".group_segment_fixed_size"] == 0 and v[".vgpr_count"] <= 128, (k, v)   # at least four waves per SIMD
    bodies = {k: v for k, v in code_object.bodies(native.build.HIP_LIB).items() if k in convert}
    assert set(bodies) == set(convert)
    for k, text in bodies.items():
        assert "atomic" not in text and "scratch_" not in text and "ds_" not in text, k
        assert "global_store_short" not in text and text.count("global_store_byte") == 20, k
        assert text.count("global_store_dwordx2") == 2 and len(re.findall(r"global_store_dword ", text)) == 2, k
        if "ILb1E" in k:   # PLANAR
            assert text.count("global_load_dwordx2") == 6 and "global_load_ubyte" not in text, k
        else:
            assert text.count("global_load_dwordx4") == 4, k
