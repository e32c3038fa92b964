"""CPU: the host side of RGB-D video frames (lfi_download_rgbd_yuv) — the symbol declared, exported and bound; what the header states about the
depth half of the restatement (tests/rgbd_yuv_ref.py): constant chroma, the one-multiply luma, inversion before the resize; the CLI's checks of
--rgbd-y4m; the code object's records of the kernel (csrc/hip/rgbd_yuv.hpp)."""
import os
import re

import numpy as np
import pytest

import code_object
import rgbd_yuv_ref as ref
import scaled_quilt_ref
import yuv_ref
from view_rows import run_cli

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "lfi.h")
TILES = [(18, 10), (16, 8), (50, 22), (2, 2)]
W, H = 50, 22


def test_symbol_is_declared_exported_and_bound(native):
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", text)
    assert ("int lfi_download_rgbd_yuv(lfi_ctx *ctx, int v0, int n, int map_k, uint32_t flags, int tile_w, int tile_h, int matrix, int range, "
            "const lfi_yuv_surfaces *dst);") in flat
    assert "enum { LFI_RGBD_INVERT = 1u, LFI_RGBD_VIEW_MAPS = 2u };" in flat
    assert "#define LFI_ABI_VERSION 1" in text   # the header has only grown
    lib = native.load_hip_library()
    assert "lfi_download_rgbd_yuv" in native.ABI_SYMBOLS and hasattr(lib, "lfi_download_rgbd_yuv")
    assert lib.lfi_download_rgbd_yuv.argtypes is not None and len(lib.lfi_download_rgbd_yuv.argtypes) == 10
    assert hasattr(native.Context, "download_rgbd_yuv")
    assert (native.LFI_RGBD_INVERT, native.LFI_RGBD_VIEW_MAPS) == (1, 2)


def _inputs(seed):
    rng = np.random.default_rng(seed)
    view = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    view[..., 3] = 255
    depth = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)   # G, B and A differ from R: the depth is the R byte
    return view, depth


def _halves(frame, tw, th):
    """(Y [th][2tw], Cb [th/2][tw], Cr [th/2][tw]) of a tight I420 frame of 2tw x th"""
    y = frame[:2 * tw * th].reshape(th, 2 * tw)
    cb = frame[2 * tw * th:2 * tw * th + tw * th // 2].reshape(th // 2, tw)
    cr = frame[2 * tw * th + tw * th // 2:].reshape(th // 2, tw)
    return y, cb, cr


@pytest.mark.parametrize("invert", [False, True], ids=["as-is", "inverted"])
@pytest.mark.parametrize("tile", TILES, ids=lambda t: f"{t[0]}x{t[1]}")
def test_the_depth_half_is_one_multiply_and_constant_chroma(tile, invert):
    """what include/lfi.h states as consequences of the coefficient tables, for the four sets: the depth half's chroma is all 128, its luma is
    y_off + ((S*s + 2^15) >> 16) of s, the rounded area mean of d; the colour half is the view's own frame"""
    tw, th = tile
    view, depth = _inputs(tw * 100 + th)
    d = depth[..., 0].astype(np.int64)
    d = 255 - d if invert else d
    s = scaled_quilt_ref.resize(np.repeat(d.astype(np.uint8)[..., None], 4, axis=2), tw, th)[..., 0].astype(np.int64)
    for matrix, rng in yuv_ref.FORMATS:
        got = ref.frame(view, depth, tw, th, invert, matrix, rng)
        assert got.shape == (yuv_ref.sizes(2 * tw, th)[2],)
        y, cb, cr = _halves(got, tw, th)
        assert (cb[:, tw // 2:] == 128).all() and (cr[:, tw // 2:] == 128).all(), (matrix, rng)
        S, y_off = (56284, 16) if rng == yuv_ref.LIMITED else (65536, 0)
        assert sum(yuv_ref.TABLE[(matrix, rng)][0]) == S
        assert (y[:, tw:] == y_off + ((S * s + (1 << 15)) >> 16)).all(), (matrix, rng)
        if rng == yuv_ref.FULL:
            assert (y[:, tw:] == s).all()
        alone = yuv_ref.frame(scaled_quilt_ref.resize(view, tw, th), matrix, rng)
        ya, cba, cra = alone[:tw * th].reshape(th, tw), alone[tw * th:tw * th + tw * th // 4], alone[tw * th + tw * th // 4:]
        assert (y[:, :tw] == ya).all() and (cb[:, :tw // 2].reshape(-1) == cba).all() and (cr[:, :tw // 2].reshape(-1) == cra).all()


def test_inversion_before_the_resize_is_not_inversion_after_it():
    """a 4 x 4 map as a tile of 2 x 2: every output is the mean of a 2 x 2 block.  Bytes {0, 0, 1, 1} have the mean 0.5, a tie, which rounds
    up to 1; inverted first they are {255, 255, 254, 254}, mean 254.5, which rounds up to 255 — and 255 - 1 is 254"""
    depth = np.zeros((4, 4, 4), np.uint8)
    depth[0:2, 0:2, 0] = [[0, 0], [1, 1]]
    depth[2:4, 2:4, 0] = [[7, 8], [8, 7]]      # mean 7.5 -> 8; inverted 247.5 -> 248, not 247
    view = np.full((4, 4, 4), 255, np.uint8)
    conv = (yuv_ref.BT709, yuv_ref.FULL)        # full range: Y = s
    plain = _halves(ref.frame(view, depth, 2, 2, False, *conv), 2, 2)[0][:, 2:]
    inverted = _halves(ref.frame(view, depth, 2, 2, True, *conv), 2, 2)[0][:, 2:]
    assert plain.tolist() == [[1, 0], [0, 8]]
    assert inverted.tolist() == [[255, 255], [255, 248]]
    assert (inverted != 255 - plain.astype(int)).sum() == 2


# ---- the command line -----------------------------------------------------------------------------------------------------------------

RUN_ARGS = ["--synthetic", "4,4,32,16", "-t", "0,0,1,1", "-m", "STD", "-n", "6", "-b", "1", "-f", "0.0"]
ALL_FOCUS = ["-r", "0.5"]


def _refused(native, tmp_path, args, *words):
    res = run_cli(native, *RUN_ARGS, "-o", str(tmp_path / "out"), *args)
    assert res.returncode != 0, res.stdout
    for word in words:
        assert word in res.stderr, (word, res.stderr)
    assert not (tmp_path / "out").exists() and not (tmp_path / "rgbd.y4m").exists()


def test_cli_refuses_rgbd_without_a_focus_map(native, tmp_path):
    _refused(native, tmp_path, ["--rgbd-y4m", str(tmp_path / "rgbd.y4m")], "--rgbd-y4m", "-r")


def test_cli_refuses_an_empty_file_name(native, tmp_path):
    _refused(native, tmp_path, [*ALL_FOCUS, "--rgbd-y4m", ""], "--rgbd-y4m", "name")


@pytest.mark.parametrize("tile", ["17x8", "16x7", "0x8", "16", "ax8"])
def test_cli_refuses_odd_and_malformed_tile_sizes(native, tmp_path, tile):
    _refused(native, tmp_path, [*ALL_FOCUS, "--rgbd-y4m", str(tmp_path / "rgbd.y4m"), "--rgbd-tile", tile], "--rgbd-tile")


@pytest.mark.parametrize("view", ["6", "64", "x"])
def test_cli_refuses_a_view_out_of_range(native, tmp_path, view):
    _refused(native, tmp_path, [*ALL_FOCUS, "--rgbd-y4m", str(tmp_path / "rgbd.y4m"), "--rgbd-view", view], "--rgbd-view")


def test_cli_refuses_a_bad_map(native, tmp_path):
    _refused(native, tmp_path, [*ALL_FOCUS, "--rgbd-y4m", str(tmp_path / "rgbd.y4m"), "--rgbd-map", "2"], "--rgbd-map")


def test_cli_refuses_more_than_one_gpu(native, tmp_path):
    _refused(native, tmp_path, [*ALL_FOCUS, "-g", "2", "--rgbd-y4m", str(tmp_path / "rgbd.y4m")], "--rgbd-y4m", "one GPU")


def test_cli_refuses_the_rgbd_options_alone(native, tmp_path):
    _refused(native, tmp_path, [*ALL_FOCUS, "--rgbd-invert"], "--rgbd-invert", "--rgbd-y4m")
    _refused(native, tmp_path, ["--fps", "25"], "--rgbd-y4m")   # the video options name it among the flags they belong to


def test_cli_help_names_the_flags(native):
    res = run_cli(native, "-h")
    assert res.returncode == 0
    for flag in ("--rgbd-y4m FILE", "--rgbd-view N", "--rgbd-tile WxH", "--rgbd-map 0|1", "--rgbd-invert"):
        assert flag in res.stdout, flag
    line = next(l for l in res.stdout.splitlines() if l.startswith("--rgbd-y4m FILE"))
    assert "white as near" in line
    line = next(l for l in res.stdout.splitlines() if l.startswith("--rgbd-invert"))
    assert "swaps" in line


# ---- the code object ------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not code_object.have_tools(), reason="ROCm LLVM tools not installed")
def test_rgbd_yuv_scale_uses_no_scratch_and_16_kib_of_lds(native):
    """From the code object's metadata records: the four instantiations of rgbd_yuv_scale exist, use no scratch, spill nothing, hold at most
    16 KiB of LDS and stay at or below the registers tests/test_host_quilt_yuv.py allows quilt_yuv_scale: 96 (RGBA views) / 128 (planar views)"""
    kernels = code_object.named(code_object.kernels(native.build.HIP_LIB), "rgbd_yuv_scale")
    # <PLANAR, FORMAT>: Lb0 / Lb1, Li0 / Li1 in the mangled name
    assert sorted(re.search(r"ILb([01])ELi([01])E", k).groups() for k in kernels) == [("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")], sorted(kernels)
    for k, v in kernels.items():
        print(k, v)
        assert v[".private_segment_fixed_size"] == 0 and v[".vgpr_spill_count"] == 0 and v[".sgpr_spill_count"] == 0, (k, v)
        assert v[".group_segment_fixed_size"] <= 16 * 1024, (k, v)
        assert v[".vgpr_count"] <= (128 if "ILb1E" in k else 96), (k, v)
