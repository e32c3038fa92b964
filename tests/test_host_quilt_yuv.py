"""CPU: the host side of quilt video frames (lfi_download_quilt_yuv) — the symbol declared, exported and bound; the restatement
(tests/quilt_yuv_ref.py) at the views' own size against the frame of the unscaled quilt; the CLI's checks of --quilt-y4m; the fused kernel's
code object (csrc/hip/quilt_yuv.hpp)."""
import os
import re

import numpy as np
import pytest

import code_object
import quilt_yuv_ref as ref
import yuv_ref
from view_rows import run_cli

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "lfi.h")


def test_symbol_is_declared_exported_and_bound(native):
    text = open(HEADER).read()
    assert re.search(r"^int lfi_download_quilt_yuv\(lfi_ctx \*ctx, int tiles_x, int tiles_y, int v0, int tile_w, int tile_h, int matrix, int range, "
                     r"const lfi_yuv_surfaces \*dst\);$", text, re.M)
    assert "#define LFI_ABI_VERSION 1" in text   # the header has only grown
    lib = native.load_hip_library()
    assert "lfi_download_quilt_yuv" in native.ABI_SYMBOLS and hasattr(lib, "lfi_download_quilt_yuv")
    assert lib.lfi_download_quilt_yuv.argtypes is not None and len(lib.lfi_download_quilt_yuv.argtypes) == 9
    assert hasattr(native.Context, "download_quilt_yuv")


@pytest.mark.parametrize("W,H,tx,ty", [(50, 22, 4, 2), (17, 9, 3, 3), (8, 2, 1, 1)])
def test_restatement_at_the_views_size_is_the_frame_of_the_unscaled_quilt(W, H, tx, ty):
    views = np.random.default_rng(W * 100 + H).integers(0, 256, (tx * ty, H, W, 4), dtype=np.uint8)
    views[..., 3] = 255
    unscaled = views.reshape(ty, tx, H, W, 4).transpose(0, 2, 1, 3, 4).reshape(ty * H, tx * W, 4)
    for fmt in yuv_ref.FORMATS:
        got = ref.frame(views, tx, ty, W, H, *fmt)
        assert got.shape == (yuv_ref.sizes(tx * W, ty * H)[2],)
        assert (got == yuv_ref.frame(unscaled, *fmt)).all(), fmt


# ---- the command line -----------------------------------------------------------------------------------------------------------------

RUN_ARGS = ["--synthetic", "4,4,32,16", "-t", "0,0,1,1", "-m", "STD", "-n", "6", "-b", "1", "-f", "0.0"]


def test_cli_refuses_a_quilt_video_without_a_quilt(native, tmp_path):
    res = run_cli(native, *RUN_ARGS, "-o", str(tmp_path / "out"), "--quilt-y4m", str(tmp_path / "quilt.y4m"))
    assert res.returncode != 0
    assert "--quilt-y4m" in res.stderr and "-q" in res.stderr
    assert not (tmp_path / "out").exists() and not (tmp_path / "quilt.y4m").exists()


def test_cli_refuses_an_empty_file_name(native, tmp_path):
    res = run_cli(native, *RUN_ARGS, "-o", str(tmp_path / "out"), "-q", "3,2", "--quilt-y4m", "")
    assert res.returncode != 0
    assert "--quilt-y4m" in res.stderr and "name" in res.stderr
    assert not (tmp_path / "out").exists()


def test_cli_refuses_more_than_one_gpu(native, tmp_path):
    res = run_cli(native, *RUN_ARGS, "-o", str(tmp_path / "out"), "-q", "3,2", "-g", "2", "--quilt-y4m", str(tmp_path / "quilt.y4m"))
    assert res.returncode != 0
    assert "--quilt-y4m" in res.stderr and "one GPU" in res.stderr
    assert not (tmp_path / "out").exists() and not (tmp_path / "quilt.y4m").exists()


def test_cli_accepts_the_video_options_with_a_quilt_video(native, tmp_path):
    """--fps, --yuv-matrix and --yuv-range alone are refused; the message names --quilt-y4m among the flags they belong to"""
    res = run_cli(native, *RUN_ARGS, "-o", str(tmp_path / "out"), "--fps", "25")
    assert res.returncode != 0 and "--quilt-y4m" in res.stderr


def test_cli_help_names_the_flag(native):
    res = run_cli(native, "-h")
    assert res.returncode == 0 and "--quilt-y4m FILE" in res.stdout


# ---- the code object ------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not code_object.have_tools(), reason="ROCm LLVM tools not installed")
def test_quilt_yuv_scale_uses_no_scratch_no_atomics_and_16_kib_of_lds(native):
    """From the code object: the four instantiations of quilt_yuv_scale exist, use no scratch, spill nothing, hold at most 16 KiB of LDS, stay at
    or below 96 (RGBA views) / 128 (planar views) registers per lane — four waves per SIMD at least — and contain no atomic instruction."""
    kernels = code_object.kernels(native.build.HIP_LIB)
    fused = code_object.named(kernels, "quilt_yuv_scale")
    # <PLANAR, FORMAT>: Lb0 / Lb1, Li0 / Li1 in the mangled name
    assert sorted(re.search(r"ILb([01])ELi([01])E", k).groups() for k in fused) == [("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")], sorted(fused)
    for k, v in fused.items():
        print(k, v)
        assert v[".private_segment_fixed_size"] == 0 and v[".vgpr_spill_count"] == 0 and v[".sgpr_spill_count"] == 0, (k, v)
        assert v[".group_segment_fixed_size"] <= 16 * 1024, (k, v)
        assert v[".vgpr_count"] <= (128 if "ILb1E" in k else 96), (k, v)
    bodies = {k: v for k, v in code_object.bodies(native.build.HIP_LIB).items() if k in fused}
    assert set(bodies) == set(fused)
    for k, text in bodies.items():
        assert "atomic" not in text and "scratch_" not in text, k
        assert "global_load_dword" in text and "ds_write_b128" in text, k   # phase 1 is quilt_scale's
