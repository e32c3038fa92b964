"""CPU: lfi_upload_images_yuv_derived's surroundings — the numpy restatement of the derived planar copy (tests/derived_ref.py) against a case
written out by hand, the three symbols in the header, the library and the binding, the code object's notes, and what the command line refuses
of --lean-inputs before a GPU is opened."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import code_object
import derived_ref
from view_rows import run_cli


def test_restatement_against_a_row_written_out_by_hand():
    """two 3 x 1 images, pitch 12, padx 4: image 0 (phase 0) has pixel 0 at byte 4, image 1 (phase 3) at byte 7"""
    images = np.zeros((2, 1, 3, 4), np.uint8)
    images[0, 0] = [[10, 20, 30, 255], [11, 21, 31, 255], [12, 22, 32, 255]]
    images[1, 0] = [[50, 60, 70, 255], [51, 61, 71, 255], [52, 62, 72, 255]]
    lay = SimpleNamespace(pitch_bytes=12, rows=1, padx=4)
    got = derived_ref.planes(images, lay, [0, 3])
    assert got.shape == (2, 3, 1, 12) and got.dtype == np.uint8
    assert got[0, 0, 0].tolist() == [10, 10, 10, 10, 10, 11, 12, 12, 12, 12, 12, 12]
    assert got[0, 1, 0].tolist() == [20, 20, 20, 20, 20, 21, 22, 22, 22, 22, 22, 22]
    assert got[0, 2, 0].tolist() == [30, 30, 30, 30, 30, 31, 32, 32, 32, 32, 32, 32]
    assert got[1, 0, 0].tolist() == [50, 50, 50, 50, 50, 50, 50, 50, 51, 52, 52, 52]
    assert got[1, 2, 0].tolist() == [70, 70, 70, 70, 70, 70, 70, 70, 71, 72, 72, 72]


def test_restatement_takes_every_row_and_no_alpha():
    rng = np.random.default_rng(7)
    images = rng.integers(0, 256, (3, 5, 18, 4), dtype=np.uint8)
    lay = SimpleNamespace(pitch_bytes=256, rows=5, padx=8)
    phases = [0, 127, 64]
    got = derived_ref.planes(images, lay, phases)
    for g in range(3):
        first = 8 + phases[g]
        assert (got[g, :, :, first:first + 18] == images[g, :, :, :3].transpose(2, 0, 1)).all()
        assert (got[g, :, :, :first] == images[g, :, :1, :3].transpose(2, 0, 1)).all()
        assert (got[g, :, :, first + 18:] == images[g, :, -1:, :3].transpose(2, 0, 1)).all()


def test_header_library_and_binding_agree(native):
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "lfi.h")).read()
    lib = native.load_hip_library()
    for name in ("lfi_upload_images_yuv_derived", "lfi_debug_derived_layout", "lfi_debug_download_derived"):
        assert name in native.ABI_SYMBOLS and hasattr(lib, name) and re.search(r"\bint %s\(" % name, header), name
    for method in ("upload_images_yuv_derived", "derived_layout", "download_derived"):
        assert hasattr(native.Context, method)
    # the struct's members, in the header's order and with its types
    body = header[header.index("typedef struct lfi_derived_layout {"):header.index("} lfi_derived_layout;")]
    members = []
    for ctype, names in re.findall(r"(int|size_t)\s+([^;]+);", body):
        members += [(name.strip(), {"int": C.c_int32, "size_t": C.c_size_t}[ctype]) for name in names.split(",")]
    assert members == list(native.DerivedLayout._fields_)
    # the span a workgroup owns: one number in the header, the kernel's (a static_assert ties it) and the binding's
    assert re.search(r"#define LFI_YUV_DERIVED_SPAN (\d+)", header).group(1) == str(native.LFI_YUV_DERIVED_SPAN)
    assert native.LFI_YUV_DERIVED_SPAN % 128 == 0
    source = open(os.path.join(ROOT, "lfinterpolator_amd", "csrc", "hip", "yuv_derived.hpp")).read()
    assert "YUVD_SPAN == LFI_YUV_DERIVED_SPAN" in source and re.search(r"YUVD_SPAN = (\d+);", source).group(1) == str(native.LFI_YUV_DERIVED_SPAN)


def test_null_arguments_are_refused_without_a_context(native):
    lib = native.load_hip_library()
    assert lib.lfi_upload_images_yuv_derived(None, 0, 1, 0, 0, 0, None) == -1
    assert lib.lfi_debug_derived_layout(None, None, None) == -1
    assert lib.lfi_debug_download_derived(None, 0, 1, None) == -1


@pytest.mark.skipif(not code_object.have_tools(), reason="ROCm LLVM tools not installed")
def test_the_four_instantiations_use_no_scratch_and_fit_eight_workgroups_a_cu(native):
    """From the code object's notes: yuvs_derived_expand<FORMAT, NEAREST> (csrc/hip/yuv_derived.hpp) exists four times, uses no scratch, spills
    nothing, stays within 128 VGPRs and within 16 KiB of LDS — eight workgroups of 256 lanes fit a CU by registers and by LDS alike."""
    kernels = code_object.kernels(native.build.HIP_LIB)
    found = code_object.named(kernels, "yuvs_derived_expand")
    assert len(found) == 4, sorted(found)
    for variant in ("ILi0ELb0E", "ILi0ELb1E", "ILi1ELb0E", "ILi1ELb1E"):
        assert any(variant in k for k in found), (variant, sorted(found))
    for k, v in found.items():
        assert v[".private_segment_fixed_size"] == 0 and v[".vgpr_spill_count"] == 0 and v[".sgpr_spill_count"] == 0, (k, v)
        assert 0 < v[".group_segment_fixed_size"] <= 16 * 1024 and v[".vgpr_count"] <= 128, (k, v)


# ---- the GPU tests' parameters, chosen here -----------------------------------------------------------------------------------------------------

def test_the_gpu_tests_focus_varies_the_alignment(native):
    """padx + phase[g] is congruent to minus image g's integer x offset mod 128 (the phases align offset + padx + phase): the focus of every
    shape of tests/test_gpu_yuv_derived.py gives both parities and three residues mod 4 (two images: two residues), and shifts to both sides"""
    import test_gpu_yuv_derived as t
    for shape in t.SHAPES:
        x = t.params(shape).focused_offsets[:, 0]
        assert t.firsts_are_varied(-x), (shape, x.tolist())
        assert x.min() < 0 < x.max(), shape
    assert t.SHAPES[2][2] == t.SHAPES[3][2] == native.LFI_YUV_DERIVED_SPAN + 10


# ---- the command line -----------------------------------------------------------------------------------------------------------------------------

VIDEO_ARGS = ["-t", "0,0,1,1", "-m", "STD", "-n", "4", "-b", "1", "-f", "0.1", "--lean-inputs"]


@pytest.mark.parametrize("extra,words", [
    (["-r", "0.5"], ("-r above 0",)),
    (["--autofocus", "-r", "0.5"], ("--autofocus",)),
    (["--autofocus"], ("--autofocus",)),
    (["--auto-range", "-r", "0.5"], ("--auto-range",)),
    (["--focus-tiles", "2x2", "-r", "0.5"], ("--focus-tiles",)),
    (["--view-maps", "-c", "-r", "0.5"], ("--view-maps",)),
    (["-c"], ("-c ",)),
    (["-F", "0.3"], ("-F ",)),
    (["-g", "2"], ("-g above 1",)),
])
def test_cli_refuses_lean_inputs_before_anything_runs(native, tmp_path, extra, words):
    """decided from the arguments alone: the input directory does not even exist"""
    res = run_cli(native, "-i", str(tmp_path / "no_such_video"), *VIDEO_ARGS, "-o", str(tmp_path / "out"), *extra)
    assert res.returncode != 0 and "--lean-inputs" in res.stderr, res.stderr
    for word in words:
        assert word in res.stderr, res.stderr
    assert not (tmp_path / "out").exists()


def test_cli_refuses_lean_inputs_without_a_video(native, tmp_path):
    res = run_cli(native, "--synthetic", "3,3,16,8", *VIDEO_ARGS, "-o", str(tmp_path / "out"))
    assert res.returncode != 0 and "--lean-inputs" in res.stderr and ".y4m" in res.stderr, res.stderr
    assert not (tmp_path / "out").exists()


def test_cli_help_names_the_flag(native):
    res = run_cli(native, "-h")
    assert res.returncode == 0 and "--lean-inputs" in res.stdout
