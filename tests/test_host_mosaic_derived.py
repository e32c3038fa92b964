"""CPU: lfi_upload_mosaic_yuv_derived's surroundings — the two new symbols in the header, the library and the binding; the code object's notes
and bodies for the twelve new kernels; the restatement the GPU tests compare against (derived_ref.planes over mosaic_ref.expand) on a case
written out by hand; and the parameters of tests/test_gpu_mosaic_derived.py that are chosen here: the focus of every case and the chunk plans
of the caps."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import code_object
import derived_ref
import mosaic_ref as mref
import yuv_in_ref as in_ref


# ---- the interface ------------------------------------------------------------------------------------------------------------------------------

def test_header_library_and_binding_agree(native):
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "lfi.h")).read()
    lib = native.load_hip_library()
    assert re.search(r"int lfi_upload_mosaic_yuv_derived\(lfi_ctx \*ctx, const lfi_mosaic \*m, int g0, int matrix, int range, int chroma, const lfi_yuv_surfaces \*src\);", header)
    assert re.search(r"int lfi_debug_set_mosaic_chunk_cap\(lfi_ctx \*ctx, size_t cap_bytes\);", header)
    for name in ("lfi_upload_mosaic_yuv_derived", "lfi_debug_set_mosaic_chunk_cap"):
        assert name in native.ABI_SYMBOLS and hasattr(lib, name), name
    for method in ("upload_mosaic_yuv_derived", "set_mosaic_chunk_cap"):
        assert hasattr(native.Context, method), method
    assert hasattr(native, "upload_mosaic_yuv_derived") and "upload_mosaic_yuv_derived" in native.__all__
    # the new call takes what lfi_upload_mosaic_yuv takes
    assert lib.lfi_upload_mosaic_yuv_derived.argtypes == lib.lfi_upload_mosaic_yuv.argtypes


def test_null_arguments_are_refused_without_a_context(native):
    lib = native.load_hip_library()
    m = native.Mosaic.make(1, 1)
    assert lib.lfi_upload_mosaic_yuv_derived(None, C.byref(m), 0, 0, 0, 0, None) == -1
    assert lib.lfi_upload_mosaic_yuv_derived(None, None, 0, 0, 0, 0, None) == -1
    assert lib.lfi_debug_set_mosaic_chunk_cap(None, 0) == -1
    assert lib.lfi_debug_set_mosaic_chunk_cap(None, 1 << 20) == -1


# ---- the code object ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not code_object.have_tools(), reason="ROCm LLVM tools not installed")
def test_mosaic_derived_kernels_exist_and_fit(native):
    """yuvs_mosaic_derived_expand<FORMAT, NEAREST, UNALIGNED> eight times and yuvs_mosaic_derived_expand_left<FORMAT, UNALIGNED> four times, under
    stems of their own.  No scratch, no spills, LDS within the 16 KiB of the frame kernels; the aligned ones within 128 VGPRs — eight
    workgroups of 256 lanes fit a CU — and they load what their yuvs_derived_expand[_left] twin loads; the unaligned ones load dwords only — no
    wider load could be aligned — and shift them with v_alignbyte_b32"""
    kernels = code_object.kernels(native.build.HIP_LIB)
    bodies = code_object.bodies(native.build.HIP_LIB)
    expect = {"yuvs_mosaic_derived_expand": [f"ILi{f}ELb{n}ELb{u}E" for f in "01" for n in "01" for u in "01"],
              "yuvs_mosaic_derived_expand_left": [f"ILi{f}ELb{u}E" for f in "01" for u in "01"]}
    loads = lambda text: sorted(re.findall(r"global_load_\w+", text))
    twins = {"yuvs_mosaic_derived_expand": "yuvs_derived_expand", "yuvs_mosaic_derived_expand_left": "yuvs_derived_expand_left"}
    for stem, variants in expect.items():
        found = code_object.named(kernels, stem)
        assert len(found) == len(variants), (stem, sorted(found))
        twin_stem = twins[stem]
        twin = {k[len(f"_ZN3lfi{len(twin_stem)}{twin_stem}"):k.index("EEEv")]: v for k, v in code_object.named(bodies, twin_stem).items()}
        for v in variants:
            assert sum(f"{stem}{v}" in k for k in found) == 1, (stem, v, sorted(found))
        for k, r in found.items():
            assert r[".private_segment_fixed_size"] == 0 and r[".vgpr_spill_count"] == 0 and r[".sgpr_spill_count"] == 0, (k, r)
            assert 0 < r[".group_segment_fixed_size"] <= 16 * 1024, (k, r)
            text = bodies[k]
            assert "scratch_" not in text and "atomic" not in text, k
            variant = k[len(f"_ZN3lfi{len(stem)}{stem}"):k.index("EEEv")]
            if variant.endswith("Lb1"):
                assert not re.search(r"global_load_dwordx[234]", text) and "v_alignbyte_b32" in text, k
                assert not re.search(r"global_load_(u|s)(byte|short)", text), k
            else:
                assert r[".vgpr_count"] <= 128, (k, r)
                assert loads(text) == loads(twin[variant[:-len("ELb0")]]), k
    # the stems are new: the existing kernels are counted as before
    assert len(code_object.named(kernels, "yuvs_derived_expand")) == 4 and len(code_object.named(kernels, "yuvs_derived_expand_left")) == 2
    assert len(code_object.named(kernels, "yuvs_mosaic_expand")) == 8 and len(code_object.named(kernels, "yuvs_mosaic_expand_left")) == 4


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------

def test_restatement_against_a_case_written_out_by_hand():
    """two 6 x 2 tiles side by side, full-range BT.601 with neutral chroma (Cb = Cr = 128), so that R = G = B = Y: tile 0 holds Y = 10 … 15
    in both rows, tile 1 Y = 50 … 55.  Pitch 16, padx 4: image 0 (phase 0) has pixel 0 at byte 4, image 1 (phase 5) at byte 9 — and its left
    padding holds its own first pixel, not tile 0's last"""
    w, h, mw, mh = 6, 2, 12, 2
    y = np.tile(np.concatenate([np.arange(10, 16), np.arange(50, 56)]).astype(np.uint8), (mh, 1))
    frame = in_ref.pack(y, np.full((1, 6), 128, np.uint8), np.full((1, 6), 128, np.uint8))
    tiles = mref.mosaic_map(2, 1, 0, 2, mref.ROWS, 0, 2, 1, 0)
    assert tiles.tolist() == [[0, 0, 0], [1, 0, 1]]
    images = mref.expand(frame, mw, mh, w, h, tiles, in_ref.BT601, in_ref.FULL, in_ref.NEAREST)
    for g, first in ((0, 10), (1, 50)):
        assert images[g].shape == (h, w, 4)
        assert (images[g][..., :3] == np.arange(first, first + 6, dtype=np.uint8)[None, :, None]).all(), g
    lay = SimpleNamespace(pitch_bytes=16, rows=2, padx=4)
    got = derived_ref.planes(np.stack([images[0], images[1]]), lay, [0, 5])
    assert got.shape == (2, 3, 2, 16)
    for c in range(3):
        for row in range(2):
            assert got[0, c, row].tolist() == [10, 10, 10, 10, 10, 11, 12, 13, 14, 15, 15, 15, 15, 15, 15, 15]
            assert got[1, c, row].tolist() == [50, 50, 50, 50, 50, 50, 50, 50, 50, 50, 51, 52, 53, 54, 55, 55]
    assert not set(range(10, 16)) & set(got[1].ravel().tolist()) and not set(range(50, 56)) & set(got[0].ravel().tolist())


def test_the_gpu_module_composes_the_same_two_restatements(native):
    import test_gpu_mosaic_derived as t
    case = t.CASES["5x1_6x2_rows_tiles_2_3"][0]
    conv = t.CONVERSIONS[0]
    frame = t._frame(30, 2, 7)
    lay = SimpleNamespace(pitch_bytes=128, rows=2, padx=16)
    phases = [0, 3, 64, 127, 1]
    images = t.want_images(frame, case, conv)
    tiles = t._tiles(case)
    assert tiles.tolist() == [[2, 0, 1], [3, 0, 2]]
    own = mref.expand(frame, 30, 2, 6, 2, tiles, *conv)
    assert (images[1] == own[1]).all() and (images[2] == own[2]).all()
    assert (t.restatement(frame, case, conv, lay, phases) == derived_ref.planes(images, lay, phases)).all()
    # the images the call does not map are the same whatever the frame
    other = t.want_images(t._frame(30, 2, 8), case, conv)
    assert (other[[0, 3, 4]] == images[[0, 3, 4]]).all() and not (other[1:3] == images[1:3]).all()


# ---- the GPU tests' parameters, chosen here ---------------------------------------------------------------------------------------------------------

def test_the_gpu_tests_focus_varies_the_alignment(native):
    """padx + phase[g] is congruent to minus image g's integer x offset mod 128: the focus of every case of tests/test_gpu_mosaic_derived.py
    gives both parities and three residues mod 4 (two images: two residues), and shifts to both sides"""
    import test_gpu_mosaic_derived as t
    from test_gpu_yuv_derived import firsts_are_varied
    for name, (case, focus, _) in list(t.CASES.items()) + [("order", (t.ORDER_CASE, t.ORDER_FOCUS, 0))]:
        x = t.params(case, focus).focused_offsets[:, 0]
        assert firsts_are_varied(-x), (name, x.tolist())
        assert x.min() < 0 < x.max(), name
    span = native.LFI_YUV_DERIVED_SPAN
    assert t.CASES["2x1_span8x12_rows"][0][2] == span + 8 and (span + 8) % 8 == 0
    assert t.CASES["2x1_span10x12_rows"][0][2] == span + 10 and (span + 10) % 8 == 2
    # six block rows: more than the five a workgroup takes
    assert t.CASES["2x1_span8x12_rows"][0][3] // 2 == 6


def _chunks(lib, m, w, h, cap):
    out = []
    for c in range(64):
        five = np.full(5, -7, np.int32)
        if lib.lfi_debug_mosaic_chunk(C.byref(m), w, h, cap, c, five.ctypes.data) != 0:
            break
        out.append(tuple(int(v) for v in five))
    return out


def test_the_gpu_tests_caps_give_the_chunks_they_claim(native):
    """(first tile row in ROWS order, tile rows, the frame's first tile row copied, first tile, tiles) of every chunk"""
    import test_gpu_mosaic_derived as t
    lib = native.load_hip_library()
    case, _, cap = t.CASES["1x3_24x4_rows_three_chunks"]
    assert cap == t.CAP_ONE_ROW and case[:4] == (1, 3, 24, 4) and not case[5]
    assert _chunks(lib, native.Mosaic.make(1, 3, "rows", False), 24, 4, cap) == [(0, 1, 0, 0, 1), (1, 1, 1, 1, 1), (2, 1, 2, 2, 1)]
    case, _, cap = t.CASES["1x3_24x4_rows_bottom_up_two_chunks"]
    assert cap == t.CAP_TWO_ROWS == 2 * (24 * 4 * 3 // 2) and case[:4] == (1, 3, 24, 4) and case[5]
    assert _chunks(lib, native.Mosaic.make(1, 3, "rows", True), 24, 4, cap) == [(0, 2, 1, 0, 2), (2, 1, 0, 2, 1)]
    # every chunk but the first copies from a tile row other than 0 or is biased: ty_bias != 0 is run
    assert any(c[2] != 0 for c in _chunks(lib, native.Mosaic.make(1, 3, "rows", False), 24, 4, t.CAP_ONE_ROW))
    # the other cases keep the calls' own cap: one chunk
    for name, (case, _, cap) in t.CASES.items():
        if name not in t.CAPPED:
            assert cap == 0
            m = native.Mosaic.make(case[0], case[1], case[4], case[5], case[6], case[7])
            cols, rows = (case[0], case[1]) if case[4] == "grid" else (case[7], 1)
            assert len(_chunks(lib, m, case[2], case[3], 0)) == 1, name
