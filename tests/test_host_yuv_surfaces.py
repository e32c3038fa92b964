"""CPU: the host side of the video surfaces (lfi_yuv_surfaces, lfi_upload_images_yuv, lfi_download_views_yuv, --nv12) — the layout helper of
tests/yuv_surfaces_ref.py, lfi_yuv_surfaces_packed against the frames' geometry, lfi_yuv_surfaces_check over good and bad descriptors (one
per refusal include/lfi.h lists; both need no GPU), header, exports and ctypes binding, the CLI's usage errors and the new kernels' code
object."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import code_object
import yuv_in_ref as in_ref
import yuv_surfaces_ref as sref
from view_rows import run_cli

SIZES = [(8, 2), (18, 5), (520, 6), (24, 10), (1, 1)]


# ---- the helper ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("fmt", [sref.I420, sref.NV12])
def test_scatter_and_gather_round_trip(fmt, w, h):
    cw, ch, fb = sref.sizes(w, h)
    frames = np.random.default_rng(w * 100 + h).integers(0, 256, (3, fb), dtype=np.uint8)
    for lay in (sref.tight(fmt, w, h), sref.pitched(fmt, w, h), sref.pitched(fmt, w, h, align=16, gap=0, tail=0)):
        assert lay.extent <= lay.frame_stride
        assert int(sref.own_mask(lay).sum()) == fb
        for poison in (0x00, 0xFF):
            s = sref.scatter(frames, lay, poison)
            assert s.shape == (3, lay.frame_stride)
            assert (sref.gather(s, lay) == frames).all() and sref.padding_holds(s, lay, poison)
            assert int((s != poison).sum()) <= 3 * fb
    # the tight I420 layout IS the frame; the tight NV12 layout has the same Y plane and the chroma interleaved
    assert (sref.scatter(frames, sref.tight(sref.I420, w, h), 0) == frames).all()
    nv = sref.scatter(frames, sref.tight(sref.NV12, w, h), 0)
    assert (nv[:, :w * h] == frames[:, :w * h]).all()
    assert (nv[:, w * h::2] == frames[:, w * h:w * h + cw * ch]).all() and (nv[:, w * h + 1::2] == frames[:, w * h + cw * ch:]).all()


# ---- lfi_yuv_surfaces_packed and lfi_yuv_surfaces_check ------------------------------------------------------------------------------------------

def _fields(s):
    return (s.format, s.memory, s.base, s.frame_stride, s.y_pitch, s.c_offset, s.c_pitch, s.cr_offset)


@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("fmt", [sref.I420, sref.NV12])
def test_packed_is_the_tight_layout(native, fmt, w, h):
    cw, ch, fb = in_ref.sizes(w, h)
    buf = np.zeros((2, fb), np.uint8)
    for memory in (sref.HOST, sref.DEVICE):
        s = native.yuv_surfaces_packed(fmt, memory, buf.ctypes.data, w, h)
        lay = sref.tight(fmt, w, h)
        assert _fields(s) == (fmt, memory, buf.ctypes.data, fb, lay.y_pitch, lay.c_offset, lay.c_pitch, lay.cr_offset)
        assert s.frame_stride == fb == lay.extent   # yuv420_frame_bytes' geometry, both formats
        assert s.check(w, h, 2)
    assert _fields(native.yuv_surfaces_packed("nv12" if fmt else "i420", "host", None, w, h))[2] is None
    lib = native.load_hip_library()
    out = native.YuvSurfaces()
    for bad in ((2, 0, w, h), (-1, 0, w, h), (fmt, 2, w, h), (fmt, -1, w, h), (fmt, 0, 0, h), (fmt, 0, w, 0), (fmt, 0, -3, h)):
        assert lib.lfi_yuv_surfaces_packed(bad[0], bad[1], None, bad[2], bad[3], C.byref(out)) == -1, bad
    assert lib.lfi_yuv_surfaces_packed(fmt, 0, None, w, h, None) == -1


W, H = 18, 5          # cw = 9, ch = 3
I_GOOD = dict(fmt=sref.I420, y_pitch=32, c_offset=5 * 32 + 16, c_pitch=16, cr_offset=5 * 32 + 16 + 3 * 16 + 16, frame_stride=512)
N_GOOD = dict(fmt=sref.NV12, y_pitch=32, c_offset=5 * 32 + 16, c_pitch=32, cr_offset=0, frame_stride=512)
GOOD = [
    ("I420 pitched", I_GOOD, 3),
    ("NV12 pitched", N_GOOD, 3),
    ("I420 at the minimum pitches, planes back to back", dict(fmt=sref.I420, y_pitch=18, c_offset=90, c_pitch=9, cr_offset=117, frame_stride=144), 3),
    ("NV12 at the minimum pitches", dict(fmt=sref.NV12, y_pitch=18, c_offset=90, c_pitch=18, cr_offset=0, frame_stride=144), 3),
    ("one frame needs no stride", dict(I_GOOD, frame_stride=0), 1),
    ("one NV12 frame needs no stride", dict(N_GOOD, frame_stride=0), 1),
]
BAD = [
    ("unknown format", dict(I_GOOD, fmt=2), 3),
    ("negative format", dict(I_GOOD, fmt=-1), 3),
    ("unknown memory", dict(I_GOOD, memory=2), 3),
    ("NULL base", dict(I_GOOD, base=None), 3),
    ("width 0", dict(I_GOOD, w=0), 3),
    ("height 0", dict(I_GOOD, h=0), 3),
    ("n = 0", I_GOOD, 0),
    ("n = -1", I_GOOD, -1),
    ("y_pitch below W", dict(I_GOOD, y_pitch=17, c_offset=400, cr_offset=460), 3),
    ("I420 c_pitch below cw", dict(I_GOOD, c_pitch=8), 3),
    ("NV12 c_pitch below 2*cw", dict(N_GOOD, c_pitch=17), 3),
    ("chroma inside the Y plane", dict(I_GOOD, c_offset=5 * 32 - 1), 3),
    ("NV12 chroma inside the Y plane", dict(N_GOOD, c_offset=5 * 32 - 1), 3),
    ("chroma before the Y plane's end (offset 0)", dict(N_GOOD, c_offset=0), 3),
    ("Cr inside the Cb plane", dict(I_GOOD, cr_offset=I_GOOD["c_offset"] + 3 * 16 - 1), 3),
    ("Cr before Cb", dict(I_GOOD, c_offset=I_GOOD["cr_offset"], cr_offset=I_GOOD["c_offset"]), 3),
    ("Cr on Cb", dict(I_GOOD, cr_offset=I_GOOD["c_offset"]), 3),
    ("NV12 with cr_offset", dict(N_GOOD, cr_offset=400), 3),
    ("frame_stride below the extent", dict(I_GOOD, frame_stride=I_GOOD["cr_offset"] + 3 * 16 - 1), 2),
    ("NV12 frame_stride below the extent", dict(N_GOOD, frame_stride=N_GOOD["c_offset"] + 3 * 32 - 1), 2),
    ("frame_stride 0 with two frames", dict(I_GOOD, frame_stride=0), 2),
]


def _descriptor(native, d, buf):
    return native.YuvSurfaces.make(d["fmt"], d.get("memory", sref.HOST), d.get("base", buf.ctypes.data), d["frame_stride"], d["y_pitch"], d["c_offset"],
                                   d["c_pitch"], d["cr_offset"], keep=buf)


@pytest.mark.parametrize("what,d,n", GOOD, ids=[g[0] for g in GOOD])
def test_check_accepts(native, what, d, n):
    buf = np.zeros(2048, np.uint8)
    assert native.load_hip_library().lfi_yuv_surfaces_check(C.byref(_descriptor(native, d, buf)), d.get("w", W), d.get("h", H), n) == 0
    # the stride exactly at the extent is enough
    extent = (d["c_offset"] if d["fmt"] == sref.NV12 else d["cr_offset"]) + 3 * d["c_pitch"]
    assert native.load_hip_library().lfi_yuv_surfaces_check(C.byref(_descriptor(native, dict(d, frame_stride=extent), buf)), W, H, 3) == 0


@pytest.mark.parametrize("what,d,n", BAD, ids=[b[0] for b in BAD])
def test_check_refuses(native, what, d, n):
    buf = np.zeros(2048, np.uint8)
    assert native.load_hip_library().lfi_yuv_surfaces_check(C.byref(_descriptor(native, d, buf)), d.get("w", W), d.get("h", H), n) == -1   # LFI_EINVAL


def test_check_refuses_a_null_descriptor_and_sizes_that_overflow(native):
    lib = native.load_hip_library()
    assert lib.lfi_yuv_surfaces_check(None, W, H, 1) == -1
    buf = np.zeros(16, np.uint8)
    huge = 1 << 62
    for d in (dict(I_GOOD, y_pitch=huge, c_offset=huge, cr_offset=huge), dict(N_GOOD, c_pitch=huge), dict(I_GOOD, frame_stride=huge)):
        assert lib.lfi_yuv_surfaces_check(C.byref(_descriptor(native, d, buf)), W, H, 1 << 20) == -1


# ---- header, exports, binding ---------------------------------------------------------------------------------------------------------------------

def test_header_exports_and_binding_agree(native):
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "lfi.h")).read()
    assert "#define LFI_ABI_VERSION 1" in re.sub(r"[ \t]+", " ", header)
    assert "enum { LFI_YUV_I420 = 0, LFI_YUV_NV12 = 1 };" in header and "enum { LFI_MEM_HOST = 0, LFI_MEM_DEVICE = 1 };" in header
    assert (native.LFI_YUV_I420, native.LFI_YUV_NV12, native.LFI_MEM_HOST, native.LFI_MEM_DEVICE) == (sref.I420, sref.NV12, sref.HOST, sref.DEVICE) == (0, 1, 0, 1)
    # the struct's members, in the header's order and with its types
    body = header[header.index("typedef struct lfi_yuv_surfaces {"):header.index("} lfi_yuv_surfaces;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = []
    for ctype, names in re.findall(r"(int32_t|void|size_t)\s+([^;]+);", body):
        for name in names.split(","):
            members.append((name.strip().lstrip("*"), {"int32_t": C.c_int32, "void": C.c_void_p, "size_t": C.c_size_t}[ctype]))
    assert members == list(native.YuvSurfaces._fields_)
    assert C.sizeof(native.YuvSurfaces) == 8 + 8 + 5 * C.sizeof(C.c_size_t)
    lib = native.load_hip_library()
    for name in ("lfi_yuv_surfaces_check", "lfi_yuv_surfaces_packed", "lfi_upload_images_yuv", "lfi_download_views_yuv"):
        assert name in native.ABI_SYMBOLS and hasattr(lib, name) and re.search(r"\bint %s\(" % name, header), name
    for method in ("upload_images_yuv", "download_views_yuv", "yuv_surfaces_packed"):
        assert hasattr(native.Context, method)
    assert lib.lfi_abi_version() == 1


# ---- the command line -----------------------------------------------------------------------------------------------------------------------------

CLI_ARGS = ["--synthetic", "3,3,16,8", "-t", "0,0,1,1", "-m", "STD", "-n", "4", "-b", "1", "-f", "0.0"]


@pytest.mark.parametrize("extra,words", [
    (["--nv12"], ("--nv12", "file")),
    (["--nv12", "v.nv12", "--fps", "0"], ("--fps", "N:D")),
    (["--nv12", "v.nv12", "--fps", "30:0"], ("--fps", "N:D")),
    (["--nv12", "v.nv12", "--fps"], ("--fps", "N:D")),
    (["--nv12", "v.nv12", "--yuv-matrix", "2020"], ("--yuv-matrix", "709", "601")),
    (["--nv12", "v.nv12", "--yuv-range", "tv"], ("--yuv-range", "limited", "full")),
    (["--nv12", "v.nv12", "--y4m"], ("--y4m", "file")),
    (["--fps", "25"], ("--fps", "--nv12")),
    (["--yuv-matrix", "601"], ("--yuv-matrix", "--nv12")),
    (["--yuv-range", "full"], ("--yuv-range", "--nv12")),
])
def test_cli_refuses_before_anything_runs(native, tmp_path, extra, words):
    extra = [str(tmp_path / e) if e == "v.nv12" else e for e in extra]
    res = run_cli(native, *CLI_ARGS, "-o", str(tmp_path / "out"), *extra)
    assert res.returncode != 0
    for word in words:
        assert word in res.stderr, res.stderr
    assert not (tmp_path / "out").exists() and not (tmp_path / "v.nv12").exists()


def test_cli_help_names_the_flag(native):
    res = run_cli(native, "-h")
    assert res.returncode == 0 and "--nv12 FILE" in res.stdout and "-f rawvideo -pix_fmt nv12" in res.stdout


# ---- the code object ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not code_object.have_tools(), reason="ROCm LLVM tools not installed")
def test_the_eight_instantiations_use_no_scratch_no_spills_and_no_lds(native):
    """From the code object's notes only: yuvs_expand<FORMAT, NEAREST> and yuvs_convert<PLANAR, FORMAT> (csrc/hip/yuv_surfaces.hpp) exist four
    times each, use no scratch and no LDS, spill nothing and stay within 128 VGPRs (at least four waves per SIMD)."""
    kernels = code_object.kernels(native.build.HIP_LIB)
    for stem, variants in (("yuvs_expand", ("ILi0ELb0E", "ILi0ELb1E", "ILi1ELb0E", "ILi1ELb1E")), ("yuvs_convert", ("ILb0ELi0E", "ILb0ELi1E", "ILb1ELi0E", "ILb1ELi1E"))):
        found = code_object.named(kernels, stem)
        assert len(found) == 4, sorted(found)
        for variant in variants:
            assert any(variant in k for k in found), (stem, variant, sorted(found))
        for k, v in found.items():
            assert v[".private_segment_fixed_size"] == 0 and v[".vgpr_spill_count"] == 0 and v[".sgpr_spill_count"] == 0, (k, v)
            assert v[".group_segment_fixed_size"] == 0 and v[".vgpr_count"] <= 128, (k, v)
