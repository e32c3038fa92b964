"""CPU: 10-bit video surfaces (LFI_YUV_I010, LFI_YUV_P010; include/lfi.h) — the header's tables against their derivation, the properties the
header states of both directions over all 2^24 colours (tests/yuv10_ref.py), lfi_yuv_surfaces_check / _packed for the new formats (both
need no GPU), the new kernels' code object, the C420p10 Y4M tag through the host library and the command line's usage errors."""
import ctypes as C
import os
import re
from fractions import Fraction as F

import numpy as np
import pytest

import code_object
import yuv10_ref as ref
import yuv_ref as ref8
from view_rows import run_cli

K = {ref.BT709: (F(2126, 10000), F(722, 10000)), ref.BT601: (F(299, 1000), F(114, 1000))}   # Kr, Kb


def _round(x):
    return int((x + F(1, 2)).__floor__())


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_output_table_equals_its_derivation(fmt):
    """round(c·scale·2^14), G adjusted so that Y sums to 56284 / 65729 and Cb, Cr to 0"""
    matrix, rng = fmt
    kr, kb = K[matrix]
    kg = 1 - kr - kb
    ys, cs = (F(876, 255), F(896, 255)) if rng == ref.LIMITED else (F(1023, 255), F(1023, 255))
    y = [_round(c * ys * 2 ** 14) for c in (kr, kg, kb)]
    y[1] += (56284 if rng == ref.LIMITED else 65729) - sum(y)
    cb = [_round(c * cs * 2 ** 14) for c in (-kr / (2 * (1 - kb)), -kg / (2 * (1 - kb)), F(1, 2))]
    cb[1] -= sum(cb)
    cr = [_round(c * cs * 2 ** 14) for c in (F(1, 2), -kg / (2 * (1 - kr)), -kb / (2 * (1 - kr)))]
    cr[1] -= sum(cr)
    assert ref.OUT_TABLE[fmt] == (tuple(y), tuple(cb), tuple(cr), 64 if rng == ref.LIMITED else 0)
    assert 65729 == _round(F(1023, 255) * 2 ** 14) and 56284 == _round(F(876, 255) * 2 ** 14)


@pytest.mark.parametrize("matrix", [ref.BT709, ref.BT601])
def test_limited_output_sets_are_the_8_bit_ones(matrix):
    """876/255·2^14 = 219/255·2^16: the same integers, with the offset 64 for 16"""
    y, cb, cr, off = ref.OUT_TABLE[(matrix, ref.LIMITED)]
    y8, cb8, cr8, off8 = ref8.TABLE[(matrix, ref8.LIMITED)]
    assert (tuple(y), tuple(cb), tuple(cr)) == (tuple(y8), tuple(cb8), tuple(cr8)) and (off, off8) == (64, 16)


@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_input_table_equals_its_derivation(fmt):
    matrix, rng = fmt
    kr, kb = K[matrix]
    kg = 1 - kr - kb
    iy, ic = (F(255, 876), F(255, 896)) if rng == ref.LIMITED else (F(255, 1023), F(255, 1023))
    want = (_round(iy * 2 ** 16), _round(2 * (1 - kr) * ic * 2 ** 16), -_round(2 * kb * (1 - kb) / kg * ic * 2 ** 16),
            -_round(2 * kr * (1 - kr) / kg * ic * 2 ** 16), _round(2 * (1 - kb) * ic * 2 ** 16), 64 if rng == ref.LIMITED else 0)
    assert ref.IN_TABLE[fmt] == want


def test_header_and_kernel_source_hold_the_literals(native):
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "lfi.h")).read()
    kernel = open(os.path.join(ROOT, "lfinterpolator_amd", "csrc", "hip", "yuv10.hpp")).read()
    flat = lambda text: re.sub(r"\s+", " ", text)
    for fmt in ref.FORMATS:
        y, cb, cr, off = ref.OUT_TABLE[fmt]
        row = lambda k: ", ".join(str(v) for v in k)
        assert re.search(rf"{row(y)}\s+{row(cb)}\s+{row(cr)}\s+{off}\b", header), fmt
        assert f"{{{{{row(y)}}}, {{{row(cb)}}}, {{{row(cr)}}}, {off}}}" in flat(kernel), fmt
        k = ref.IN_TABLE[fmt]
        assert re.search(r"\s+".join(str(v) for v in k) + r"\b", header), fmt
        assert "{" + ", ".join(str(v) for v in k) + "}" in flat(kernel), fmt
    assert f"{ref.BRACKET_BOUND:,}" in header and f"{ref.BRACKET_BOUND:,}" in kernel
    assert re.search(r"#define LFI_YUV_10BIT 0x100\b", header)
    assert re.search(r"enum \{ LFI_YUV_I010 = LFI_YUV_I420 \| LFI_YUV_10BIT, LFI_YUV_P010 = LFI_YUV_NV12 \| LFI_YUV_10BIT \};", header)
    assert (native.LFI_YUV_10BIT, native.LFI_YUV_I010, native.LFI_YUV_P010) == (0x100, ref.I010, ref.P010) == (0x100, 0x100, 0x101)
    assert native.abi.YUV_FORMATS["i010"] == ref.I010 and native.abi.YUV_FORMATS["p010"] == ref.P010


# ---- all 2^24 colours ---------------------------------------------------------------------------------------------------------------------------

def _colour_chunks():
    """all 2^24 colours as [2^20][3] int64 chunks of 16 values of R"""
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for r0 in range(0, 256, 16):
        r = np.repeat(np.arange(r0, r0 + 16), 65536)
        yield np.stack([r, np.tile(g.reshape(-1), 16), np.tile(b.reshape(-1), 16)], axis=-1).astype(np.int64)


@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_ranges_greys_and_the_exact_round_trip_over_all_colours(fmt):
    """a uniform image of every colour: the ranges the header states, chroma 512 for every grey, the left-sited sample equal to the
    centre-sited one, and RGB8 -> 10-bit YUV -> RGB8 (nearest chroma) exact"""
    matrix, rng = fmt
    _, kb, kr, _ = ref.OUT_TABLE[fmt]
    y_lo = c_lo = 1 << 20
    y_hi = c_hi = raw_hi = -1
    for p in _colour_chunks():
        y = ref.luma(p, matrix, rng)
        planes = []
        for k in (kb, kr):
            c = ref.chroma(k, 4 * p, ref.CENTRE)
            assert (c == ref.chroma(k, 8 * p, ref.LEFT)).all()
            raw_hi = max(raw_hi, int(ref.chroma(k, 4 * p, ref.CENTRE, clamp=False).max()))
            planes.append(c)
        grey = (p[:, 0] == p[:, 1]) & (p[:, 1] == p[:, 2])
        assert (planes[0][grey] == 512).all() and (planes[1][grey] == 512).all()
        y_lo, y_hi = min(y_lo, int(y.min())), max(y_hi, int(y.max()))
        c_lo, c_hi = min(c_lo, int(min(planes[0].min(), planes[1].min()))), max(c_hi, int(max(planes[0].max(), planes[1].max())))
        back = ref.convert(y, 16 * planes[0], 16 * planes[1], matrix, rng)
        assert (back[:, :3] == p).all() and (back[:, 3] == 255).all(), "the round trip is not exact"
    if rng == ref.LIMITED:
        assert (y_lo, y_hi, c_lo, c_hi, raw_hi) == (64, 940, 64, 960, 960)
    else:
        assert (y_lo, y_hi, c_lo, c_hi, raw_hi) == (0, 1023, 1, 1023, 1023)   # the bracket ends 384 below 2^26: the min is a guard here


# ---- input: the bracket, the fixed points ---------------------------------------------------------------------------------------------------------

def test_input_bracket_bound_over_the_corner_triples():
    """each bracket is linear in Y, SU, SV: its extremes lie at the corners of [0, 1023] x [0, 16368]^2.  The largest, rounding term included, is
    the header's figure, and int32 holds it"""
    worst = 0
    for fmt in ref.FORMATS:
        y, su, sv = np.meshgrid([0, 1023], [0, 16 * 1023], [0, 16 * 1023], indexing="ij")
        worst = max(worst, max(int(np.abs(b).max()) for b in ref.brackets(y, su, sv, *fmt)))
    assert worst == ref.BRACKET_BOUND < 2 ** 31
    # and no interior triple exceeds a corner: a random sample
    rng = np.random.default_rng(10)
    y, su, sv = rng.integers(0, 1024, 1 << 16), rng.integers(0, 16369, 1 << 16), rng.integers(0, 16369, 1 << 16)
    for fmt in ref.FORMATS:
        assert max(int(np.abs(b).max()) for b in ref.brackets(y, su, sv, *fmt)) <= ref.BRACKET_BOUND


@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_input_fixed_points(fmt):
    """chroma 512 gives R = G = B for every luma code; limited 64 -> 0 and 940 -> 255, full 0 -> 0 and 1023 -> 255; codes outside the nominal
    range are clamped"""
    matrix, rng = fmt
    y = np.arange(1024)
    px = ref.convert(y, np.full(1024, 16 * 512), np.full(1024, 16 * 512), matrix, rng)
    assert (px[:, 0] == px[:, 1]).all() and (px[:, 1] == px[:, 2]).all() and (px[:, 3] == 255).all()
    if rng == ref.LIMITED:
        assert px[64, 0] == 0 and px[940, 0] == 255 and (px[:64, 0] == 0).all() and (px[940:, 0] == 255).all() and px[65, 0] == 0 and px[939, 0] == 255
        assert px[66, 0] == 1   # (2·19077·16 + 2^19) >> 20
    else:
        assert px[0, 0] == 0 and px[1023, 0] == 255 and px[2, 0] == 0 and px[3, 0] == 1
    assert (np.diff(px[:, 0].astype(int)) >= 0).all()


def test_restatement_of_the_filters_on_a_small_frame():
    """by hand, 4 x 2 with cw = 2: centre bilinear 9/3/3/1 with clamped neighbours, left-sited 3·h(cy) + h(ny); nearest under either siting"""
    u = np.array([[100, 900]])
    assert (ref.chroma16(u, 4, 2, ref.NEAREST, ref.CENTRE) == 16 * np.array([[100, 100, 900, 900]] * 2)).all()
    assert (ref.chroma16(u, 4, 2, ref.NEAREST, ref.LEFT) == ref.chroma16(u, 4, 2, ref.NEAREST, ref.CENTRE)).all()
    # centre: one chroma row, so ny = cy and the column weights are 12 / 4
    assert (ref.chroma16(u, 4, 2, ref.BILINEAR, ref.CENTRE) == np.array([[1600, 12 * 100 + 4 * 900, 12 * 900 + 4 * 100, 14400]] * 2)).all()
    # left: even columns sit on their sample, odd ones halfway to the next (clamped at the edge)
    assert (ref.chroma16(u, 4, 2, ref.BILINEAR, ref.LEFT) == np.array([[1600, 8 * 100 + 8 * 900, 14400, 14400]] * 2)).all()


# ---- the surfaces' helper ------------------------------------------------------------------------------------------------------------------------

SIZES = [(8, 2), (18, 5), (520, 6), (24, 10), (1, 1), (9, 3)]


@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("fmt", [ref.I010, ref.P010])
def test_scatter_and_gather_round_trip(fmt, w, h):
    cw, ch, n = ref.sizes(w, h)
    rng = np.random.default_rng(w * 100 + h)
    codes = rng.integers(0, 1024, (3, n), dtype=np.uint16)
    junk = rng.integers(0, 65536, (3, n), dtype=np.uint16)
    for lay in (ref.tight(fmt, w, h), ref.pitched(fmt, w, h), ref.pitched(fmt, w, h, align=16, gap=0, tail=0)):
        assert lay.extent <= lay.frame_stride and int(ref.own_mask(lay).sum()) == 2 * n
        for poison in (0x00, 0xFF):
            s = ref.scatter(codes, lay, poison)
            assert s.shape == (3, lay.frame_stride) and ref.padding_holds(s, lay, poison)
            assert (ref.gather(s, lay) == ref.words(codes, fmt)).all()
            dirty = ref.gather(ref.scatter(codes, lay, poison, junk), lay)
            assert ((dirty >> 6 if fmt == ref.P010 else dirty & 1023) == codes).all() and (dirty != ref.words(codes, fmt)).any()
    # the tight I010 layout IS the codes as little-endian words; tight P010: the Y plane, then Cb and Cr interleaved, the code in the upper bits
    assert (ref.scatter(codes, ref.tight(ref.I010, w, h), 0).view("<u2") == codes).all()
    p = ref.scatter(codes, ref.tight(ref.P010, w, h), 0).view("<u2")
    assert (p[:, :w * h] == codes[:, :w * h] << 6).all()
    assert (p[:, w * h::2] == codes[:, w * h:w * h + cw * ch] << 6).all() and (p[:, w * h + 1::2] == codes[:, w * h + cw * ch:] << 6).all()


# ---- lfi_yuv_surfaces_packed and lfi_yuv_surfaces_check ------------------------------------------------------------------------------------------

def _fields(s):
    return (s.format, s.memory, s.base, s.frame_stride, s.y_pitch, s.c_offset, s.c_pitch, s.cr_offset)


@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("fmt", [ref.I010, ref.P010])
def test_packed_is_the_tight_layout(native, fmt, w, h):
    cw, ch, n = ref.sizes(w, h)
    buf = np.zeros((2, 2 * n), np.uint8)
    lay = ref.tight(fmt, w, h)
    for memory in (ref.HOST, ref.DEVICE):
        s = native.yuv_surfaces_packed(fmt, memory, buf.ctypes.data, w, h)
        assert _fields(s) == (fmt, memory, buf.ctypes.data, 2 * n, lay.y_pitch, lay.c_offset, lay.c_pitch, lay.cr_offset)
        assert s.frame_stride == 2 * (w * h + 2 * cw * ch) == lay.extent
        assert s.check(w, h, 2)
    assert _fields(native.yuv_surfaces_packed("p010" if fmt == ref.P010 else "i010", "host", None, w, h))[0] == fmt
    lib = native.load_hip_library()
    out = native.YuvSurfaces()
    for bad in (0x100 | 2, 0x100 | 3, 0x200, 0x300, 2):
        assert lib.lfi_yuv_surfaces_packed(bad, 0, None, w, h, C.byref(out)) == -1, bad


W, H = 18, 5          # cw = 9, ch = 3
I_GOOD = dict(fmt=ref.I010, y_pitch=64, c_offset=5 * 64 + 16, c_pitch=32, cr_offset=5 * 64 + 16 + 3 * 32 + 16, frame_stride=1024)
P_GOOD = dict(fmt=ref.P010, y_pitch=64, c_offset=5 * 64 + 16, c_pitch=64, cr_offset=0, frame_stride=1024)
GOOD = [
    ("I010 pitched", I_GOOD, 3),
    ("P010 pitched", P_GOOD, 3),
    ("I010 at the minimum pitches, planes back to back", dict(fmt=ref.I010, y_pitch=36, c_offset=180, c_pitch=18, cr_offset=234, frame_stride=288), 3),
    ("P010 at the minimum pitches", dict(fmt=ref.P010, y_pitch=36, c_offset=180, c_pitch=36, cr_offset=0, frame_stride=288), 3),
    ("one frame needs no stride", dict(I_GOOD, frame_stride=0), 1),
    ("an even base that is no multiple of 4", dict(P_GOOD, shift=2), 3),
]
BAD = [
    ("0x100 | 2", dict(I_GOOD, fmt=0x100 | 2), 3),
    ("plain 2", dict(I_GOOD, fmt=2), 3),
    ("0x200", dict(I_GOOD, fmt=0x200), 3),
    ("another flag beside the depth", dict(I_GOOD, fmt=ref.I010 | 0x200), 3),
    ("I010 y_pitch one byte below 2W", dict(I_GOOD, y_pitch=35), 3),
    ("I010 y_pitch one sample below 2W", dict(I_GOOD, y_pitch=34), 3),
    ("the 8-bit minimum is not enough", dict(I_GOOD, y_pitch=18), 3),
    ("I010 c_pitch one byte below 2cw", dict(I_GOOD, c_pitch=17), 3),
    ("I010 c_pitch one sample below 2cw", dict(I_GOOD, c_pitch=16), 3),
    ("P010 c_pitch one byte below 4cw", dict(P_GOOD, c_pitch=35), 3),
    ("P010 c_pitch one sample below 4cw", dict(P_GOOD, c_pitch=34), 3),
    ("P010 c_pitch at I010's minimum", dict(P_GOOD, c_pitch=18), 3),
    ("an odd y_pitch", dict(I_GOOD, y_pitch=65, c_offset=5 * 65 + 17, cr_offset=5 * 65 + 17 + 3 * 32 + 16), 3),
    ("an odd c_pitch", dict(P_GOOD, c_pitch=65), 3),
    ("an odd c_offset", dict(P_GOOD, c_offset=P_GOOD["c_offset"] + 1), 3),
    ("an odd cr_offset", dict(I_GOOD, cr_offset=I_GOOD["cr_offset"] + 1), 3),
    ("an odd frame_stride", dict(I_GOOD, frame_stride=1023), 3),
    ("an odd base", dict(I_GOOD, shift=1), 3),
    ("an odd base, P010", dict(P_GOOD, shift=1), 1),
    ("chroma inside the Y plane", dict(I_GOOD, c_offset=5 * 64 - 2), 3),
    ("Cr inside the Cb plane", dict(I_GOOD, cr_offset=I_GOOD["c_offset"] + 3 * 32 - 2), 3),
    ("P010 with cr_offset", dict(P_GOOD, cr_offset=800), 3),
    ("frame_stride below the extent", dict(I_GOOD, frame_stride=I_GOOD["cr_offset"] + 3 * 32 - 2), 2),
]


def _descriptor(native, d, buf):
    assert buf.ctypes.data % 16 == 0
    return native.YuvSurfaces.make(d["fmt"], ref.HOST, buf.ctypes.data + d.get("shift", 0), d["frame_stride"], d["y_pitch"], d["c_offset"], d["c_pitch"],
                                   d["cr_offset"], keep=buf)


def _aligned(n):
    raw = np.zeros(n + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + n]


@pytest.mark.parametrize("what,d,n", GOOD, ids=[g[0] for g in GOOD])
def test_check_accepts(native, what, d, n):
    assert native.load_hip_library().lfi_yuv_surfaces_check(C.byref(_descriptor(native, d, _aligned(4096))), W, H, n) == 0


@pytest.mark.parametrize("what,d,n", BAD, ids=[b[0] for b in BAD])
def test_check_refuses(native, what, d, n):
    assert native.load_hip_library().lfi_yuv_surfaces_check(C.byref(_descriptor(native, d, _aligned(4096))), W, H, n) == -1   # LFI_EINVAL


def test_the_8_bit_formats_keep_odd_layouts(native):
    """the alignment rule is the 10-bit formats' alone: an odd base, pitch, offset and stride stay legal for I420 and NV12"""
    lib = native.load_hip_library()
    buf = _aligned(4096)
    odd = native.YuvSurfaces.make(0, ref.HOST, buf.ctypes.data + 1, 301, 19, 95, 9, 123, keep=buf)
    assert lib.lfi_yuv_surfaces_check(C.byref(odd), W, H, 3) == 0
    odd = native.YuvSurfaces.make(1, ref.HOST, buf.ctypes.data + 1, 301, 19, 95, 19, 0, keep=buf)
    assert lib.lfi_yuv_surfaces_check(C.byref(odd), W, H, 3) == 0


# ---- the code object ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not code_object.have_tools(), reason="ROCm LLVM tools not installed")
def test_ten_bit_kernels_exist_and_fit(native):
    """yuvs_expand10<FORMAT, NEAREST> and yuvs_convert10<PLANAR, FORMAT> four times each, yuvs_expand10_left<FORMAT> twice,
    yuvs_convert10_left<PLANAR, FORMAT> four times: no scratch, no LDS, no spills, at most 128 registers, no atomics; the left-sited
    conversion takes its one value from the neighbour lane with ONE cross-lane move.  The 8-bit kernels are as many as they were"""
    kernels = code_object.kernels(native.build.HIP_LIB)
    bodies = code_object.bodies(native.build.HIP_LIB)
    expect = {"yuvs_expand10": ("ILi0ELb0E", "ILi0ELb1E", "ILi1ELb0E", "ILi1ELb1E"), "yuvs_expand10_left": ("ILi0E", "ILi1E"),
              "yuvs_convert10": ("ILb0ELi0E", "ILb0ELi1E", "ILb1ELi0E", "ILb1ELi1E"), "yuvs_convert10_left": ("ILb0ELi0E", "ILb0ELi1E", "ILb1ELi0E", "ILb1ELi1E")}
    for stem, variants in expect.items():
        found = code_object.named(kernels, stem)
        assert len(found) == len(variants), (stem, sorted(found))
        for v in variants:
            assert sum(f"{stem}{v}" in k for k in found) == 1, (stem, v, sorted(found))
        for k, r in found.items():
            assert r[".private_segment_fixed_size"] == 0 and r[".vgpr_spill_count"] == 0 and r[".sgpr_spill_count"] == 0, (k, r)
            assert r[".group_segment_fixed_size"] == 0 and r[".vgpr_count"] <= 128, (k, r)
            text = bodies[k]
            assert "scratch_" not in text and "atomic" not in text and "ds_read" not in text and "ds_write" not in text, k
            moves = len(re.findall(r"_dpp|ds_bpermute|ds_permute|ds_swizzle|v_permlane|v_readlane", text))
            assert moves == (1 if stem == "yuvs_convert10_left" else 0), (k, moves)
    # a whole block leaves as words: a Y row is one 16-byte store, P010 chroma one more, I010 chroma two 8-byte stores; nothing narrower than a
    # sample is ever stored
    for k in list(code_object.named(kernels, "yuvs_convert10")) + list(code_object.named(kernels, "yuvs_convert10_left")):
        text = bodies[k]
        p010 = re.search(r"ILb[01]ELi1E", k) is not None
        assert text.count("global_store_dwordx4") == (3 if p010 else 2), k
        assert text.count("global_store_dwordx2") == (0 if p010 else 2), k
        assert "global_store_byte" not in text and "global_store_short" in text, k
    for stem in ("yuvs_expand", "yuvs_convert", "yuvs_convert_left"):
        assert len(code_object.named(kernels, stem)) == 4, stem
    assert len(code_object.named(kernels, "yuvs_expand_left")) == 2


# ---- Y4M ------------------------------------------------------------------------------------------------------------------------------------------

def test_y4m_c420p10_is_written_and_read_back(native, tmp_path):
    w, h = 18, 5
    n = ref.sizes(w, h)[2]
    codes = np.random.default_rng(4).integers(0, 1024, (3, n), dtype=np.uint16)
    frames = ref.scatter(codes, ref.tight(ref.I010, w, h), 0)
    assert frames.shape == (3, 2 * n)
    path = str(tmp_path / "deep.y4m")
    native.write_y4m(path, frames, w, h, fps=(25, 1), full_range=True, left_sited=True, depth=10)
    data = open(path, "rb").read()
    assert data.startswith(b"YUV4MPEG2 W18 H5 F25:1 Ip A1:1 C420p10 XCOLORRANGE=FULL\n")   # the tag has no siting
    assert len(data) == len(data.split(b"\n")[0]) + 1 + 3 * (6 + 2 * n)
    info = native.read_y4m_info(path, deep=True)
    assert (info["width"], info["height"], info["frames"], info["chroma"], info["depth"], info["full_range"]) == (w, h, 3, "420p10", 10, True)
    got = native.read_y4m(path, deep=True)
    assert (got == frames).all() and (got.view("<u2") == codes).all()
    assert (native.read_y4m(path, 1, 1, deep=True)[0] == frames[1]).all()
    # the 8-bit reader refuses the file as before, and the deep reader reads 8-bit files
    with pytest.raises(ValueError, match="4:2:0"):
        native.read_y4m_info(path)
    plain = str(tmp_path / "plain.y4m")
    native.write_y4m(plain, frames[:, :n], w, h)
    assert native.read_y4m_info(plain, deep=True)["depth"] == 8 and (native.read_y4m(plain, deep=True) == frames[:, :n]).all()
    # frames shorter than a 10-bit frame are refused before the file is made
    with pytest.raises(ValueError, match="frame"):
        native.write_y4m(str(tmp_path / "short.y4m"), np.ascontiguousarray(frames[:, :2 * n - 1]), w, h, depth=10)
    assert not os.path.exists(tmp_path / "short.y4m")
    with pytest.raises(ValueError, match="8 or 10"):
        native.write_y4m(str(tmp_path / "twelve.y4m"), frames, w, h, depth=12)
    # auto siting: the tag carries none and is read left-sited
    assert native.y4m_input_siting("420p10", "auto") == "left" and native.y4m_input_siting("420p10", "centre") == "centre"


def test_loader_refuses_mixed_depths(native, tmp_path):
    w, h = 6, 4
    n = ref.sizes(w, h)[2]
    d = tmp_path / "mixed"
    d.mkdir()
    native.write_y4m(str(d / "0_0.y4m"), np.zeros((2, n), np.uint8), w, h)
    native.write_y4m(str(d / "0_1.y4m"), np.zeros((2, 2 * n), np.uint8), w, h, depth=10)
    with pytest.raises(RuntimeError, match="10-bit"):
        native.load_grid_y4m(str(d))


# ---- the command line ---------------------------------------------------------------------------------------------------------------------------------

ARGS = ["--synthetic", "3,3,16,8", "-t", "0,0,1,1", "-m", "STD", "-n", "4", "-b", "1", "-f", "0.0"]


def test_cli_help_lists_the_options(native):
    res = run_cli(native, "-h")
    assert res.returncode == 0
    for word in ("--yuv-depth 8|10", "--p010 FILE", "C420p10", "-f rawvideo -pix_fmt p010le", "-chroma_sample_location"):
        assert word in res.stdout, word


@pytest.mark.parametrize("extra,word", [
    (["--yuv-depth", "12", "--y4m", "v.y4m"], "--yuv-depth expects 8 or 10"),
    (["--yuv-depth", "10"], "--yuv-depth belongs"),
    (["--p010", ""], "--p010 needs the name"),
    (["--yuv-depth", "10", "--rgbd-y4m", "d.y4m", "-r", "0.3"], "10-bit RGB-D frames are not supported"),
])
def test_cli_usage_errors(native, tmp_path, extra, word):
    extra = [str(tmp_path / e) if e.endswith(".y4m") else e for e in extra]
    res = run_cli(native, *ARGS, "-o", str(tmp_path / "out"), *extra)
    assert res.returncode != 0 and word in res.stderr, (res.stdout, res.stderr)
    assert not (tmp_path / "out").exists() and not (tmp_path / "v.y4m").exists() and not (tmp_path / "d.y4m").exists()
