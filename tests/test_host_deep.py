"""CPU: deep views (LFI_FLAG_DEEP_VIEWS, LFI_YUV_DEEP: include/lfi.h) — the coefficient tables against their rule, the brackets against the header's
bounds, the fixed points of the conversion, the surface checks for the three new formats and their neighbours, the command line's usage errors,
what the compiler made of the new kernels, and, on the oracle alone, how often the TEN_WM contract leaves a code two values."""
import itertools
import os
import re

import numpy as np
import pytest

import code_object
import deep_ref as ref
import ten_interval
import yuv10_ref
from view_rows import run_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMAT_IDS = [f"{'709' if m == ref.BT709 else '601'}-{'limited' if r == ref.LIMITED else 'full'}" for m, r in ref.FORMATS]


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ref.FORMATS, ids=FORMAT_IDS)
def test_table_equals_its_rule_and_sums_as_stated(fmt):
    ky, kb, kr, y_off = ref.TABLE[fmt]
    assert (ky, kb, kr, y_off) == ref.rule(*fmt)
    assert sum(ky) == ref.Y_SUM[fmt[1]] and sum(kb) == 0 and sum(kr) == 0
    assert y_off == (64 if fmt[1] == ref.LIMITED else 0)


def test_full_range_sets_are_the_8_bit_ones():
    import yuv_ref
    for m in (ref.BT709, ref.BT601):
        assert ref.TABLE[(m, ref.FULL)][:3] == tuple(tuple(r) for r in yuv_ref.TABLE[(m, yuv_ref.FULL)][:3])


def test_header_and_kernel_source_hold_the_literals():
    header = open(os.path.join(ROOT, "include", "lfi.h")).read()
    source = open(os.path.join(ROOT, "lfinterpolator_amd", "csrc", "hip", "deep_yuv.hpp")).read()
    for (ky, kb, kr, y_off) in ref.TABLE.values():
        row = r"\s+".join(r",\s*".join(str(v) for v in k) for k in (ky, kb, kr)) + rf"\s+{y_off}\b"
        assert re.search(row, header), (ky, kb, kr)
        lit = r"\{\{" + r"\},\s*\{".join(r",\s*".join(str(v) for v in k) for k in (ky, kb, kr)) + r"\},\s*" + str(y_off) + r"\}"
        assert re.search(lit, source), (ky, kb, kr)
    for word in ("#define LFI_YUV_DEEP 0x200", "LFI_FLAG_DEEP_VIEWS = 64u", "LFI_POISON_DEEP = 64", "LFI_YUV_GBRP10 = 4 | LFI_YUV_10BIT | LFI_YUV_DEEP"):
        assert word in header, word


@pytest.mark.parametrize("fmt", ref.FORMATS, ids=FORMAT_IDS)
def test_brackets_stay_inside_their_bounds(fmt):
    """every corner of the cube of codes in every arrangement of the sums (the brackets are linear in each sum: their extremes lie at corners), and
    random codes; the upper ends of the chroma bounds are reached, by full-range pure blue and pure red"""
    ky, kb, kr, _ = ref.TABLE[fmt]
    corners = np.array(list(itertools.product((0, 1023), repeat=3)), np.int64)
    rng = np.random.default_rng(7)
    rgb = np.concatenate([corners, rng.integers(0, 1024, (4096, 3))])
    b = ref.luma_bracket(rgb, *fmt)
    assert b.min() >= 0 and b.max() < ref.LUMA_BOUND
    peak = {}
    for siting, weight in ((ref.CENTRE, 4), (ref.LEFT, 8)):
        s = np.concatenate([weight * corners, rng.integers(0, weight * 1023 + 1, (4096, 3))])
        for k in (kb, kr):
            c = ref.chroma_bracket(k, s, siting)
            assert c.min() > 0 and c.max() <= ref.CHROMA_BOUND[siting], (siting, k, int(c.min()), int(c.max()))
            peak[siting] = max(peak.get(siting, 0), int(c.max()))
    print(fmt, "largest chroma brackets", peak)
    if fmt[1] == ref.FULL:
        assert peak == ref.CHROMA_BOUND


@pytest.mark.parametrize("fmt", ref.FORMATS, ids=FORMAT_IDS)
def test_greys_and_the_ends_of_the_ranges(fmt):
    d = np.arange(1024)
    grey = np.stack([d, d, d], axis=-1)
    _, kb, kr, _ = ref.TABLE[fmt]
    for siting, weight in ((ref.CENTRE, 4), (ref.LEFT, 8)):
        assert (ref.chroma(kb, weight * grey, siting) == 512).all() and (ref.chroma(kr, weight * grey, siting) == 512).all()
    y = ref.luma(grey, *fmt)
    if fmt[1] == ref.LIMITED:
        assert y[0] == 64 and y[1023] == 940 and (np.diff(y) >= 0).all()
    else:
        assert (y == d).all()
    # a frame of one grey under both sitings, odd sizes: the replicated edges change nothing
    view = np.full((5, 7, 3), 600, np.int64)
    for siting in (ref.CENTRE, ref.LEFT):
        c = ref.codes(view, *fmt, siting)
        assert (c[:35] == ref.luma(view[0, 0], *fmt)).all() and (c[35:] == 512).all()


def test_q10_is_the_ten_wm_byte_with_two_more_bits():
    s = np.concatenate([np.linspace(0.0, 300.0, 200001), np.random.default_rng(3).uniform(0, 256, 100000)])
    code = ref.q10_ten(s)
    assert (code >> 2 == ten_interval.quantise(s)).all() and (np.diff(ref.q10_ten(np.sort(s)).astype(int)) >= 0).all() and code.max() == 1023
    pre = np.array([0.0, 0.124, 0.125, 0.375, 0.625, 254.875, 255.75, 255.874, 255.875, 300.0], np.float32)   # x.125 ties go to even
    assert ref.q10_std(pre).tolist() == [0, 0, 0, 2, 2, 1020, 1023, 1023, 1023, 1023]


def test_gbrp10_packing():
    deep = np.random.default_rng(5).integers(0, 1024, (2, 3, 4, 3)).astype(np.uint16)
    planes = ref.gbrp10(deep)
    assert planes.shape == (2, 3, 3, 4) and (planes[:, 0] == deep[..., 1]).all() and (planes[:, 1] == deep[..., 2]).all() and (planes[:, 2] == deep[..., 0]).all()
    raw = ref.gbrp10_bytes(deep, 16, 64, 32, 192, 320, 0xA5)
    assert raw[0, 0] == deep[0, 0, 0, 1] & 0xFF and raw[0, 1] == deep[0, 0, 0, 1] >> 8 and raw[0, 8] == 0xA5 and raw[1, 192 + 32] == deep[1, 1, 0, 0] & 0xFF


# ---- the surface checks ---------------------------------------------------------------------------------------------------------------------------

def _desc(native, fmt, w, h, base=0x1000):
    return native.yuv_surfaces_packed(fmt, "host", base, w, h)


def test_check_accepts_the_new_layout_and_refuses_the_source_flag_and_the_neighbours(native):
    """LFI_YUV_GBRP10 is a layout and is known to the two context-free calls.  LFI_YUV_DEEP on I010 / P010 is a SOURCE flag: the surfaces are
    described as I010 / P010 and the flag is set for lfi_download_views_yuv (tests/test_gpu_deep.py); for the calls that know no source 0x300 and
    0x301 stay the unknown formats tests/test_host_yuv10.py holds 0x300 to"""
    w, h = 18, 5
    g = _desc(native, ref.GBRP10, w, h)
    assert g.check(w, h, 1) and g.check(w, h, 3)
    assert (g.format, g.frame_stride, g.y_pitch, g.c_offset, g.c_pitch, g.cr_offset) == (ref.GBRP10, 6 * w * h, 2 * w, 2 * w * h, 2 * w, 4 * w * h)
    assert native.yuv_surfaces_packed("gbrp10", "device", None, w, h).format == ref.GBRP10
    for fmt, plain in ((ref.I010_DEEP, yuv10_ref.I010), (ref.P010_DEEP, yuv10_ref.P010)):
        p = _desc(native, plain, w, h)
        assert p.check(w, h, 3)
        p.format |= ref.DEEP
        assert p.format == fmt and not p.check(w, h, 3)
    for fmt in (ref.I010_DEEP, ref.P010_DEEP, 2, 0x102, 0x200, 0x201, 0x204, 0x104):
        with pytest.raises(native.LfiError):
            _desc(native, fmt, w, h)
        d = native.YuvSurfaces.make(fmt, "host", 0x1000, g.frame_stride, g.y_pitch, g.c_offset, g.c_pitch, g.cr_offset)
        assert not d.check(w, h, 1), hex(fmt)


def test_gbrp10_geometry_is_checked(native):
    w, h = 18, 5
    tight = dict(frame_stride=6 * w * h, y_pitch=2 * w, c_offset=2 * w * h, c_pitch=2 * w, cr_offset=4 * w * h)

    def ok(n=1, base=0x1000, **kw):
        return native.YuvSurfaces.make(ref.GBRP10, "host", base, **{**tight, **kw}).check(w, h, n)
    assert ok() and ok(n=2) and ok(y_pitch=64, c_offset=64 * h, c_pitch=48, cr_offset=64 * h + 48 * h)
    assert not ok(y_pitch=2 * w - 2)                        # a pitch below 2·W
    assert not ok(c_pitch=2 * w - 2)
    assert not ok(c_offset=2 * w * h - 2)                   # B overlaps G
    assert not ok(cr_offset=4 * w * h - 2)                  # R overlaps B: the planes are full size
    assert not ok(base=0x1001) and not ok(y_pitch=2 * w + 1, c_offset=(2 * w + 1) * h + 1)   # odd addresses
    assert not ok(n=2, frame_stride=6 * w * h - 2)          # the stride below the frame's extent


# ---- the command line -------------------------------------------------------------------------------------------------------------------------------

ARGS = ["--synthetic", "3,3,16,8", "-t", "0,0,1,1", "-m", "TEN_WM", "-n", "4", "-b", "1", "-f", "0.2"]


def test_cli_help_lists_the_options(native):
    res = run_cli(native, "-h")
    assert res.returncode == 0
    for word in ("--deep", "--gbrp10 FILE", "-f rawvideo -pix_fmt gbrp10le", "without a first quantisation"):
        assert word in res.stdout, word


@pytest.mark.parametrize("extra,word", [
    (["-r", "0.3"], "-r above 0"),
    (["-F", "0.4"], "-F"),
    (["-c"], "-c (view-centred"),
    (["-c", "-r", "0.3", "--view-maps"], "cannot be combined"),
    (["-g", "2"], "-g above 1"),
    (["--nv12", "v.nv12"], "--nv12 (an 8-bit video"),
    (["--y4m", "v.y4m"], "--y4m at 8 bits"),
    (["--y4m", "v.y4m", "--yuv-depth", "8"], "--y4m at 8 bits"),
    (["-q", "2,2", "--quilt-y4m", "q.y4m"], "--quilt-y4m"),
    (["-r", "0.3", "--rgbd-y4m", "d.y4m"], "cannot be combined"),
])
def test_cli_usage_errors_come_back_without_a_gpu(native, tmp_path, extra, word):
    extra = [str(tmp_path / e) if "." in e and not e[0].isdigit() else e for e in extra]
    res = run_cli(native, *ARGS, "-o", str(tmp_path / "out"), "--deep", *extra)
    assert res.returncode != 0 and "--deep" in res.stderr and word in res.stderr, (res.stdout, res.stderr)
    assert not (tmp_path / "out").exists() and not list(tmp_path.glob("*.y4m")) and not list(tmp_path.glob("*.nv12"))


def test_gbrp10_needs_deep(native, tmp_path):
    res = run_cli(native, *ARGS, "-o", str(tmp_path / "out"), "--gbrp10", str(tmp_path / "v.raw"))
    assert res.returncode != 0 and "--gbrp10" in res.stderr and "--deep" in res.stderr
    res = run_cli(native, *ARGS, "-o", str(tmp_path / "out"), "--deep", "--gbrp10", "")
    assert res.returncode != 0 and "--gbrp10 needs the name" in res.stderr
    assert not (tmp_path / "out").exists() and not (tmp_path / "v.raw").exists()


# ---- the code object -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not code_object.have_tools(), reason="ROCm LLVM tools not installed")
def test_deep_kernels_exist_and_fit(native):
    """deep_blend twice (STD, TEN_WM), deep_convert10 and deep_convert10_left twice each (I010, P010): no scratch, no spills; the convert kernels
    no LDS and no atomics either; the TEN_WM blend on the matrix cores, the STD one not; the stems that existing tests count keep their counts"""
    kernels = code_object.kernels(native.build.HIP_LIB)
    bodies = code_object.bodies(native.build.HIP_LIB)
    for stem, count in (("deep_blend", 2), ("deep_convert10", 2), ("deep_convert10_left", 2)):
        found = code_object.named(kernels, stem)
        assert len(found) == count, (stem, sorted(found))
        for k, r in found.items():
            assert r[".private_segment_fixed_size"] == 0 and r[".vgpr_spill_count"] == 0 and r[".sgpr_spill_count"] == 0, (k, r)
            assert "scratch_" not in bodies[k], k
            if stem != "deep_blend":
                assert r[".group_segment_fixed_size"] == 0 and r[".vgpr_count"] <= 128, (k, r)
                assert "atomic" not in bodies[k] and "ds_read" not in bodies[k] and "ds_write" not in bodies[k], k
    blends = code_object.named(bodies, "deep_blend")
    ten = [k for k in blends if "ILb0E" in k][0]
    std = [k for k in blends if "ILb1E" in k][0]
    assert "v_mfma_f32_16x16x32_f16" in blends[ten] and "v_mfma" not in blends[std]
    assert any(op in blends[std] for op in ("v_pk_fma_f32", "v_fma_f32", "v_fmac_f32"))   # the chain: IEEE fused multiply-adds, one per image
    for k in blends:
        assert "global_load_lds_dwordx4" in blends[k], k
    for k in code_object.named(bodies, "deep_convert10_left"):
        assert "row_shr:1" in bodies[k] or "wave_shr:1" in bodies[k], k
    # what existing tests count
    for stem in ("yuvs_convert10", "yuvs_convert10_left", "yuvs_expand10", "yuvs_convert", "yuvs_expand"):
        assert len(code_object.named(kernels, stem)) == 4, stem
    assert len(code_object.named(kernels, "yuvs_expand_left")) == 2 and len(code_object.named(kernels, "yuvs_expand10_left")) == 2
    pipelined = ("blend_p3", "blend_planar", "blend_persist", "blend_wave", "blend_stdx", "blend_afs")
    assert not [k for k in kernels if "deep_" in k and any(s in k for s in pipelined)]
    assert not [k for k in kernels if "deep" in k and ("yuvs_expand" in k or "yuvs_convert" in k)]


# ---- the TEN_WM contract on the oracle alone ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ref.CASES, ids=ref.CASE_IDS)
def test_few_codes_have_two_admissible_values(case, native, oracle_c):
    """for the inputs tests/test_gpu_deep.py renders: the interval [q10(S − ε), q10(S + ε)] of the exact sum S (blend_f64) under the accumulation
    bound ε (tests/ten_interval.epsilon) holds two values for at most 10 % of the codes, and never more than two"""
    hp, lf = ref.inputs(native, oracle_c, case)
    S, eps = ten_interval.exact_sums(oracle_c, lf, hp)
    lo, hi = ref.interval10(S, eps)
    width = hi.astype(int) - lo.astype(int)
    share = float((width > 0).mean())
    print(case[0], f"codes with two admissible values: {100 * share:.2f} %, eps {eps.max():.3g}")
    assert width.min() >= 0 and width.max() <= 1, (case[0], int(width.max()))
    assert share <= 0.10, (case[0], share)
