"""CPU: left-sited chroma (lfi_set_yuv_siting, include/lfi.h) — the header's constants and the binding, the properties the header states of
the two definitions (tests/yuv_left_ref.py), what siting costs on a colour ramp, the Y4M tag, and the new kernels' resources."""
import os
import re

import numpy as np
import pytest

import code_object
import yuv_in_ref as in_ref
import yuv_left_ref as left
import yuv_ref as out_ref


# ---- the interface ------------------------------------------------------------------------------------------------------------------------------

def test_header_constants_equal_the_bindings(native):
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "lfi.h")).read()
    m = re.search(r"enum \{ LFI_YUV_SITING_CENTRE = (\d+), LFI_YUV_SITING_LEFT = (\d+) \};", text)
    assert m and (int(m.group(1)), int(m.group(2))) == (native.LFI_YUV_SITING_CENTRE, native.LFI_YUV_SITING_LEFT) == (0, 1)
    assert native.YUV_SITINGS == {"centre": native.LFI_YUV_SITING_CENTRE, "left": native.LFI_YUV_SITING_LEFT}
    assert re.search(r"int lfi_set_yuv_siting\(lfi_ctx \*ctx, int in_siting, int out_siting\);", text)
    assert re.search(r"int lfi_yuv_siting\(lfi_ctx \*ctx, int \*in_siting, int \*out_siting\);", text)
    lib = native.load_hip_library()
    for name in ("lfi_set_yuv_siting", "lfi_yuv_siting"):
        assert name in native.ABI_SYMBOLS and hasattr(lib, name)
    assert hasattr(native.Context, "set_yuv_siting") and hasattr(native.Context, "yuv_siting")
    # without a context both calls refuse and touch nothing
    a, b = np.full(1, 7, np.int32), np.full(1, 7, np.int32)
    assert lib.lfi_set_yuv_siting(None, 0, 0) == -1
    assert lib.lfi_yuv_siting(None, a.ctypes.data_as(lib.lfi_yuv_siting.argtypes[1]), b.ctypes.data_as(lib.lfi_yuv_siting.argtypes[2])) == -1
    assert a[0] == 7 and b[0] == 7


# ---- output: the bracket, greys, uniform images ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", out_ref.FORMATS)
def test_output_bracket_stays_in_u32(fmt):
    """analytically: each of ΣR, ΣG, ΣB is 0 or 8·255 = 2040 at an extreme — the positive coefficients at 2040 and the negative at 0, and the
    other way round; over all four rows the extremes are 524,288 and 134,217,728 = 2²⁷, inside (0, 2²⁸]"""
    _, kb, kr, _ = out_ref.TABLE[fmt]
    for k in (kb, kr):
        hi = (1 << 26) + (1 << 18) + 2040 * sum(c for c in k if c > 0)
        lo = (1 << 26) + (1 << 18) + 2040 * sum(c for c in k if c < 0)
        assert 0 < lo and hi <= 1 << 28
        assert 524_288 <= lo and hi <= 134_217_728
        # limited range: [16, 240]; full range reaches 256 before the min
        assert (lo >> 19, hi >> 19) == ((16, 240) if fmt[1] == out_ref.LIMITED else (1, 256))
    los = [(1 << 26) + (1 << 18) + 2040 * sum(c for c in k if c < 0) for f in out_ref.FORMATS for k in out_ref.TABLE[f][1:3]]
    his = [(1 << 26) + (1 << 18) + 2040 * sum(c for c in k if c > 0) for f in out_ref.FORMATS for k in out_ref.TABLE[f][1:3]]
    assert min(los) == 524_288 and max(his) == 134_217_728


@pytest.mark.parametrize("fmt", out_ref.FORMATS)
def test_output_over_the_corner_views(fmt):
    """yuv_ref.corner_views(128, 66, 3): the cube's corners in every 2 x 2 arrangement.  `planes` asserts the bracket's interval itself"""
    views = out_ref.corner_views(128, 66, 3)
    lo, hi = 255, 0
    for v in views:
        y, cb, cr = left.planes(v, *fmt, clamp=False)
        assert (y == out_ref.planes(v, *fmt)[0]).all()          # luma does not move
        lo, hi = min(lo, cb.min(), cr.min()), max(hi, cb.max(), cr.max())
    # the left filter reaches into the block on its left, so these views need not reach the extremes: inside them
    bound = (16, 240) if fmt[1] == out_ref.LIMITED else (1, 256)
    assert bound[0] <= lo and hi <= bound[1]


@pytest.mark.parametrize("fmt", out_ref.FORMATS)
def test_greys_give_128_and_uniform_images_the_centre_sited_frame(fmt):
    rng = np.random.default_rng(5)
    grey = np.repeat(rng.integers(0, 256, (9, 13, 1), dtype=np.uint8), 4, axis=2)     # a different grey per pixel
    _, cb, cr = left.planes(grey, *fmt)
    assert (cb == 128).all() and (cr == 128).all()
    for colour in [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (12, 200, 99), (255, 0, 255)]:
        img = np.empty((5, 7, 4), np.uint8)
        img[...] = (*colour, 255)
        assert (left.frame(img, *fmt) == out_ref.frame(img, *fmt)).all(), colour


def test_output_by_hand():
    """3 x 3, BT.601 full, one red pixel at (1, 0): chroma column 0 sees it at xr with weight 1, column 1 at xl with weight 1"""
    img = np.zeros((3, 3, 4), np.uint8)
    img[0, 1, 0] = 255
    _, cb, cr = left.planes(img, out_ref.BT601, out_ref.FULL)
    assert cr[0, 0] == cr[0, 1] == ((1 << 26) + (1 << 18) + 32768 * 255) >> 19
    assert cb[0, 0] == ((1 << 26) + (1 << 18) - 11058 * 255) >> 19
    assert cr[1, 0] == cr[1, 1] == 128
    # … and at (0, 0): xl = xc = 0, weight 3 in column 0, none in column 1 (its xl is column 1)
    img = np.zeros((3, 3, 4), np.uint8)
    img[0, 0, 0] = 255
    _, cb, cr = left.planes(img, out_ref.BT601, out_ref.FULL)
    assert cr[0, 0] == ((1 << 26) + (1 << 18) + 32768 * 3 * 255) >> 19 and cr[0, 1] == 128
    # the last column of an odd width: xc = xr = 2, xl = 1
    img = np.zeros((3, 3, 4), np.uint8)
    img[2, 2, 2] = 255                                                   # blue, last row too: replicated into both rows of the sample
    _, cb, cr = left.planes(img, out_ref.BT601, out_ref.FULL)
    assert cb[1, 1] == ((1 << 26) + (1 << 18) + 32768 * 2 * 3 * 255) >> 19


# ---- input ----------------------------------------------------------------------------------------------------------------------------------------

def test_nearest_input_is_siting_independent_and_bilinear_by_hand():
    w, h = 7, 5
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (3, in_ref.sizes(w, h)[2]), dtype=np.uint8)
    for fmt in in_ref.FORMATS:
        assert (left.images(frames, w, h, *fmt, in_ref.NEAREST) == in_ref.images(frames, w, h, *fmt, in_ref.NEAREST)).all()
    # a uniform chroma plane gives 16·U under both sitings
    plane = np.full((3, 4), 77, np.int64)
    assert (left.chroma16(plane, w, h, in_ref.BILINEAR) == 16 * 77).all()
    # by hand: U = [[0, 16, 32, 48]] · one row (ch = 1): even x is its own sample, odd x the mean of two, the last odd column clamps
    plane = np.array([[0, 16, 32, 48]], np.int64)
    assert left.chroma16(plane, 8, 1, in_ref.BILINEAR).tolist() == [[0, 128, 256, 384, 512, 640, 768, 768]]
    # rows: 3·h(cy) + h(ny), ny above an even row and below an odd one, clamped
    plane = np.array([[0], [64]], np.int64)
    assert left.chroma16(plane, 1, 4, in_ref.BILINEAR)[:, 0].tolist() == [0, 4 * 64, 3 * 4 * 64, 16 * 64]


# ---- what siting costs: a colour ramp ---------------------------------------------------------------------------------------------------------------

def _ramp():
    x = np.arange(28)
    img = np.empty((6, 28, 4), np.uint8)
    img[..., 0], img[..., 1], img[..., 2], img[..., 3] = 8 * x + 10, 128, 250 - 8 * x, 255
    return img


@pytest.mark.parametrize("fmt", out_ref.FORMATS)
def test_siting_ramp(fmt):
    """28 x 6, R = 8x + 10, G = 128, B = 250 − 8x, columns 2 … 25: frames made and read under the same siting come back within 2 code values
    per channel; under mismatched siting they are at least 5 off.  The thresholds are what the two definitions give (printed), not tolerances
    of any kernel: the chroma of a ramp sampled at one place and read as if at another is off by a quarter pixel of slope"""
    img = _ramp()
    w, h = 28, 6
    made = {"left": left.frame(img, *fmt), "centre": out_ref.frame(img, *fmt)}
    read = {"left": lambda f: left.rgba(f, w, h, *fmt), "centre": lambda f: in_ref.rgba(f, w, h, *fmt)}
    worst = {}
    for out_site in made:
        for in_site in read:
            back = read[in_site](made[out_site]).astype(np.int64)
            worst[(out_site, in_site)] = int(np.abs(back[:, 2:26, :3] - img[:, 2:26, :3].astype(np.int64)).max())
    print(fmt, worst)
    assert worst[("left", "left")] <= 2 and worst[("centre", "centre")] <= 2
    assert worst[("left", "centre")] >= 5 and worst[("centre", "left")] >= 5


# ---- Y4M ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("full", [False, True])
def test_y4m_writer_tags_left_sited_frames(native, tmp_path, full):
    w, h, n = 17, 9, 2
    size = out_ref.sizes(w, h)[2]
    frames = np.random.default_rng(3).integers(0, 256, (n, size + 3), dtype=np.uint8)
    a, b, c = tmp_path / "a.y4m", tmp_path / "b.y4m", tmp_path / "c.y4m"
    native.write_y4m(str(a), frames, w, h, fps=(25, 1), full_range=full)
    native.write_y4m(str(b), frames, w, h, fps=(25, 1), full_range=full, left_sited=False)
    native.write_y4m(str(c), frames, w, h, fps=(25, 1), full_range=full, left_sited=True)
    head = f"YUV4MPEG2 W{w} H{h} F25:1 Ip A1:1 C420%s XCOLORRANGE={'FULL' if full else 'LIMITED'}\n"
    assert a.read_bytes() == b.read_bytes() and a.read_bytes().startswith((head % "jpeg").encode())        # unchanged bytes otherwise
    assert c.read_bytes() == (head % "mpeg2").encode() + a.read_bytes()[len(head % "jpeg"):]               # only the tag differs
    info = native.read_y4m_info(str(c))
    assert (info["chroma"], info["centre_sited"], info["frames"]) == ("420mpeg2", False, n)
    assert (native.read_y4m(str(c)) == frames[:, :size]).all()


def test_y4m_reader_resolves_the_siting_per_tag(native):
    want = {"420mpeg2": "left", "420jpeg": "centre", "420paldv": "centre", "420": "centre"}
    for tag, auto in want.items():
        assert native.y4m_input_siting(tag, "auto") == auto
        assert native.y4m_input_siting(tag, "centre") == "centre" and native.y4m_input_siting(tag, "left") == "left"
    host = native.load_host_library()
    assert host.lfi_host_y4m_input_siting(None, 2) == -1 and host.lfi_host_y4m_input_siting(b"420jpeg", 3) == -1


def test_cli_help_and_refusals(native, tmp_path):
    from test_host_yuv import Y4M_ARGS, run_cli
    res = run_cli(native, "-h")
    assert res.returncode == 0
    for flag in ("--chroma-site centre|left", "--in-chroma-site centre|left|auto"):
        assert flag in res.stdout
    out = tmp_path / "out"
    for extra, words in [
        (["--y4m", str(tmp_path / "v.y4m"), "--chroma-site", "top"], ("--chroma-site", "centre", "left")),
        (["--chroma-site", "left"], ("--chroma-site", "--y4m")),
        (["--rgbd-y4m", str(tmp_path / "v.y4m"), "-r", "0.1", "--chroma-site", "left"], ("--chroma-site left", "--rgbd-y4m")),
        (["--in-chroma-site", "auto"], ("--in-chroma-site", ".y4m")),
    ]:
        res = run_cli(native, *Y4M_ARGS, "-o", str(out), *extra)
        assert res.returncode != 0, extra
        for word in words:
            assert word in res.stderr, (extra, res.stderr)
        assert not out.exists() and not (tmp_path / "v.y4m").exists()
    # a directory of images is no light-field video; an unknown value is refused before anything is opened
    res = run_cli(native, "-i", str(tmp_path), "-t", "0,0,1,1", "-m", "STD", "-o", str(out), "--in-chroma-site", "top")
    assert res.returncode != 0 and "--in-chroma-site" in res.stderr and "auto" in res.stderr


# ---- the code object --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not code_object.have_tools(), reason="ROCm LLVM tools not installed")
def test_left_sited_kernels_exist_and_fit(native):
    """yuvs_convert_left<PLANAR, FORMAT> four times, yuvs_expand_left<FORMAT> and yuvs_derived_expand_left<FORMAT> twice each (a left-sited
    nearest upload is the nearest kernel); no scratch, no spills, at most 128 registers; no LDS in the first two, at most 16 KiB in the
    third; the conversion takes its one value from the neighbour lane with ONE cross-lane move and stores exactly what yuvs_convert stores"""
    kernels = code_object.kernels(native.build.HIP_LIB)
    bodies = code_object.bodies(native.build.HIP_LIB)
    expect = {"yuvs_convert_left": ("ILb0ELi0E", "ILb0ELi1E", "ILb1ELi0E", "ILb1ELi1E"), "yuvs_expand_left": ("ILi0E", "ILi1E"),
              "yuvs_derived_expand_left": ("ILi0E", "ILi1E")}
    for stem, variants in expect.items():
        found = code_object.named(kernels, stem)
        assert len(found) == len(variants), (stem, sorted(found))
        for v in variants:
            assert sum(f"{stem}{v}" in k for k in found) == 1, (stem, v, sorted(found))
        for k, r in found.items():
            assert r[".private_segment_fixed_size"] == 0 and r[".vgpr_spill_count"] == 0 and r[".sgpr_spill_count"] == 0, (k, r)
            assert r[".vgpr_count"] <= 128, (k, r)
            if stem == "yuvs_derived_expand_left":
                assert 0 < r[".group_segment_fixed_size"] <= 16 << 10, (k, r)
            else:
                assert r[".group_segment_fixed_size"] == 0, (k, r)
            text = bodies[k]
            assert "scratch_" not in text and "atomic" not in text, k
    centre = {k[len("_ZN3lfi12yuvs_convert"):]: v for k, v in code_object.named(bodies, "yuvs_convert").items()}
    for k in code_object.named(kernels, "yuvs_convert_left"):
        text = bodies[k]
        moves = len(re.findall(r"_dpp|ds_bpermute|ds_permute|ds_swizzle|v_permlane|v_readlane", text))
        assert moves == 1, (k, moves)
        assert "ds_read" not in text and "ds_write" not in text, k
        twin = centre[k[len("_ZN3lfi17yuvs_convert_left"):]]
        for store in ("global_store_byte", "global_store_short", "global_store_dwordx2", "global_store_dwordx4"):
            assert text.count(store) == twin.count(store), (k, store)
        assert len(re.findall(r"global_store_dword ", text)) == len(re.findall(r"global_store_dword ", twin)), k
    for stem in ("yuvs_expand_left", "yuvs_derived_expand_left"):
        twins = code_object.named(bodies, stem[:-len("_left")])
        for k in code_object.named(kernels, stem):
            # one load fewer per chroma row than the centre-sited bilinear kernel: three rows of Cb and Cr (I420), three CbCr rows (NV12)
            fmt = re.search(r"_leftILi([01])E", k).group(1)
            twin = next(v for t, v in twins.items() if f"ILi{fmt}ELb0E" in t)
            loads = lambda text: len(re.findall(r"global_load_", text))
            assert loads(bodies[k]) == loads(twin) - (3 if fmt == "1" else 6), (k, loads(bodies[k]), loads(twin))
