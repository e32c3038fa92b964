"""CPU: the host side of native lenticular images (lfi_download_native) — the numpy restatement (tests/native_ref.py) against the definition as
written and against the properties that follow from it; the coverage of the cases the GPU test shares; the calibration function
(csrc/host/lenticular.cpp through lfi_host_lenticular) against its restatement in Python floats, bit for bit; the exported symbols, the CLI's
checks and the new kernel's code object."""

import numpy as np
import pytest

import code_object
import native_ref as ref
import scaled_quilt_ref as quilt_ref
from view_rows import run_cli


def _views(seed, n=ref.V, w=ref.W, h=ref.H):
    views = np.random.default_rng(seed).integers(0, 256, (n, h, w, 4), dtype=np.uint8)
    views[..., 3] = 255
    return views


VIEWS = _views(15)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps", sorted(ref.STEPS))
@pytest.mark.parametrize("tile,out,n,v0,invert", [((50, 22), (7, 5), 10, 0, False), ((17, 9), (9, 4), 3, 7, True), ((1, 1), (3, 2), 1, 4, False),
                                                  ((25, 11), (31, 13), 8, 1, True)])
def test_restatement_equals_the_definition_as_written(steps, tile, out, n, v0, invert):
    lens = ref.Lens(*ref.STEPS[steps], n, ref.INVERT if invert else 0)
    assert (ref.native(VIEWS, lens, v0, *out, *tile) == ref.native_slow(VIEWS, lens, v0, *out, *tile)).all()


@pytest.mark.parametrize("tile,out", [((17, 9), (7, 5)), ((17, 9), (64, 36)), ((25, 11), (25, 11)), ((50, 22), (131, 67)), ((1, 1), (4, 3))])
def test_one_view_is_the_nearest_resample_of_the_scaled_view(tile, out):
    """n = 1: every subpixel selects the one view, whatever the steps"""
    (tw, th), (ow, oh) = tile, out
    for steps in ref.STEPS.values():
        got = ref.native(VIEWS, ref.Lens(*steps, 1), 4, ow, oh, tw, th)
        scaled = quilt_ref.resize(VIEWS[4], tw, th)
        ys = [((2 * y + 1) * th) // (2 * oh) for y in range(oh)]
        xs = [((2 * x + 1) * tw) // (2 * ow) for x in range(ow)]
        assert (got == scaled[np.ix_(ys, xs)]).all()


def test_one_view_at_the_views_size_is_the_view():
    for v in (0, 4, 9):
        assert (ref.native(VIEWS, ref.Lens(*ref.STEPS["slant"], 1), v, ref.W, ref.H, ref.W, ref.H) == VIEWS[v]).all()


@pytest.mark.parametrize("n", [1, 3, 7, 8, 10])
def test_zero_steps_select_one_view_everywhere(n):
    """x_step = y_step = 0 and phase0 = ⌈k·2³²/n⌉, the smallest phase of view k: view k everywhere; one unit less: view k − 1"""
    for k in range(n):
        p = ref.one_view_phase(k, n)
        assert (ref.select(ref.Lens(0, 0, p, n), 9, 4) == k).all()
        if k:
            assert (ref.select(ref.Lens(0, 0, p - 1, n), 9, 4) == k - 1).all()
        got = ref.native(VIEWS, ref.Lens(0, 0, p, n), 0, 64, 36, 17, 9)
        assert (got == ref.native(VIEWS, ref.Lens(0, 0, 0, 1), k, 64, 36, 17, 9)).all()


@pytest.mark.parametrize("steps", sorted(ref.STEPS))
def test_invert_mirrors_the_views(steps):
    for n in (1, 3, 8, 10):
        lens = ref.Lens(*ref.STEPS[steps], n)
        k, ki = ref.select(lens, 64, 36), ref.select(lens.with_views(n, invert=True), 64, 36)
        assert (ki == n - 1 - k).all()
        # … which is the plain image of the views in reverse order
        assert (ref.native(VIEWS, lens.with_views(n, invert=True), 0, 64, 36, 25, 11) == ref.native(VIEWS[n - 1::-1] if n < ref.V else VIEWS[::-1], lens, 0, 64, 36, 25, 11)).all()


def test_boundaries_are_hit_exactly():
    """n = 8, x_step = 2²⁹: subpixel j has the phase j·2³²/8, exactly the boundary between views j − 1 and j (mod 8) — it belongs to view j;
    one unit of 2⁻³² below (phase0 = 2³² − 1) it belongs to view j − 1.  Both sides of every boundary occur."""
    j = (3 * np.arange(31)[None, :, None] + np.arange(3)[None, None, :]) % 8
    on = ref.select(ref.Lens(*ref.STEPS["boundary"], 8), 31, 5)
    below = ref.select(ref.Lens(*ref.STEPS["below boundary"], 8), 31, 5)
    assert (on == j).all() and (below == (j - 1) % 8).all()
    assert set(np.unique(on)) == set(np.unique(below)) == set(range(8))
    rows = ref.select(ref.Lens(*ref.STEPS["boundary rows"], 8), 31, 5)   # + 3 boundaries per row, from phase ½
    assert (rows == (j + 4 + 3 * np.arange(5)[:, None, None]) % 8).all()


def test_a_negative_slant_wraps():
    """y_step = 2³² − s is a step of −s: the phases equal those of signed arithmetic reduced mod 2³²"""
    xs, ys, p0 = ref.STEPS["negative slant"]
    s = (1 << 32) - ys
    assert 0 < s < 1 << 31
    n, ow, oh = 10, 20, 12
    k = ref.select(ref.Lens(xs, ys, p0, n), ow, oh)
    for y in range(oh):
        for x in range(ow):
            for c in range(3):
                assert k[y, x, c] == (((p0 + (3 * x + c) * xs - y * s) % (1 << 32)) * n) >> 32
    # the rows differ (the slant is seen) and differ from the positive slant's
    assert (k[0] != k[1]).any() and (k != ref.select(ref.Lens(xs, s, p0, n), ow, oh)).any()


@pytest.mark.parametrize("steps", ref.GENERAL)
@pytest.mark.parametrize("out", ref.OUTPUTS)
@pytest.mark.parametrize("n,v0", ref.VIEW_RANGES)
def test_shared_cases_select_every_view_in_every_channel(steps, out, n, v0):
    """what makes the GPU comparison worth its name: with the general step sets every one of the n views is read in every channel, and
    (n ≥ 3) the three channels of some pixel read three different views — by construction of the steps, asserted here"""
    for invert in (False, True):
        k = ref.select(ref.Lens(*ref.STEPS[steps], n, ref.INVERT if invert else 0), *out)
        for c in range(3):
            assert set(np.unique(k[..., c])) == set(range(n)), (c, np.unique(k[..., c]))
        if n >= 3:
            assert ((k[..., 0] != k[..., 1]) & (k[..., 1] != k[..., 2]) & (k[..., 0] != k[..., 2])).any()


# ---- the calibration --------------------------------------------------------------------------------------------------------------------------

def _as_tuple(lens):
    return (lens.x_step, lens.y_step, lens.phase0, lens.views, lens.flags)


def test_calibration_equals_its_restatement_bit_for_bit(native):
    rng = np.random.default_rng(2026)
    cases = [(47.5636, -5.4392, 0.0412, 338.0, False, 2560, 1600, 45), (52.5741, -7.1956, -0.3817, 283.0, True, 3840, 2160, 45),
             (49.8, 5.5, 1.75, 324.0, False, 1536, 2048, 48), (80.0, 6.0, -2.25, 491.0, True, 7680, 4320, 100)]
    for _ in range(40):
        cases.append((float(rng.uniform(20, 120)), float(rng.uniform(2, 12)) * (1 if rng.integers(2) else -1), float(rng.uniform(-3, 3)),
                      float(rng.uniform(90, 600)), bool(rng.integers(2)), int(rng.integers(1, 8000)), int(rng.integers(1, 5000)), int(rng.integers(1, 120))))
    seen_negative = seen_outside = 0
    for case in cases:
        got, want = native.lenticular(*case), ref.calibrate(*case)
        assert _as_tuple(got) == _as_tuple(want), case
        seen_negative += case[1] < 0
        seen_outside += not (0 <= case[2] < 1)
    assert seen_negative >= 5 and seen_outside >= 5
    # a negative slope gives a negative y step: it wraps into the upper half
    assert native.lenticular(47.5636, -5.4392, 0.0412, 338.0, False, 2560, 1600, 45).y_step >= 1 << 31
    assert native.lenticular(47.5636, 5.4392, 0.0412, 338.0, False, 2560, 1600, 45).y_step < 1 << 31


def test_calibration_by_hand(native):
    """slope = 2³⁰: slope² + 1 rounds to slope², so |slope| / sqrt(slope² + 1) is exactly 1 and p = pitch·out_w / dpi.
    pitch = 3·dpi: three lenses per pixel, one per subpixel — x_step = 2³² ≡ 0; tilt = out_h / (out_w·2³⁰), so y_step = 2³²·3·out_w·tilt / out_h
    = 3·2³² / 2³⁰ = 12; phase0 = 2³²·(3·out_w·(½ / out_w + ½ / (out_w·2³⁰)) − center) = 2³²·(3/2 − center) + 6.
    pitch = 3·dpi / 8: x_step = 2²⁹ (the boundary case of the tests), y_step = 12 / 8 = 1.5 → 2 (ties away from zero)."""
    s = float(1 << 30)
    for ow, oh in ((1024, 512), (2048, 2048)):
        lens = native.lenticular(300.0, s, 0.0, 100.0, False, ow, oh, 8)
        assert _as_tuple(lens) == (0, 12, (1 << 31) + 6, 8, 0)
        lens = native.lenticular(300.0, s, 0.25, 100.0, True, ow, oh, 8)
        assert _as_tuple(lens) == (0, 12, (1 << 30) + 6, 8, ref.INVERT)
        lens = native.lenticular(300.0, -s, 0.0, 100.0, False, ow, oh, 8)
        assert _as_tuple(lens) == (0, (1 << 32) - 12, (1 << 31) - 6, 8, 0)
        lens = native.lenticular(37.5, s, 0.0, 100.0, False, ow, oh, 8)
        assert _as_tuple(lens) == (1 << 29, 2, ((3 << 28) + 1) & ref.MASK, 8, 0)   # phase0 = 2³²·3/16 + 0.75 → + 1
    assert _as_tuple(ref.calibrate(300.0, s, 0.0, 100.0, False, 1024, 512, 8)) == (0, 12, (1 << 31) + 6, 8, 0)


@pytest.mark.parametrize("case", [(0.0, 5.0, 0.0, 300.0), (50.0, 0.0, 0.0, 300.0), (50.0, 5.0, 0.0, 0.0), (50.0, 5.0, float("nan"), 300.0),
                                  (float("inf"), 5.0, 0.0, 300.0), (-50.0, 5.0, 0.0, 300.0)])
def test_calibration_refuses_what_is_no_display(native, case):
    with pytest.raises(ValueError, match="calibration"):
        native.lenticular(*case, False, 1920, 1080, 45)
    for size in ((0, 1080, 45), (1920, 0, 45), (1920, 1080, 0)):
        with pytest.raises(ValueError, match="calibration"):
            native.lenticular(50.0, 5.0, 0.0, 300.0, False, *size)


# ---- the library and the command line -----------------------------------------------------------------------------------------------------

def test_symbols_are_exported_and_bound(native):
    lib = native.load_hip_library()
    assert "lfi_download_native" in native.ABI_SYMBOLS and hasattr(lib, "lfi_download_native")
    assert hasattr(native.load_host_library(), "lfi_host_lenticular")
    assert hasattr(native.Context, "download_native") and native.LFI_LENT_INVERT == ref.INVERT == 1
    assert [f[0] for f in native.Lenticular._fields_] == ["x_step", "y_step", "phase0", "views", "flags"]


NATIVE_ARGS = ["--synthetic", "4,4,32,16", "-t", "0,0,1,1", "-m", "STD", "-n", "6", "-b", "1", "-f", "0.0"]


@pytest.mark.parametrize("extra,words", [
    (["--lens", "50,5,0,300"], ("--native", "--lens")),
    (["--native", "64x36"], ("--native", "--lens")),
    (["--native-tile", "16x8"], ("--native-tile", "--native")),
    (["--native-views", "3"], ("--native-views", "--native")),
    (["--native", "64x36", "--lens", "50,5,0,300", "-g", "2"], ("--native", "one GPU")),
])
def test_cli_refuses_before_anything_runs(native, tmp_path, extra, words):
    res = run_cli(native, *NATIVE_ARGS, "-o", str(tmp_path / "out"), *extra)
    assert res.returncode != 0
    for word in words:
        assert word in res.stderr, res.stderr
    assert not (tmp_path / "out").exists()


def test_cli_help_names_the_flags(native):
    res = run_cli(native, "-h")
    assert res.returncode == 0
    for flag in ("--native WxH", "--lens pitch,slope,center,dpi[,invert]", "--native-tile WxH", "--native-views N"):
        assert flag in res.stdout


# ---- the code object --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not code_object.have_tools(), reason="ROCm LLVM tools not installed")
def test_native_interlace_uses_no_scratch_no_lds_and_whole_dword_stores(native):
    """From the code object: both instantiations of native_interlace (csrc/hip/native_image.hpp) exist, use no scratch and no LDS, spill nothing,
    stay at or below 64 registers per lane (eight waves per SIMD), load bytes and store dwords only, and contain no atomic instruction."""
    kernels = code_object.kernels(native.build.HIP_LIB)
    interlace = code_object.named(kernels, "native_interlace")
    assert len(interlace) == 2, sorted(interlace)
    for k, v in interlace.items():
        assert v[".private_segment_fixed_size"] == 0 and v[".vgpr_spill_count"] == 0 and v[".sgpr_spill_count"] == 0, (k, v)
        assert v[".group_segment_fixed_size"] == 0 and v[".vgpr_count"] <= 64, (k, v)
    bodies = {k: v for k, v in code_object.bodies(native.build.HIP_LIB).items() if k in interlace}
    assert set(bodies) == set(interlace)
    for k, text in bodies.items():
        assert "atomic" not in text and "scratch_" not in text and "ds_" not in text, k
        assert text.count("global_load_ubyte") == 3 and text.count("global_store_dword") == 1, k
        assert "global_store_byte" not in text and "global_store_short" not in text, k
