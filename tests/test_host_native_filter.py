"""CPU: the host side of FILTERED native images (LFI_LENT_BGR, LFI_LENT_BILINEAR, LFI_LENT_BLEND of lfi_download_native) — the numpy
restatement (tests/native_filter_ref.py) against the definition as written and against the properties that follow from it; the coverage of
the cases the GPU test shares; the tap arithmetic the kernel runs (csrc/native_taps.h through lfi_host_native_taps) against the definition;
the calibration file (csrc/host/lenticular.cpp through lfi_host_lenticular_json); the exported symbols, the CLI's checks and the new kernel's
code object."""
import functools
import json
import os
import re

import numpy as np
import pytest

import code_object
import native_filter_ref as fref
import native_ref as ref
from conftest import GOLDEN_DIR
from native_filter_ref import BGR, BILINEAR, BLEND
from native_ref import INVERT
from view_rows import run_cli


def _views(seed, n=ref.V, w=ref.W, h=ref.H):
    views = np.random.default_rng(seed).integers(0, 256, (n, h, w, 4), dtype=np.uint8)
    views[..., 3] = 255
    return views


VIEWS = _views(1)


@functools.lru_cache(maxsize=None)
def _tiles(tile):
    """T_v of every view of VIEWS, once per tile size"""
    return ref.tiles(VIEWS, *tile)


def _native(lens, v0, out, tile):
    return fref.native(_tiles(tile), lens, v0, *out, *tile)


# ---- the restatement against itself -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", fref.FLAG_SETS)
@pytest.mark.parametrize("tile,out,n,v0,invert,steps", [((50, 22), (7, 5), 10, 0, False, "slant"), ((17, 9), (9, 4), 3, 7, True, "negative slant"),
                                                        ((1, 1), (3, 2), 1, 4, False, "slant"), ((25, 11), (31, 13), 8, 1, True, "boundary rows"),
                                                        ((17, 9), (40, 3), 2, 0, False, "below boundary")])
def test_restatement_equals_the_definition_as_written(flags, tile, out, n, v0, invert, steps):
    lens = ref.Lens(*ref.STEPS[steps], n, flags | (INVERT if invert else 0))
    assert (fref.native(VIEWS, lens, v0, *out, *tile) == fref.native_slow(VIEWS, lens, v0, *out, *tile)).all()


@pytest.mark.parametrize("steps", sorted(ref.STEPS))
def test_without_the_new_flags_it_is_the_nearest_image(steps):
    for tile, out, n, v0 in (((50, 22), (64, 36), 10, 0), ((17, 9), (131, 67), 3, 7), ((25, 11), (7, 5), 8, 1), ((1, 1), (50, 22), 1, 4)):
        for flags in (0, INVERT):
            lens = ref.Lens(*ref.STEPS[steps], n, flags)
            assert (_native(lens, v0, out, tile) == ref.native(_tiles(tile), lens, v0, *out, *tile)).all()


# ---- what follows from the definition -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps", sorted(ref.STEPS))
def test_bilinear_at_the_tiles_own_size_is_nearest(steps):
    """tile = out: U = 2·x·D/2 … fx = fy = 0 everywhere, and the tap is the nearest pixel"""
    for size in ((50, 22), (17, 9), (1, 1)):
        assert (fref.taps(size[0], size[0])[2] == 0).all() and (fref.taps(size[0], size[0])[0] == np.arange(size[0])).all()
        for n, v0 in fref.VIEW_RANGES:
            for flags in (0, BLEND, INVERT | BGR):
                lens = ref.Lens(*ref.STEPS[steps], n, flags)
                assert (_native(ref.Lens(*ref.STEPS[steps], n, flags | BILINEAR), v0, size, size) == _native(lens, v0, size, size)).all()


def test_a_phase_on_a_views_centre_blends_nothing():
    """n = 8, x_step = 2²⁹, phase0 = 2²⁸: subpixel j has the phase (j + ½)·2³²/8 — f = 128, wb = 0: view k alone"""
    lens = ref.Lens(*fref.CENTRES, 8, BLEND)
    k, f = fref.fractions(lens, 31, 5)
    assert (f == 128).all() and set(np.unique(k)) == set(range(8))
    ka, kb, wb = fref.selection(lens, 31, 5)
    assert (ka == k).all() and (wb == 0).all()
    for tile in ref.TILES:
        for flags in (0, BILINEAR, INVERT | BGR):
            assert (_native(ref.Lens(*fref.CENTRES, 8, flags | BLEND), 1, (64, 36), tile) == _native(ref.Lens(*fref.CENTRES, 8, flags), 1, (64, 36), tile)).all()


def test_a_phase_on_a_boundary_is_the_even_mix():
    """"boundary": f = 0, wb = 128 — the rounded mean of views k − 1 and k (k = 0: of view 0 with itself); "below boundary": f = 255, wb = 127"""
    on = ref.Lens(*ref.STEPS["boundary"], 8, BLEND)
    ka, kb, wb = fref.selection(on, 31, 5)
    k, f = fref.fractions(on, 31, 5)
    assert (f == 0).all() and (wb == 128).all() and (kb == k).all() and (ka == np.maximum(k, 1) - 1).all()
    ka, kb, wb = fref.selection(ref.Lens(*ref.STEPS["below boundary"], 8, BLEND), 31, 5)
    assert (wb == 127).all() and (kb == np.minimum(ka + 1, 7)).all()
    got = _native(on, 1, (31, 5), (50, 22))
    S = fref.samples(VIEWS[1:9], 0, 31, 5)
    y, x, c = np.arange(5)[:, None, None], np.arange(31)[None, :, None], np.arange(3)[None, None, :]
    assert (got[..., :3] == (S[np.maximum(k, 1) - 1, y, x, c] + S[k, y, x, c] + 1) >> 1).all()


@pytest.mark.parametrize("flags", fref.FLAG_SETS)
def test_one_view_is_that_view_and_two_views_blend_once(flags):
    for steps in ref.STEPS.values():
        # n = 1: view v0 under any flags — the sampled view itself
        got = _native(ref.Lens(*steps, 1, flags), 4, (64, 36), (17, 9))
        assert (got[..., :3] == fref.samples(_tiles((17, 9))[4:5], flags, 64, 36)[0]).all() and (got[..., 3] == 255).all()
        # n = 2: the only pair is (0, 1); the outer halves of both views are not blended
        ka, kb, wb = fref.selection(ref.Lens(*steps, 2, flags), 64, 36)
        assert set(np.unique(ka)) <= {0, 1} and set(np.unique(kb)) <= {0, 1}
        if flags & BLEND:
            k, f = fref.fractions(ref.Lens(*steps, 2, flags), 64, 36)
            assert (ka[(k == 0) & (f < 128)] == 0).all() and (kb[(k == 0) & (f < 128)] == 0).all()
            assert (ka[(k == 1) & (f >= 128)] == 1).all() and (kb[(k == 1) & (f >= 128)] == 1).all()
            assert (kb[(k == 0) & (f >= 128)] == 1).all() and (ka[(k == 1) & (f < 128)] == 0).all()


# ---- the coverage of the shared cases -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps", ref.GENERAL)
@pytest.mark.parametrize("out", fref.OUTPUTS)
@pytest.mark.parametrize("n,v0", fref.VIEW_RANGES)
def test_shared_cases_reach_both_clamped_ends_and_blend_two_views(steps, out, n, v0):
    for bgr in (0, BGR):
        lens = ref.Lens(*ref.STEPS[steps], n, BLEND | bgr)
        k, f = fref.fractions(lens, *out)
        assert ((k == 0) & (f < 128)).any() and ((k == n - 1) & (f >= 128)).any(), (out, n)
        ka, kb, wb = fref.selection(lens, *out)
        assert (ka >= 0).all() and (kb <= n - 1).all() and (wb >= 0).all() and (wb <= 255).all()
        if n >= 2:
            assert ((ka != kb) & (wb > 0)).any()


@pytest.mark.parametrize("steps", ref.GENERAL)
@pytest.mark.parametrize("tile", ref.TILES)
def test_shared_cases_change_a_quarter_of_the_bytes(steps, tile):
    """On random views the filters are seen: a kernel that ignored a flag could not pass the GPU comparison.  Both shares are of the
    restatement alone."""
    for out in fref.OUTPUTS:
        for n, v0 in fref.VIEW_RANGES:
            plain = _native(ref.Lens(*ref.STEPS[steps], n, 0), v0, out, tile)[..., :3]
            if n >= 2:
                blended = _native(ref.Lens(*ref.STEPS[steps], n, BLEND), v0, out, tile)[..., :3]
                assert (blended != plain).mean() >= 0.25, (tile, out, n, float((blended != plain).mean()))
            if tile != out and tile != (1, 1):
                bilinear = _native(ref.Lens(*ref.STEPS[steps], n, BILINEAR), v0, out, tile)[..., :3]
                assert (bilinear != plain).mean() >= 0.25, (tile, out, n, float((bilinear != plain).mean()))


@pytest.mark.parametrize("flags", [0, BILINEAR, BLEND, INVERT | BILINEAR | BLEND])
def test_bgr_is_rgb_of_views_with_red_and_blue_swapped(flags):
    swapped = VIEWS[..., [2, 1, 0, 3]]
    for steps in ref.GENERAL:
        for tile, out, n, v0 in (((50, 22), (64, 36), 10, 0), ((17, 9), (131, 67), 3, 7), ((25, 11), (7, 5), 8, 1)):
            got = fref.native(VIEWS, ref.Lens(*ref.STEPS[steps], n, flags | BGR), v0, *out, *tile)
            want = fref.native(swapped, ref.Lens(*ref.STEPS[steps], n, flags), v0, *out, *tile)
            assert (got[..., :3] == want[..., [2, 1, 0]]).all()
            assert (got != fref.native(VIEWS, ref.Lens(*ref.STEPS[steps], n, flags), v0, *out, *tile)).any()


def test_constant_tiles_stay_constant():
    """the weights of every stage sum to 256 and the rounding adds half: no value leaves the range, none drifts"""
    for value in (0, 1, 127, 254, 255):
        views = np.full((ref.V, ref.H, ref.W, 4), value, np.uint8)
        views[..., 3] = 255
        for tile, out in (((50, 22), (131, 67)), ((17, 9), (64, 36)), ((25, 11), (7, 5)), ((1, 1), (50, 22))):
            got = fref.native(views, ref.Lens(*ref.STEPS["slant"], 10, BILINEAR | BLEND), 0, *out, *tile)
            assert (got[..., :3] == value).all() and (got[..., 3] == 255).all()


# ---- the taps the kernel computes ---------------------------------------------------------------------------------------------------------------

def test_the_kernels_taps_equal_the_definition(native):
    """csrc/native_taps.h splits (2·o + 1)·src to stay in 32 bits: the same taps as the definition in Python integers, at the shared sizes, at
    the largest sizes and at random ones; both clamps occur"""
    rng = np.random.default_rng(7)
    pairs = [(s, d) for s in (1, 9, 11, 17, 22, 25, 50) for d in (1, 3, 5, 7, 22, 36, 50, 64, 67, 131, 300)]
    pairs += [(int(rng.integers(1, 65536)), int(rng.integers(1, 65536))) for _ in range(40)]
    clamped_low = clamped_high = 0
    for src, dst in pairs:
        p0, p1, f = fref.taps(dst, src)
        for o in range(dst) if dst <= 300 else [0, 1, dst // 2, dst - 2, dst - 1] + [int(v) for v in rng.integers(0, dst, 20)]:
            assert native.native_taps(src, dst, o) == (p0[o], p1[o], f[o]), (src, dst, o)
        clamped_low += (2 * 0 + 1) * src < dst
        clamped_high += src > 1 and p0[-1] == src - 1
    assert clamped_low and clamped_high
    for src, dst in ((65535, 65535), (65535, 1), (1, 65535), (65535, 65534), (65534, 65535), (2, 65535), (65535, 2)):
        for o in sorted({0, 1 % dst, dst // 2, dst - 1, max(dst - 2, 0)}):
            D = 2 * dst
            U = min(max((2 * o + 1) * src - dst, 0), (src - 1) * D)
            assert native.native_taps(src, dst, o) == (U // D, min(U // D + 1, src - 1), 256 * (U % D) // D), (src, dst, o)
    for bad in ((0, 4, 0), (4, 0, 0), (65536, 4, 0), (4, 65536, 0), (4, 4, 4), (4, 4, -1)):
        with pytest.raises(ValueError):
            native.native_taps(*bad)


# ---- the calibration file -------------------------------------------------------------------------------------------------------------------

GOLDEN = os.path.join(GOLDEN_DIR, "lens_calibration.json")
CALIBRATION = {"pitch": 52.5741, "slope": -7.1956, "center": -0.3817, "DPI": 283.0, "invView": 1.0, "flipSubp": 0.0, "screenW": 3840.0, "screenH": 2160.0}


def _as_tuple(lens):
    return (lens.x_step, lens.y_step, lens.phase0, lens.views, lens.flags)


def _write(path, entries, spelling="object"):
    """a calibration file of the entries, numbers as {"value": x} or plain"""
    path.write_text(json.dumps({k: ({"value": v} if spelling == "object" and not isinstance(v, str) else v) for k, v in entries.items()}, indent=1))
    return str(path)


def test_calibration_file_equals_the_restatement_bit_for_bit(native):
    for size in ((3840, 2160, 45), (2560, 1600, 48), (31, 17, 6)):
        lens, screen = native.lenticular_file(GOLDEN, *size, with_screen=True)
        assert _as_tuple(lens) == _as_tuple(ref.calibrate(52.5741, -7.1956, -0.3817, 283.0, True, *size)) and screen == (3840, 2160)
        assert _as_tuple(lens) == _as_tuple(native.lenticular(52.5741, -7.1956, -0.3817, 283.0, True, *size))


def test_calibration_file_spellings_order_and_flags(native, tmp_path):
    want = _as_tuple(native.lenticular_file(GOLDEN, 3840, 2160, 45))
    noise = {"serial": "a \"quoted\" {name}", "viewCone": 40.0, "notes": "pitch: 1, \"slope\": {\"value\": 2}"}
    for spelling in ("object", "plain"):
        assert _as_tuple(native.lenticular_file(_write(tmp_path / f"{spelling}.json", {**noise, **CALIBRATION}, spelling), 3840, 2160, 45)) == want
        reordered = dict(reversed(list({**CALIBRATION, **noise}.items())))
        assert _as_tuple(native.lenticular_file(_write(tmp_path / f"{spelling}_r.json", reordered, spelling), 3840, 2160, 45)) == want
    # a mixed file, nested values that are skipped, exponents, no optional key: invView and flipSubp default to 0, the screen to "not stated"
    (tmp_path / "mixed.json").write_text('\ufeff{ "extra": {"a": [1, {"b": null}, "x"], "value": true}, "DPI": 2.83e2,\n"center": {"note": "first", "value": -0.3817},'
                                         '"list": [], "slope": {"value": -7.1956}, "pitch": 52.5741 }\n', encoding="utf-8")
    lens, screen = native.lenticular_file(str(tmp_path / "mixed.json"), 3840, 2160, 45, with_screen=True)
    assert _as_tuple(lens) == _as_tuple(ref.calibrate(52.5741, -7.1956, -0.3817, 283.0, False, 3840, 2160, 45)) and screen == (0, 0)
    # flipSubp: BGR; with invView both
    for inv, flip, flags in ((0.0, 1.0, BGR), (1.0, 1.0, INVERT | BGR), (0.0, 0.0, 0)):
        got = native.lenticular_file(_write(tmp_path / "f.json", {**CALIBRATION, "invView": inv, "flipSubp": flip}), 3840, 2160, 45)
        assert got.flags == flags and _as_tuple(got)[:4] == want[:4]
    assert native.LFI_LENT_BGR == BGR and native.LFI_LENT_BILINEAR == BILINEAR and native.LFI_LENT_BLEND == BLEND


def test_calibration_file_refusals_name_the_key(native, tmp_path):
    for key in ("pitch", "slope", "center", "DPI"):
        with pytest.raises(ValueError, match=f'no "{key}"'):
            native.lenticular_file(_write(tmp_path / "m.json", {k: v for k, v in CALIBRATION.items() if k != key}), 3840, 2160, 45)
        with pytest.raises(ValueError, match=f'"{key}" without a number'):
            native.lenticular_file(_write(tmp_path / "s.json", {**CALIBRATION, key: "12"}), 3840, 2160, 45)
    (tmp_path / "o.json").write_text(json.dumps({**CALIBRATION, "invView": {"valve": 1.0}}))
    with pytest.raises(ValueError, match='"invView" without a number'):
        native.lenticular_file(str(tmp_path / "o.json"), 3840, 2160, 45)
    for key in ("flipImageX", "flipImageY"):
        with pytest.raises(ValueError, match=f'"{key}".*mirrored'):
            native.lenticular_file(_write(tmp_path / "x.json", {**CALIBRATION, key: 1.0}), 3840, 2160, 45)
        assert native.lenticular_file(_write(tmp_path / "x0.json", {**CALIBRATION, key: 0.0}), 3840, 2160, 45).flags == INVERT
    for text in ("", "[1, 2]", '{"pitch": 1', '{"pitch": 1,}', '{"pitch" 1}', '{"pitch": 50, "slope": 5, "center": 0, "DPI": 300} x', '{"pitch": "unterminated}'):
        (tmp_path / "bad.json").write_text(text)
        with pytest.raises(ValueError, match="JSON object"):
            native.lenticular_file(str(tmp_path / "bad.json"), 3840, 2160, 45)
    with pytest.raises(ValueError, match="cannot be opened"):
        native.lenticular_file(str(tmp_path / "missing.json"), 3840, 2160, 45)
    with pytest.raises(ValueError, match="calibration"):   # the calibration's own refusals reach through: a slope of 0
        native.lenticular_file(_write(tmp_path / "z.json", {**CALIBRATION, "slope": 0.0}), 3840, 2160, 45)


# ---- the library and the command line -----------------------------------------------------------------------------------------------------

def test_symbols_are_exported_and_bound(native):
    host = native.load_host_library()
    assert hasattr(host, "lfi_host_lenticular_json") and hasattr(host, "lfi_host_native_taps")
    assert (native.LFI_LENT_INVERT, native.LFI_LENT_BGR, native.LFI_LENT_BILINEAR, native.LFI_LENT_BLEND) == (1, 4, 8, 16)
    header = open(os.path.join(os.path.dirname(GOLDEN_DIR), "..", "include", "lfi.h")).read()
    for name, value in (("LFI_LENT_BGR", 4), ("LFI_LENT_BILINEAR", 8), ("LFI_LENT_BLEND", 16)):
        assert re.search(rf"#define {name}\s+{value}u\b", header), name


NATIVE_ARGS = ["--synthetic", "4,4,32,16", "-t", "0,0,1,1", "-m", "STD", "-n", "6", "-b", "1", "-f", "0.0"]


@pytest.mark.parametrize("extra,words", [
    (["--native", "64x36", "--lens", "50,5,0,300", "--lens-file", GOLDEN], ("--lens", "--lens-file", "one of them")),
    (["--lens-file", GOLDEN], ("--native", "--lens-file")),
    (["--native-filter", "bilinear"], ("--native-filter", "--native WxH")),
    (["--native-blend"], ("--native-blend", "--native WxH")),
    (["--lens-bgr"], ("--lens-bgr", "--native WxH")),
    (["--native", "64x36", "--lens", "50,5,0,300", "--native-filter", "cubic"], ("--native-filter", "nearest or bilinear")),
    (["--native", "64x36", "--lens", "50,5,0,300", "--native-filter"], ("--native-filter", "nearest or bilinear")),
    (["--native", "64x36", "--lens-file", os.path.join(GOLDEN_DIR, "no_such_file.json")], ("--lens-file", "cannot be opened")),
    (["--native", "64x36", "--lens-file"], ("--lens-file", "name of the calibration file")),
])
def test_cli_refuses_before_anything_runs(native, tmp_path, extra, words):
    res = run_cli(native, *NATIVE_ARGS, "-o", str(tmp_path / "out"), *extra)
    assert res.returncode != 0
    for word in words:
        assert word in res.stderr, res.stderr
    assert not (tmp_path / "out").exists()


def test_cli_refuses_a_calibration_file_it_cannot_use(native, tmp_path):
    for entries, words in (({**CALIBRATION, "flipImageX": 1.0}, ("flipImageX", "mirrored")), ({k: v for k, v in CALIBRATION.items() if k != "DPI"}, ('no "DPI"',)),
                           ({**CALIBRATION, "pitch": "52"}, ('"pitch" without a number',))):
        res = run_cli(native, *NATIVE_ARGS, "-o", str(tmp_path / "out"), "--native", "64x36", "--lens-file", _write(tmp_path / "c.json", entries))
        assert res.returncode != 0 and "--lens-file" in res.stderr
        for word in words:
            assert word in res.stderr, res.stderr
        assert not (tmp_path / "out").exists()


def test_cli_help_names_the_flags(native):
    res = run_cli(native, "-h")
    assert res.returncode == 0
    for flag in ("--native-filter nearest|bilinear", "--native-blend", "--lens-bgr", "--lens-file FILE"):
        assert flag in res.stdout


# ---- the code object --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not code_object.have_tools(), reason="ROCm LLVM tools not installed")
def test_native_filter_uses_no_scratch_no_lds_and_whole_dword_stores(native):
    """From the code object: the eight instantiations of native_filter (csrc/hip/native_filter.hpp) exist, use no scratch and no LDS, spill
    nothing, stay at or below 64 registers per lane (eight waves per SIMD), load one byte per (channel, view, row, tap), store one dword and
    nothing narrower, and contain no atomic instruction."""
    kernels = code_object.kernels(native.build.HIP_LIB)
    filt = code_object.named(kernels, "native_filter")
    assert len(filt) == 8, sorted(filt)
    for k, v in filt.items():
        assert v[".private_segment_fixed_size"] == 0 and v[".vgpr_spill_count"] == 0 and v[".sgpr_spill_count"] == 0, (k, v)
        assert v[".group_segment_fixed_size"] == 0 and v[".vgpr_count"] <= 64, (k, v)
    bodies = {k: v for k, v in code_object.bodies(native.build.HIP_LIB).items() if k in filt}
    assert set(bodies) == set(filt)
    loads = []
    for k, text in sorted(bodies.items()):
        assert "atomic" not in text and "scratch_" not in text and "ds_" not in text, k
        assert set(re.findall(r"\b\w+_store_\w+", text)) == {"global_store_dword"} and len(re.findall(r"\bglobal_store_dword\b", text)) == 1, k
        loads.append(len(re.findall(r"\bglobal_load_ubyte\b", text)))
        assert len(re.findall(r"\b\w+_load_\w+", text)) - len(re.findall(r"\bs_load_\w+", text)) == loads[-1], k   # every vector load is a byte
    # PLANAR × BILINEAR × BLEND in the mangled names' order: three channels × (1, 2 views) × (1, 4 taps)
    assert loads == [3, 6, 12, 24, 3, 6, 12, 24], loads
