"""CPU: the numpy reference of lfi_compare_views (tests/quality_ref.py) against the window-by-window loop that lfi_compare_view is asserted with,
and the two new entry points of the library as far as they go without a device."""
import ctypes
import math

import numpy as np
import pytest

import code_object
import quality_ref as ref


def _ssim_psnr_loop(a, b):
    """tests/test_gpu_plumbing.py::_ssim_psnr_numpy, restated: per channel MSE over all pixels; SSIM = mean over 8×8 windows at stride 4"""
    a = a[..., :3].astype(np.float64)
    b = b[..., :3].astype(np.float64)
    mse = ((a - b) ** 2).mean(axis=(0, 1))
    H, W = a.shape[:2]
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    ssim = np.zeros(3)
    count = 0
    for y in range(0, H - 7, 4):
        for x in range(0, W - 7, 4):
            wa, wb = a[y:y + 8, x:x + 8].reshape(64, 3), b[y:y + 8, x:x + 8].reshape(64, 3)
            mu1, mu2 = wa.mean(0), wb.mean(0)
            var1, var2 = (wa * wa).mean(0) - mu1 * mu1, (wb * wb).mean(0) - mu2 * mu2
            cov = (wa * wb).mean(0) - mu1 * mu2
            ssim += ((2 * mu1 * mu2 + C1) * (2 * cov + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (var1 + var2 + C2))
            count += 1
    return mse, ssim / max(count, 1), count


def _pair(rng, w, h, kind):
    a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    a[..., :3] = (a[..., :3].astype(np.int32) // 3 + np.arange(w)[None, :, None] // 2).clip(0, 255).astype(np.uint8)
    if kind == "near":      # within one LSB, as TEN_WM against STD
        b = (a.astype(np.int32) + rng.integers(-1, 2, a.shape)).clip(0, 255).astype(np.uint8)
    elif kind == "unrelated":
        b = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    else:
        b = a.copy()
    b[..., 3] = rng.integers(0, 256, (h, w), dtype=np.uint8)   # alpha is ignored
    return a, b


@pytest.mark.parametrize("w,h", [(150, 61), (64, 32), (7, 40), (40, 7), (258, 130), (8, 8), (11, 9), (12, 13)])
@pytest.mark.parametrize("kind", ["near", "unrelated", "same"])
def test_vectorised_reference_equals_the_window_loop(w, h, kind):
    rng = np.random.default_rng(w * 1000 + h)
    a, b = _pair(rng, w, h, kind)
    got = ref.compare(a, b)
    mse, ssim, count = _ssim_psnr_loop(a, b)
    assert got["windows"] == count == (max((w - 8) // 4 + 1, 0) * max((h - 8) // 4 + 1, 0) if w >= 8 and h >= 8 else 0)
    assert np.allclose(got["mse"], mse, rtol=1e-12, atol=0)
    if count:
        assert np.allclose(got["ssim"], ssim, rtol=1e-9, atol=0)
    else:
        assert got["ssim"] == [1.0, 1.0, 1.0] and got["ssim_all"] == 1.0
    d = a[..., :3].astype(int) - b[..., :3].astype(int)
    assert got["sq_err"] == [int((d[..., c] ** 2).sum()) for c in range(3)]
    assert got["differing_bytes"] == int((d != 0).sum()) and got["max_abs_diff"] == int(abs(d).max())
    if kind == "same":
        assert got["psnr_all"] == math.inf and got["psnr"] == [math.inf] * 3 and got["differing_bytes"] == 0 and got["max_abs_diff"] == 0
        assert abs(got["ssim_all"] - 1.0) < 1e-12
    else:
        assert abs(got["psnr_all"] - 10 * np.log10(255.0 ** 2 / mse.mean())) < 1e-9


def test_aggregate_is_built_from_the_integers():
    rng = np.random.default_rng(5)
    w, h = 37, 21
    recs = [ref.compare(*_pair(rng, w, h, kind)) for kind in ("near", "unrelated", "same", "near")]
    agg = ref.aggregate(recs, w, h)
    for c in range(3):
        assert agg["mse"][c] == sum(r["sq_err"][c] for r in recs) / (4 * w * h)
        assert abs(agg["ssim"][c] - np.mean([r["ssim"][c] for r in recs])) < 1e-15
    assert agg["psnr_all"] == 10.0 * math.log10(255.0 * 255.0 / (agg["mse"][0] / 3.0 + agg["mse"][1] / 3.0 + agg["mse"][2] / 3.0))


def test_library_exports_the_batch_comparison(native):
    native.load_hip_library()
    lib = ctypes.CDLL(native.build.HIP_LIB)
    for name in ("lfi_keep_views", "lfi_compare_views"):
        assert hasattr(lib, name), name
        assert name in native.ABI_SYMBOLS


def test_null_context_is_einval(native):
    lib = native.load_hip_library()
    out = (native.abi.ViewQuality * 1)()
    assert lib.lfi_keep_views(None, 0, 1) == -1
    assert lib.lfi_keep_views(None, 0, 0) == -1
    assert lib.lfi_compare_views(None, 0, 1, None, 0, 0, out, None) == -1


def test_record_layout_matches_the_header(native):
    """lfi_view_quality as include/lfi.h lays it out: lfi_quality (11 doubles), five 64-bit integers, one 32-bit, padded to 8"""
    q = native.abi.ViewQuality
    assert ctypes.sizeof(native.abi.Quality) == 88
    assert (q.sq_err.offset, q.differing_bytes.offset, q.windows.offset, q.max_abs_diff.offset, ctypes.sizeof(q)) == (88, 112, 120, 128, 136)


def test_the_new_kernels_use_no_scratch(native):
    """quality_tiles (three layout pairs) and quality_views: no scratch, no spills, wave size 64 (the code object's notes)"""
    kernels = code_object.kernels(native.build.HIP_LIB)
    tiles, views = code_object.named(kernels, "quality_tiles"), code_object.named(kernels, "quality_views")
    ours = {**tiles, **views}
    assert len(tiles) == 3 and len(views) == 1, sorted(ours)
    for k, v in ours.items():
        assert v[".private_segment_fixed_size"] == 0 and v[".vgpr_spill_count"] == 0 and v[".sgpr_spill_count"] == 0 and v[".wavefront_size"] == 64, (k, v)
