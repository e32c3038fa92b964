"""The definitions of lfi_compare_views (include/lfi.h, at lfi_compare_view) restated in vectorised numpy — the reference the
GPU tests compare against.  tests/test_host_compare_views.py holds it against the window-by-window loop the project already asserts
lfi_compare_view with (tests/test_gpu_plumbing.py::_ssim_psnr_numpy).

Per colour channel (alpha is ignored): the squared error summed over all pixels, in integers; MSE = that sum / (W·H); PSNR = 10·log10(255² / MSE),
+inf for MSE 0; "all" from the mean of the three MSEs.  SSIM = the mean over all 8×8 windows at stride 4 that fit of
((2·μa·μb + C1)(2·σab + C2)) / ((μa² + μb² + C1)(σa² + σb² + C2)) with the window's biased moments, C1 = (0.01·255)², C2 = (0.03·255)²; 1.0 when no
window fits; "all" = the mean of the channels.  The window sums are exact integers here too (from integral images), so the moments are the very
numbers the device forms; only the order of the final sum over windows differs."""
import math

import numpy as np

C1 = 0.01 * 255.0 * 0.01 * 255.0
C2 = 0.03 * 255.0 * 0.03 * 255.0


def _psnr(mse):
    return 10.0 * math.log10(255.0 * 255.0 / mse) if mse > 0 else math.inf


def _window_sums(p):
    """p: [H][W][3] int64 → the sums over every 8×8 window at stride 4 that fits, [wy][wx][3] (empty if none fits)"""
    H, W = p.shape[:2]
    integral = np.zeros((H + 1, W + 1, 3), np.int64)
    integral[1:, 1:] = p.cumsum(0).cumsum(1)
    ys, xs = np.arange(0, H - 7, 4), np.arange(0, W - 7, 4)
    if len(ys) == 0 or len(xs) == 0:
        return np.zeros((0, 0, 3), np.int64)
    y0, x0 = np.meshgrid(ys, xs, indexing="ij")
    return integral[y0 + 8, x0 + 8] - integral[y0, x0 + 8] - integral[y0 + 8, x0] + integral[y0, x0]


def finish(mse, ssim):
    """psnr per channel, psnr_all and ssim_all from the per-channel mse and ssim — lfi_compare_view's arithmetic"""
    mse_all = ssim_all = 0.0
    for c in range(3):
        mse_all += mse[c] / 3.0
        ssim_all += ssim[c] / 3.0
    return dict(mse=list(mse), ssim=list(ssim), psnr=[_psnr(m) for m in mse], psnr_all=_psnr(mse_all), ssim_all=ssim_all)


def compare(a, b):
    """a, b: [H][W][≥3] uint8.  Returns a dict with the fields of lfi_view_quality (q's fields at the top level)."""
    assert a.shape[:2] == b.shape[:2]
    H, W = a.shape[:2]
    ia, ib = a[..., :3].astype(np.int64), b[..., :3].astype(np.int64)
    d = ia - ib
    sq_err = [int(v) for v in (d * d).sum(axis=(0, 1))]
    mse = [float(s) / float(W * H) for s in sq_err]
    s1, s2, s11, s22, s12 = (_window_sums(v) for v in (ia, ib, ia * ia, ib * ib, ia * ib))
    windows = s1.shape[0] * s1.shape[1]
    if windows:
        mu1, mu2 = s1 / 64.0, s2 / 64.0
        var1, var2, cov = s11 / 64.0 - mu1 * mu1, s22 / 64.0 - mu2 * mu2, s12 / 64.0 - mu1 * mu2
        index = ((2.0 * mu1 * mu2 + C1) * (2.0 * cov + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (var1 + var2 + C2))
        ssim = [float(index[..., c].sum() / windows) for c in range(3)]
    else:
        ssim = [1.0, 1.0, 1.0]
    out = finish(mse, ssim)
    out.update(sq_err=sq_err, differing_bytes=int((d != 0).sum()), windows=windows, max_abs_diff=int(np.abs(d).max()))
    return out


def aggregate(per_view, width, height):
    """lfi_compare_views' out_all from the per-view records (dicts of compare): mse from the summed integers, ssim the mean of the views' in view order"""
    n = len(per_view)
    mse = [float(sum(r["sq_err"][c] for r in per_view)) / float(n * width * height) for c in range(3)]
    ssim = []
    for c in range(3):
        s = 0.0
        for r in per_view:
            s += r["ssim"][c]
        ssim.append(s / float(n))
    return finish(mse, ssim)
