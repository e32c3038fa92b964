"""numpy restatement of the fine focus map (lfi_set_focus_steps + lfi_focus_map) — test infrastructure, anchored to the committed oracle and
not to the code under test: tests/test_host_focus_steps.py checks that at 32 steps it is oracle_c.focus_estimate byte for byte.

With `steps` candidates f_i = fmaf(range / (steps - 1), i, focus) (focus_curve_ref.candidates), a pixel's winner is the first i with the
strictly smallest comparison key: 16 * S_i (focus_curve_ref.pixel_costs), or, where S_i = 0, the number of FLT_MIN taps — the reference starts
its running maximum at FLT_MIN (src/kernels.cu:178), so a tap whose range is 0 and one of whose channels is 0 in every sampled image adds
FLT_MIN to the float sum; a sum of k such terms orders like k, below every sum with S >= 1.  Map 0 byte = round((f_best - focus) / range * 255)
in float32 (focus_curve_ref.map_byte); map 1 is oracle_c.focus_filter of map 0.
"""
import numpy as np

from focus_curve_ref import _warp, candidates, map_byte, pixel_costs
from oracle.lfi_oracle_np import fetch


def flt_min_taps(lf, offs, ids, f, radius):
    """the number of a pixel's nine taps whose colour range is 0 and where some channel's maximum over the sampled images is 0: [H][W] int64"""
    n, h, w, _ = lf.shape
    ys, xs = np.meshgrid(np.arange(h, dtype=np.int32), np.arange(w, dtype=np.int32), indexing="ij")
    lo = np.full((9, h, w, 3), 255, dtype=np.int64)
    hi = np.zeros((9, h, w, 3), dtype=np.int64)
    for g in ids:
        cx = _warp(f, offs[g, 0], xs)
        cy = _warp(f, offs[g, 1], ys)
        t = 0
        for dx in (-int(radius[0]), 0, int(radius[0])):
            for dy in (-int(radius[1]), 0, int(radius[1])):
                px = fetch(lf[g], cx + dx, cy + dy)[..., :3].astype(np.int64)
                lo[t] = np.minimum(lo[t], px)
                hi[t] = np.maximum(hi[t], px)
                t += 1
    return (((hi - lo).max(axis=-1) == 0) & (hi.min(axis=-1) == 0)).sum(axis=0)


def keys(lf, offs, ids, focus, rng, radius, steps):
    """the comparison key of every candidate and pixel, [steps][H][W] int64, and the mask [steps][H][W] of the keys the S = 0 rule gave"""
    costs = pixel_costs(lf, offs, ids, focus, rng, radius, steps)
    key = costs * 16
    zero = costs == 0
    f = candidates(focus, rng, steps)
    for i in np.nonzero(zero.any(axis=(1, 2)))[0]:
        key[i][zero[i]] = flt_min_taps(lf, offs, ids, f[i], radius)[zero[i]]
    return key, zero


def winners(key):
    """the first candidate with the strictly smallest key, per pixel: [H][W] (np.argmin returns the first minimum)"""
    return np.argmin(key, axis=0)


def map0(lf, offs, ids, focus, rng, radius, steps, with_index=False, key=None):
    """map 0 as lfi_download_map returns it: [H][W][4] u8, the byte in R, G and B, alpha 255 (key: the keys, where the caller has them)"""
    if key is None:
        key, _ = keys(lf, offs, ids, focus, rng, radius, steps)
    best = winners(key)
    byte = map_byte(candidates(focus, rng, steps)[best], focus, rng)
    out = np.empty(byte.shape + (4,), np.uint8)
    out[..., :3] = byte[..., None]
    out[..., 3] = 255
    return (out, best) if with_index else out


def shifts(offs, ids, f):
    """every sampled image's integer shift at focus f, [len(ids)][2]: floor(f * offset), the product of two floats exact in double"""
    return np.floor(np.float64(np.float32(f)) * offs[np.asarray(ids)].astype(np.float64)).astype(np.int64)
