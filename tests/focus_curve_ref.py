"""numpy restatement of the focus curve (lfi_focus_curve) — test infrastructure, anchored to the committed oracle and not to the code under
test: tests/test_host_focus_curve.py checks that the per-pixel argmin of these costs is oracle_c.focus_estimate's map byte.

S_i(x, y) is the integer form of FocusMap::focusDispersion (reference src/kernels.cu:196-217, ElementRange :173-194) for candidate
f_i = fmaf(range / (steps - 1), i, focus): over the sampled images, at (int)fmaf(f_i, offsets[g], pixel) +- block_radius (3 x 3 taps, clamp
to edge), per tap the largest channel's max - min, summed over the nine taps.  The reference's FLT_MIN start value (:178) is dropped: an
all-zero tap contributes 0 (include/lfi.h documents the departure).  cost[i] = the sum of S_i over the region.
"""
import numpy as np

from oracle.lfi_oracle_np import _fma32, fetch

F32 = np.float32


def candidates(focus, rng, steps):
    """f_i in float32: step = range / (float)(steps - 1), f_i = fmaf(step, (float)i, focus)"""
    step = F32(F32(rng) / F32(steps - 1))
    return np.array([_fma32(step, F32(i), F32(focus)) for i in range(steps)], dtype=F32)


def _warp(f, off, coord):
    """(int)fmaf(f, off, coord): C truncation; the conversion saturates on the device"""
    v = np.trunc(_fma32(f, off, coord.astype(F32))).astype(np.float64)
    return np.clip(v, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def dispersion(lf, offs, ids, f, radius):
    """S(x, y) of one candidate f for every pixel: [H][W] int64"""
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
    return (hi - lo).max(axis=-1).sum(axis=0)


def pixel_costs(lf, offs, ids, focus, rng, radius, steps=32):
    """S_i(x, y) for every candidate and pixel: [steps][H][W] int64"""
    return np.stack([dispersion(lf, offs, ids, f, radius) for f in candidates(focus, rng, steps)])


def curve(costs, x0, y0, x1, y1):
    """cost[i] of the region [x0, x1) x [y0, y1) from pixel_costs: [steps] uint64"""
    return costs[:, y0:y1, x0:x1].sum(axis=(1, 2)).astype(np.uint64)


def first_min(cost):
    """the first candidate with the strictly smallest cost (MinDispersion, src/kernels.cu:225-231)"""
    return int(np.argmin(cost))


def map_byte(f_best, focus, rng):
    """what FocusMap::estimate stores for a winning candidate: round((f - focus) / range * 255) (src/kernels.cu:252-256)"""
    normalized = ((np.asarray(f_best, F32) - F32(focus)) / F32(rng)).astype(F32)
    return np.floor((normalized * F32(255.0)).astype(np.float64) + 0.5).astype(np.uint8)


# ---- the planted scene: a texture seen at one focus -----------------------------------------------------------------------------------

# 4 x 4 grid of 96 x 64 images, every image sampled; 32 candidates over [0, 0.5].  The camera sits on the last grid point ("1,1,1,1"), so every
# offset is >= 0 and the (int) of the shifts below is the floor the warp applies: (int)fmaf(f_k, offset, x) = x + (int)(f_k * offset), and all
# images show the same texel exactly at f_k (cost 0 there).  tests/test_host_focus_curve.py asserts on the CPU that the curve of every region
# has its strict minimum at the planted candidate, for both values of k; the GPU test uploads the same images.
PLANTED = dict(cols=4, rows=4, W=96, H=64, traj="1,1,1,1", focus=0.0, rng=0.5, steps=32, seed=20241, ks=(9, 22))
PLANTED_REGIONS = [(16, 8, 48, 24), (9, 11, 58, 30), (30, 14, 42, 26)]   # inside the area where no tap of any candidate clamps


def planted_scene(offs, k, cols, rows, W, H, focus, rng, steps, seed, **_):
    """[N][H][W][4] u8: a random texture T of 8 x 8-pixel cells; image g shows T(x - sx_g, y - sy_g) with
    (sx_g, sy_g) = ((int)(f_k * offsets[g].x), (int)(f_k * offsets[g].y)) — what fill_scene (csrc/hip/focus_map.hpp) does on the device, with
    one focus for the whole image: sampling image g at pixel + (sx_g, sy_g) shows the same texel in every image."""
    f_k = candidates(focus, rng, steps)[k]
    rs = np.random.RandomState(seed)
    reach = int(np.ceil(np.abs(offs).max() * max(abs(focus), abs(focus + rng)))) + 8
    cells = rs.randint(0, 256, size=((H + 2 * reach) // 8 + 2, (W + 2 * reach) // 8 + 2, 3), dtype=np.int64).astype(np.uint8)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    lf = np.empty((cols * rows, H, W, 4), np.uint8)
    lf[..., 3] = 255
    for g in range(cols * rows):
        sx, sy = int(F32(f_k) * F32(offs[g, 0])), int(F32(f_k) * F32(offs[g, 1]))
        lf[g, ..., :3] = cells[(ys - sy + reach) >> 3, (xs - sx + reach) >> 3]
    return lf
