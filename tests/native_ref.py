"""The native image of lfi_download_native restated in numpy, from the definition in include/lfi.h, and the calibration arithmetic of
csrc/host/lenticular.h restated in Python floats (IEEE-754 doubles: +, −, ×, ÷ and sqrt round the same everywhere).

For output pixel (x, y) and colour channel c:  phase = phase0 + (3·x + c)·x_step + y·y_step (mod 2³²),  k = (phase·n) >> 32 (inverted:
n − 1 − k),  sx = ((2·x + 1)·tile_w) // (2·out_w),  sy likewise,  out[y][x][c] = T_{v0+k}[sy][sx][c],  alpha = 255, with T_v view v resized to the
tile by scaled_quilt_ref.resize.  `native` does this with uint64 arrays (every product stays below 2⁵¹), `native_slow` as a triple loop in
Python integers; tests/test_host_native.py holds the two against each other.

STEPS and the case lists below are shared by the CPU and the GPU tests."""
import math
from dataclasses import dataclass

import numpy as np

import scaled_quilt_ref as quilt_ref

INVERT = 1          # LFI_LENT_INVERT
MASK = (1 << 32) - 1


@dataclass(frozen=True)
class Lens:
    """lfi_lenticular"""
    x_step: int
    y_step: int
    phase0: int
    views: int
    flags: int = 0

    def with_views(self, n, invert=False):
        return Lens(self.x_step, self.y_step, self.phase0, n, INVERT if invert else 0)


def select(lens: Lens, out_w: int, out_h: int) -> np.ndarray:
    """[out_h][out_w][3] int64: the k every subpixel selects (after LFI_LENT_INVERT)"""
    x = np.arange(out_w, dtype=np.uint64)[None, :, None]
    y = np.arange(out_h, dtype=np.uint64)[:, None, None]
    c = np.arange(3, dtype=np.uint64)[None, None, :]
    phase = (np.uint64(lens.phase0) + (np.uint64(3) * x + c) * np.uint64(lens.x_step) + y * np.uint64(lens.y_step)) & np.uint64(MASK)
    k = ((phase * np.uint64(lens.views)) >> np.uint64(32)).astype(np.int64)
    return lens.views - 1 - k if lens.flags & INVERT else k


def nearest(dst: int, src: int) -> np.ndarray:
    """[dst] int64: ((2·o + 1)·src) // (2·dst), the source pixel under the centre of output pixel o"""
    o = np.arange(dst, dtype=np.int64)
    return ((2 * o + 1) * src) // (2 * dst)


def tiles(views: np.ndarray, tile_w: int, tile_h: int) -> np.ndarray:
    """[V][H][W][4] -> [V][tile_h][tile_w][4]: T_v (the views themselves at their own size)"""
    if views.shape[1:3] == (tile_h, tile_w):
        return views
    return np.stack([quilt_ref.resize(v, tile_w, tile_h) for v in views])


def native(views: np.ndarray, lens: Lens, v0: int, out_w: int, out_h: int, tile_w: int, tile_h: int) -> np.ndarray:
    """views [V][H][W][4] u8 -> the native image [out_h][out_w][4] u8"""
    t = tiles(views[v0:v0 + lens.views], tile_w, tile_h)
    assert len(t) == lens.views
    k = select(lens, out_w, out_h)
    sy = nearest(out_h, tile_h)[:, None, None]
    sx = nearest(out_w, tile_w)[None, :, None]
    out = np.full((out_h, out_w, 4), 255, np.uint8)
    out[..., :3] = t[k, sy, sx, np.arange(3)[None, None, :]]
    return out


def native_slow(views: np.ndarray, lens: Lens, v0: int, out_w: int, out_h: int, tile_w: int, tile_h: int) -> np.ndarray:
    """the definition as it is written: a loop over y, x and c in Python integers (tiny cases only)"""
    H, W = views.shape[1:3]
    t = {}
    out = np.zeros((out_h, out_w, 4), np.uint8)
    for y in range(out_h):
        for x in range(out_w):
            for c in range(3):
                phase = (lens.phase0 + (3 * x + c) * lens.x_step + y * lens.y_step) % (1 << 32)
                k = (phase * lens.views) >> 32
                if lens.flags & INVERT:
                    k = lens.views - 1 - k
                sx = ((2 * x + 1) * tile_w) // (2 * out_w)
                sy = ((2 * y + 1) * tile_h) // (2 * out_h)
                if k not in t:
                    t[k] = views[v0 + k] if (tile_w, tile_h) == (W, H) else quilt_ref.resize_dense(views[v0 + k], tile_w, tile_h)
                out[y, x, c] = t[k][sy, sx, c]
            out[y, x, 3] = 255
    return out


# ---- the calibration (csrc/host/lenticular.cpp, operation by operation) ----------------------------------------------------------------

def _round_to_phase(v: float) -> int:
    """nearest integer, ties away from zero, mod 2³²"""
    mag = -v if v < 0.0 else v
    assert mag < 4503599627370496.0
    r = int(mag + 0.5)
    return (-r if v < 0.0 else r) & MASK


def calibrate(pitch: float, slope: float, center: float, dpi: float, invert: bool, out_w: int, out_h: int, n: int) -> Lens:
    w, h, two32 = float(out_w), float(out_h), 4294967296.0
    abs_slope = -slope if slope < 0.0 else slope
    p = ((pitch * w) / dpi) * (abs_slope / math.sqrt(slope * slope + 1.0))
    tilt = h / (w * slope)
    return Lens(_round_to_phase((two32 * p) / (3.0 * w)),
                _round_to_phase(((two32 * p) * tilt) / h),
                _round_to_phase(two32 * (p * (0.5 / w + (0.5 * tilt) / h) - center)),
                n, INVERT if invert else 0)


# ---- the cases the CPU and the GPU tests share --------------------------------------------------------------------------------------------

W, H, V = 50, 22, 10                                    # the views of tests/test_gpu_scaled_quilt.py
TILES = [(50, 22), (17, 9), (25, 11), (1, 1)]           # (50, 22): no stage 1
OUTPUTS = [(50, 22), (7, 5), (64, 36), (131, 67)]       # the views' size, smaller, larger, and an odd size of more than two waves per row that upsamples
VIEW_RANGES = [(10, 0), (3, 7), (1, 4)]                 # (n, v0)

# x_step, y_step, phase0.  "slant" and "negative slant" are the GENERAL sets: 0.37 and 0.23 of a lens period per subpixel and per row, chosen
# so that for every output size and every n above each of the n views is selected in every channel, and (n ≥ 3) some pixel's three channels
# select three different views — test_host_native.py asserts both.  The other sets pin special phases and cannot cover every view:
# "boundary" puts every subpixel exactly ON a boundary between two of 8 views (k·2³²/8 selects k), "below boundary" one unit below
# it (selects k − 1): both sides; "boundary rows" also steps by three boundaries per row.
STEPS = {
    "slant": (1589137899, 987842478, 305419896),
    "negative slant": (1589137899, (1 << 32) - 987842478, 2882400001),
    "boundary": (1 << 29, 0, 0),
    "below boundary": (1 << 29, 0, MASK),
    "boundary rows": (1 << 29, 3 << 29, 1 << 31),
}
GENERAL = ("slant", "negative slant")


def one_view_phase(k: int, n: int) -> int:
    """the smallest phase that selects view k of n: ⌈k·2³²/n⌉"""
    return -((-k << 32) // n)
