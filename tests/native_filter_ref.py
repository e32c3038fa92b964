"""The FILTERED native image of lfi_download_native (LFI_LENT_BGR, LFI_LENT_BILINEAR, LFI_LENT_BLEND) restated in numpy, from the definition in
include/lfi.h.  It reuses tests/native_ref.py's Lens, STEPS, tiles and case lists; with none of the three flags it is native_ref.native.

For output pixel (x, y) and colour channel c:  s = c (BGR: 2 − c),  phase = phase0 + (3·x + s)·x_step + y·y_step (mod 2³²),  P = phase·n,
k = P >> 32,  f = (P >> 24) & 255.  BLEND:  f ≥ 128: ka = k, kb = min(k + 1, n − 1), wb = f − 128;  else ka = max(k, 1) − 1, kb = k, wb = f + 128;
INVERT maps every index q to n − 1 − q;  out = ((256 − wb)·S_ka + wb·S_kb + 128) >> 8 — without BLEND out = S_k.  BILINEAR, along x with
D = 2·out_w:  U = clamp((2·x + 1)·tile_w − out_w, 0, (tile_w − 1)·D),  x0 = U // D,  fx = (256·(U − x0·D)) // D,  x1 = min(x0 + 1, tile_w − 1), along y
likewise, h_j = (256 − fx)·T[y_j][x0][c] + fx·T[y_j][x1][c],  S = ((256 − fy)·h_0 + fy·h_1 + 2¹⁵) >> 16 — without BILINEAR S = T[sy][sx][c], the
nearest pixel.  Alpha is 255.

`native` does this with int64 arrays (every product stays below 2⁵¹), `native_slow` as a triple loop in Python integers;
tests/test_host_native_filter.py holds the two against each other and against the properties that follow from the definition."""
import numpy as np

import native_ref as ref
import scaled_quilt_ref as quilt_ref
from native_ref import INVERT, Lens

BGR, BILINEAR, BLEND = 4, 8, 16          # LFI_LENT_BGR, LFI_LENT_BILINEAR, LFI_LENT_BLEND
FLAG_SETS = [a | b | c for a in (0, BGR) for b in (0, BILINEAR) for c in (0, BLEND)]   # the eight combinations of the three


def phases(lens: Lens, out_w: int, out_h: int) -> np.ndarray:
    """[out_h][out_w][3] uint64: the phase of every channel's subpixel"""
    x = np.arange(out_w, dtype=np.uint64)[None, :, None]
    y = np.arange(out_h, dtype=np.uint64)[:, None, None]
    c = np.arange(3, dtype=np.uint64)
    s = (np.uint64(2) - c if lens.flags & BGR else c)[None, None, :]
    return (np.uint64(lens.phase0) + (np.uint64(3) * x + s) * np.uint64(lens.x_step) + y * np.uint64(lens.y_step)) & np.uint64(ref.MASK)


def fractions(lens: Lens, out_w: int, out_h: int):
    """(k, f) before any flag: the view the phase falls into and the top eight bits of the fraction, [out_h][out_w][3] int64 each"""
    p = phases(lens, out_w, out_h) * np.uint64(lens.views)
    return (p >> np.uint64(32)).astype(np.int64), ((p >> np.uint64(24)) & np.uint64(255)).astype(np.int64)


def selection(lens: Lens, out_w: int, out_h: int):
    """(ka, kb, wb), [out_h][out_w][3] int64 each, after LFI_LENT_INVERT; without BLEND ka = kb = k and wb = 0"""
    n = lens.views
    k, f = fractions(lens, out_w, out_h)
    if lens.flags & BLEND:
        upper = f >= 128
        ka = np.where(upper, k, np.maximum(k, 1) - 1)
        kb = np.where(upper, np.minimum(k + 1, n - 1), k)
        wb = np.where(upper, f - 128, f + 128)
    else:
        ka, kb, wb = k, k, np.zeros_like(k)
    if lens.flags & INVERT:
        ka, kb = n - 1 - ka, n - 1 - kb
    return ka, kb, wb


def taps(dst: int, src: int):
    """(p0, p1, f), [dst] int64 each: the two tile pixels of every output pixel along one axis and the weight of p1 in 1/256"""
    o = np.arange(dst, dtype=np.int64)
    D = 2 * dst
    U = np.clip((2 * o + 1) * src - dst, 0, (src - 1) * D)
    p0 = U // D
    return p0, np.minimum(p0 + 1, src - 1), (256 * (U - p0 * D)) // D


def samples(t: np.ndarray, flags: int, out_w: int, out_h: int) -> np.ndarray:
    """t [n][tile_h][tile_w][4] u8 -> S_v(x, y, c) as [n][out_h][out_w][3] int64"""
    tile_h, tile_w = t.shape[1:3]
    t = t[..., :3].astype(np.int64)
    if not flags & BILINEAR:
        return t[:, ref.nearest(out_h, tile_h)][:, :, ref.nearest(out_w, tile_w)]
    x0, x1, fx = taps(out_w, tile_w)
    y0, y1, fy = taps(out_h, tile_h)
    fx, fy = fx[None, None, :, None], fy[None, :, None, None]
    h0 = (256 - fx) * t[:, y0][:, :, x0] + fx * t[:, y0][:, :, x1]
    h1 = (256 - fx) * t[:, y1][:, :, x0] + fx * t[:, y1][:, :, x1]
    return ((256 - fy) * h0 + fy * h1 + (1 << 15)) >> 16


def native(views: np.ndarray, lens: Lens, v0: int, out_w: int, out_h: int, tile_w: int, tile_h: int) -> np.ndarray:
    """views [V][H][W][4] u8 -> the native image [out_h][out_w][4] u8 under lens.flags"""
    t = ref.tiles(views[v0:v0 + lens.views], tile_w, tile_h)
    assert len(t) == lens.views
    S = samples(t, lens.flags, out_w, out_h)
    ka, kb, wb = selection(lens, out_w, out_h)
    y = np.arange(out_h)[:, None, None]
    x = np.arange(out_w)[None, :, None]
    c = np.arange(3)[None, None, :]
    out = np.full((out_h, out_w, 4), 255, np.uint8)
    out[..., :3] = ((256 - wb) * S[ka, y, x, c] + wb * S[kb, y, x, c] + 128) >> 8
    return out


def native_slow(views: np.ndarray, lens: Lens, v0: int, out_w: int, out_h: int, tile_w: int, tile_h: int) -> np.ndarray:
    """the definition as it is written: a loop over y, x and c in Python integers (tiny cases only)"""
    H, W = views.shape[1:3]
    n, flags = lens.views, lens.flags
    t = {}

    def tile(q):
        if flags & INVERT:
            q = n - 1 - q
        if q not in t:
            t[q] = (views[v0 + q] if (tile_w, tile_h) == (W, H) else quilt_ref.resize_dense(views[v0 + q], tile_w, tile_h)).astype(object)
        return t[q]

    def axis(o, src, dst):
        D = 2 * dst
        U = min(max((2 * o + 1) * src - dst, 0), (src - 1) * D)
        p0 = U // D
        return p0, min(p0 + 1, src - 1), (256 * (U - p0 * D)) // D

    def sample(q, x, y, c):
        T = tile(q)
        if not flags & BILINEAR:
            return int(T[((2 * y + 1) * tile_h) // (2 * out_h)][((2 * x + 1) * tile_w) // (2 * out_w)][c])
        x0, x1, fx = axis(x, tile_w, out_w)
        y0, y1, fy = axis(y, tile_h, out_h)
        h0 = (256 - fx) * int(T[y0][x0][c]) + fx * int(T[y0][x1][c])
        h1 = (256 - fx) * int(T[y1][x0][c]) + fx * int(T[y1][x1][c])
        assert h0 < 1 << 24 and h1 < 1 << 24 and (256 - fy) * h0 + fy * h1 + (1 << 15) < 1 << 24
        return ((256 - fy) * h0 + fy * h1 + (1 << 15)) >> 16

    out = np.zeros((out_h, out_w, 4), np.uint8)
    for y in range(out_h):
        for x in range(out_w):
            for c in range(3):
                s = 2 - c if flags & BGR else c
                phase = (lens.phase0 + (3 * x + s) * lens.x_step + y * lens.y_step) % (1 << 32)
                P = phase * n
                k, f = P >> 32, (P >> 24) & 255
                if flags & BLEND:
                    if f >= 128:
                        ka, kb, wb = k, min(k + 1, n - 1), f - 128
                    else:
                        ka, kb, wb = max(k, 1) - 1, k, f + 128
                    out[y, x, c] = ((256 - wb) * sample(ka, x, y, c) + wb * sample(kb, x, y, c) + 128) >> 8
                else:
                    out[y, x, c] = sample(k, x, y, c)
            out[y, x, 3] = 255
    return out


# ---- the cases the CPU and the GPU tests share --------------------------------------------------------------------------------------------

OUTPUTS = ref.OUTPUTS + [(300, 3)]                    # … and a row that spans two workgroups
VIEW_RANGES = ref.VIEW_RANGES + [(8, 1), (2, 0)]      # (n, v0): … the 8 views the boundary step sets are made for, and the smallest blend
GPU_FLAG_SETS = [BILINEAR, BLEND, BGR, BILINEAR | BLEND, INVERT | BGR | BILINEAR | BLEND]   # what the GPU test runs every case under
CENTRES = (1 << 29, 0, 1 << 28)                       # n = 8: every subpixel exactly on a view's centre (f = 128)
