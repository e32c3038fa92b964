"""In-frame blending (LFI_FLAG_IN_FRAME: include/lfi.h) restated in numpy, and the renders both test modules check (tests/test_host_inframe.py on
the restatement and the oracle alone, tests/test_gpu_inframe.py on the device).  Written from the header's text; shares no code with the product.

STD is float32 arithmetic throughout: a byte times an fp16 weight is exact in fp32 (8 + 11 bits), so fmaf(px, w, acc) IS the float32 addition of the
exact product, which numpy reproduces; den, wall, r and s are float32 operations; the byte is rint(s) & 0xff.

TEN_WM is an interval: the exact masked sum S_N in float64, the accumulation bound eps of tests/ten_interval.py (2^-15 per addend, k_pad addends),
r the restatement's float32 quotient, and the admitted bytes [q(max(0, S_N - eps) * r * (1 - 2^-23)), q((S_N + eps) * r * (1 + 2^-23))]: the 2^-23 covers
the one fp32 rounding of the product (2^-24 relative) with a factor two to spare.  den == 0 admits only 0."""
import numpy as np

import ten_interval

FLAG_IN_FRAME = 128   # LFI_FLAG_IN_FRAME
SEED = 0x1F1F


def in_frame(focused, w, h):
    """[N][H][W] bool: image g has pixel (x, y) in frame — 0 <= x + ox_g < W and 0 <= y + oy_g < H"""
    foc = np.asarray(focused, np.int64)
    x, y = np.arange(w), np.arange(h)
    sx, sy = x[None, :] + foc[:, 0, None], y[None, :] + foc[:, 1, None]
    return ((sy >= 0) & (sy < h))[:, :, None] & ((sx >= 0) & (sx < w))[:, None, :]


def samples(lf, focused):
    """[N][H][W][3] uint8: image g at pixel + focused_offsets[g], clamped to the frame (what a left-out sample would have been)"""
    n, h, w, _ = lf.shape
    foc = np.asarray(focused, np.int64)
    out = np.empty((n, h, w, 3), np.uint8)
    for g in range(n):
        ys, xs = np.clip(np.arange(h) + foc[g, 1], 0, h - 1), np.clip(np.arange(w) + foc[g, 0], 0, w - 1)
        out[g] = lf[g][ys][:, xs, :3]
    return out


def weights_f32(weights_vn):
    return np.ascontiguousarray(weights_vn, np.uint16).view(np.float16).astype(np.float32)


class Restated:
    """bytes [V][H][W][3] uint8 (STD), prequant s [V][H][W][3] float32, num, den [V][H][W], wall [V], r [V][H][W] (all float32), and for TEN_WM
    S [V][H][W][3] float64, the exact masked sum"""


def restate(lf, hp, force_full=False):
    """the definition, both methods' parts; force_full: every mask full (the clamped samples all count) — the flag-free render"""
    lf = np.asarray(lf, np.uint8)
    n, h, w, _ = lf.shape
    w32 = weights_f32(hp.weights)
    v = w32.shape[0]
    mask = in_frame(hp.focused_offsets, w, h)
    if force_full:
        mask = np.ones_like(mask)
    px = samples(lf, hp.focused_offsets)
    num = np.zeros((v, h, w, 3), np.float32)
    den = np.zeros((v, h, w), np.float32)
    wall = np.zeros(v, np.float32)
    S = np.zeros((v, h, w, 3), np.float64)
    for g in range(n):
        wg = w32[:, g]
        prod = px[g].astype(np.float32)[None] * wg[:, None, None, None]   # exact
        m = mask[g][None]
        num = np.where(m[..., None], num + prod, num)                      # float32 addition of the exact product: fmaf(px, w, num)
        den = np.where(m, den + wg[:, None, None], den)
        wall = wall + wg
        S += np.where(m[..., None], px[g].astype(np.float64)[None] * wg.astype(np.float64)[:, None, None, None], 0.0)
    assert num.dtype == den.dtype == wall.dtype == np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        q = wall[:, None, None] / den
    r = np.where(den == 0, np.float32(0), q).astype(np.float32)
    s = num * r[..., None]
    assert s.dtype == np.float32
    out = Restated()
    out.num, out.den, out.wall, out.r, out.s, out.S = num, den, wall, r, s, S
    out.bytes = (np.rint(s).astype(np.int64) & 0xff).astype(np.uint8)
    out.all_in = mask.all(axis=0)        # [H][W]: every image has the pixel in frame
    out.none_in = ~mask.any(axis=0)      # [H][W]: no image has
    return out


def ten_interval_of(res, hp, n_images):
    """lo, hi [V][H][W][3] uint8: the bytes a TEN_WM in-frame render may write"""
    eps = ten_interval.epsilon(hp.weights, n_images)[:, None, None, None]
    r = res.r.astype(np.float64)[..., None]
    slack = np.where(r == 1.0, 0.0, 2.0 ** -23)   # r = 1 (every image in frame, or den == wall all the same): the product is exact, the ordinary interval
    lo = ten_interval.quantise(np.maximum(0.0, res.S - eps) * r * (1.0 - slack))
    hi = ten_interval.quantise((res.S + eps) * r * (1.0 + slack))
    zero = (res.den == 0)[..., None]
    return np.where(zero, 0, lo).astype(np.uint8), np.where(zero, 0, hi).astype(np.uint8)


def ten_exact(res):
    """q of the float32 restatement's s: what TEN_WM writes where every sum is exact whatever its order (dyadic weights)"""
    return ten_interval.quantise(res.s.astype(np.float64))


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------
# (name, cols, rows, W, H, views, offsets): the smallest shapes at which the kernel can go wrong.  Offsets are set explicitly: [N][2] (ox, oy).

def _spread(cols, rows, ax, ay):
    """image (cx, cy) of the grid at ox, oy spread linearly over [-ax, ax] x [-ay, ay] (rounded), row-major"""
    out = []
    for cy in range(rows):
        for cx in range(cols):
            fx = 0.0 if cols == 1 else 2.0 * cx / (cols - 1) - 1.0
            fy = 0.0 if rows == 1 else 2.0 * cy / (rows - 1) - 1.0
            out.append((int(round(fx * ax)), int(round(fy * ay))))
    return np.array(out, np.int32)


def _w64():
    o = _spread(8, 8, 3, 2)
    o[0], o[63], o[9] = (64, 0), (-64, 0), (0, 10)   # never in frame: ox = +W, ox = -W, oy = H
    return o


CASES = [
    # validity edges inside a lane's 8 pixels, on its boundary, one past it; rows out at top and bottom; a second, partial tile
    ("g2x2_130x12_a", 2, 2, 130, 12, 3, np.array([(1, 3), (-1, -3), (7, 3), (-7, -3)], np.int32)),
    ("g2x2_130x12_b", 2, 2, 130, 12, 3, np.array([(8, 3), (-8, -3), (9, -3), (-9, 3)], np.int32)),
    # one chunk of 64; 70 views: a second view pass (ranges of them: 3 views, 64 views, (5, 23))
    ("g8x8_130x12_v70", 8, 8, 130, 12, 70, _spread(8, 8, 10, 5)),
    # two chunks (72 images): den and wall carried across chunks; 70 views: a second launch
    ("g9x8_130x12_v70", 9, 8, 130, 12, 70, _spread(9, 8, 10, 5)),
    # four chunks, 256 images
    ("g16x16_130x10", 16, 16, 130, 10, 3, _spread(16, 16, 10, 4)),
    # W below the tile; three images never in frame
    ("g8x8_64x10", 8, 8, 64, 10, 3, _w64()),
    # columns 4 ... 19 have no image in frame and must be 0; the others are divided by a small den
    ("g2x2_24x6", 2, 2, 24, 6, 3, np.array([(20, 0), (22, 0), (-20, 0), (-22, 0)], np.int32)),
    # tile 1 is interior between two border tiles (and tile 3, ragged, a border tile again): both code paths in one launch
    ("g8x8_400x6", 8, 8, 400, 6, 3, _spread(8, 8, 8, 0)),
    # 1100 tiles: every one of the 512 workgroups walks from a border tile into interior ones and, at the bottom, back; one chunk and two
    ("g2x2_64x1100", 2, 2, 64, 1100, 3, np.array([(0, 3), (0, -3), (0, 3), (0, -3)], np.int32)),
    ("g9x8_64x1100", 9, 8, 64, 1100, 3, np.array([(0, 3 if g % 2 else -3) for g in range(72)], np.int32)),
]
CASE_IDS = [c[0] for c in CASES]
ONE_CHUNK_70 = CASES[2]
TWO_CHUNKS_70 = CASES[3]
NONE_IN_FRAME = CASES[6]
# the TEN_WM interval's two-valued share of the border bytes: at most 2 % up to 72 images, 6 % on the 256-image case (eps grows with k_pad)
TWO_VALUED_CAP = {c[0]: (0.06 if c[1] * c[2] > 72 else 0.02) for c in CASES}

_inputs, _restated = {}, {}


def inputs(L, oc, case):
    """(hp, lf) of a case: the host parameters with the case's integer offsets, and the synthetic light field the device fills itself with"""
    if case[0] not in _inputs:
        _, cols, rows, w, h, views, offs = case
        hp = L.build_params(cols, rows, w, h, "0.1,0.2,0.9,0.7", 0.0, 0.0, 3.0, 1.783, views)
        hp = L.host.HostParams(np.ascontiguousarray(offs, np.int32), hp.offsets, hp.weights, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)
        _inputs[case[0]] = (hp, oc.synthetic_lf(cols * rows, w, h, SEED))
    return _inputs[case[0]]


def restated(L, oc, case):
    """the restatement of a case, computed once and shared; nobody writes into it"""
    if case[0] not in _restated:
        hp, lf = inputs(L, oc, case)
        _restated[case[0]] = restate(lf, hp)
    return _restated[case[0]]


def dyadic(L, oc):
    """(hp, lf): the one-chunk case with weights 1/64 in row 0 — every product and partial sum exact in fp32 whatever the order"""
    hp, lf = inputs(L, oc, ONE_CHUNK_70)
    w = hp.weights[:1].copy()
    w[0, :] = np.float16(1.0 / 64).view(np.uint16)
    return L.host.HostParams(hp.focused_offsets, hp.offsets, w, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius), lf
