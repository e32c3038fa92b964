"""LEFT-sited chroma (lfi_set_yuv_siting, include/lfi.h: MPEG-2 / H.264 siting, Y4M's C420mpeg2), both directions, restated in numpy int64.
Written from the header's text; shares no code with the product.  Everything the header leaves as it is under left siting — the tables, the
luma, the geometry, the conversion of chroma in sixteenths to RGBA — is taken from tests/yuv_ref.py and tests/yuv_in_ref.py."""
import numpy as np

import yuv_in_ref as in_ref
import yuv_ref as out_ref

BT709, BT601, LIMITED, FULL = out_ref.BT709, out_ref.BT601, out_ref.LIMITED, out_ref.FULL
BILINEAR, NEAREST = in_ref.BILINEAR, in_ref.NEAREST
FORMATS = out_ref.FORMATS


# ---- output: views -> frames ----------------------------------------------------------------------------------------------------------------------

def sums(rgba):
    """[ch][cw][3] int64: Σ_j [C(xl, y_j) + 2·C(xc, y_j) + C(xr, y_j)], xl = max(2cx − 1, 0), xc = 2cx, xr = min(2cx + 1, W − 1),
    y_j = min(2cy + j, H − 1)"""
    p = np.asarray(rgba)[..., :3].astype(np.int64)
    h, w = p.shape[:2]
    cw, ch, _ = out_ref.sizes(w, h)
    cx, cy = np.arange(cw), np.arange(ch)
    xl, xc, xr = np.maximum(2 * cx - 1, 0), 2 * cx, np.minimum(2 * cx + 1, w - 1)
    s = np.zeros((ch, cw, 3), np.int64)
    for j in range(2):
        rows = p[np.minimum(2 * cy + j, h - 1)]   # [ch][W][3]
        s += rows[:, xl] + 2 * rows[:, xc] + rows[:, xr]
    return s


def bracket(k, s):
    """2²⁶ + 2¹⁸ + uR·ΣR + uG·ΣG + uB·ΣB of a coefficient row k"""
    s = np.asarray(s, np.int64)
    return (1 << 26) + (1 << 18) + k[0] * s[..., 0] + k[1] * s[..., 1] + k[2] * s[..., 2]


def planes(rgba, matrix, rng, clamp=True):
    """(Y, Cb, Cr) as int64; Y is the centre-sited definition's (luma does not move)"""
    _, kb, kr, _ = out_ref.TABLE[(matrix, rng)]
    y = out_ref.planes(rgba, matrix, rng)[0]
    s = sums(rgba)
    out = []
    for k in (kb, kr):
        b = bracket(k, s)
        assert (b > 0).all() and (b <= 1 << 28).all()
        c = b >> 19
        out.append(np.minimum(c, 255) if clamp else c)
    return y, out[0], out[1]


def frame(rgba, matrix, rng):
    """the left-sited I420 frame of one view, uint8 [frame_bytes]"""
    return in_ref.pack(*planes(rgba, matrix, rng))


def frames(views, matrix, rng):
    return np.stack([frame(v, matrix, rng) for v in views])


# ---- input: frames -> images ----------------------------------------------------------------------------------------------------------------------

def chroma16(plane, w, h, chroma):
    """the chroma of every pixel in sixteenths, [H][W] int64: h(r) = 4·U[r][cx] (even x), 2·U[r][cx] + 2·U[r][min(cx + 1, cw − 1)] (odd x);
    SU = 3·h(cy) + h(ny).  NEAREST: 16·U[cy][cx], the same under either siting"""
    plane = np.asarray(plane, np.int64)
    if chroma == NEAREST:
        return in_ref.chroma16(plane, w, h, NEAREST)
    ch, cw = plane.shape
    x, y = np.arange(w), np.arange(h)
    cx, cy = x >> 1, y >> 1
    ny = np.clip(cy + np.where(y & 1, 1, -1), 0, ch - 1)
    hrow = np.where((x & 1)[None, :] == 0, 4 * plane[:, cx], 2 * plane[:, cx] + 2 * plane[:, np.minimum(cx + 1, cw - 1)])   # [ch][W]
    return 3 * hrow[cy] + hrow[ny]


def rgba(frame, w, h, matrix, rng, chroma=BILINEAR):
    y, cb, cr = in_ref.split(frame, w, h)
    return in_ref.convert(y, chroma16(cb, w, h, chroma), chroma16(cr, w, h, chroma), matrix, rng)


def images(frames, w, h, matrix, rng, chroma=BILINEAR):
    return np.stack([rgba(f, w, h, matrix, rng, chroma) for f in frames])
