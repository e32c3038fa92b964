"""The definition of the YUV 4:2:0 frames of lfi_download_views_yuv420 / lfi_render_stream_yuv420 (include/lfi.h), restated in numpy integers.
Written from the definition; shares no code with the product.  tests/test_host_yuv.py holds the table against its derivation and the
properties the header states; the GPU tests compare the library's bytes with `frame` applied to the views' own downloads, byte for byte."""
import numpy as np

BT709, BT601 = 0, 1
LIMITED, FULL = 0, 1
FORMATS = [(m, r) for m in (BT709, BT601) for r in (LIMITED, FULL)]

# (matrix, range): (Y (R, G, B), Cb (R, G, B), Cr (R, G, B), y_off) — the literals of the header
TABLE = {
    (BT709, LIMITED): ((11966, 40254, 4064), (-6596, -22188, 28784), (28784, -26145, -2639), 16),
    (BT709, FULL): ((13933, 46871, 4732), (-7509, -25259, 32768), (32768, -29763, -3005), 0),
    (BT601, LIMITED): ((16829, 33039, 6416), (-9714, -19070, 28784), (28784, -24103, -4681), 16),
    (BT601, FULL): ((19595, 38470, 7471), (-11058, -21710, 32768), (32768, -27439, -5329), 0),
}


def sizes(w, h):
    """(cw, ch, frame_bytes)"""
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    return cw, ch, w * h + 2 * cw * ch


def planes(rgba, matrix, rng, clamp=True):
    """(Y [H][W], Cb [ch][cw], Cr [ch][cw]) of an [H][W][>=3] uint8 image, as int64; clamp=False: the chroma before min(255, .)"""
    ky, kb, kr, y_off = TABLE[(matrix, rng)]
    p = np.asarray(rgba)[..., :3].astype(np.int64)
    h, w = p.shape[:2]
    cw, ch, _ = sizes(w, h)
    y = y_off + ((ky[0] * p[..., 0] + ky[1] * p[..., 1] + ky[2] * p[..., 2] + (1 << 15)) >> 16)
    ys = np.minimum(2 * np.arange(ch)[:, None] + np.arange(2)[None, :], h - 1)      # [ch][2]: the two rows of a chroma sample
    xs = np.minimum(2 * np.arange(cw)[:, None] + np.arange(2)[None, :], w - 1)      # [cw][2]
    s = p[ys[:, None, :, None], xs[None, :, None, :]].sum(axis=(2, 3))              # [ch][cw][3]: sums over the four pixels
    out = []
    for k in (kb, kr):
        bracket = (1 << 25) + (1 << 17) + k[0] * s[..., 0] + k[1] * s[..., 1] + k[2] * s[..., 2]
        assert (bracket > 0).all() and (bracket < 1 << 27).all()
        c = bracket >> 18
        out.append(np.minimum(c, 255) if clamp else c)
    return y, out[0], out[1]


def frame(rgba, matrix, rng):
    """the I420 frame of one view: Y, Cb, Cr tightly packed, uint8 [frame_bytes]"""
    y, cb, cr = planes(rgba, matrix, rng)
    assert 0 <= y.min() and y.max() <= 255
    return np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)]).astype(np.uint8)


def frames(views, matrix, rng):
    return np.stack([frame(v, matrix, rng) for v in views])


def corner_views(w, h, n):
    """n RGBA views of w x h for the extremes: 2x2 blocks that hold the 8 cube corners in EVERY arrangement (8^4 blocks, walked in an order
    that differs per view, wrapped over the views' blocks), followed by uniform blocks of the 8 corners and of greys — the inputs that reach
    16, 235, 240 and the 255 clamp.  Odd sizes cut the last blocks."""
    corners = np.array([[255 * (c & 1), 255 * (c >> 1 & 1), 255 * (c >> 2 & 1)] for c in range(8)], np.uint8)
    bw, bh = (w + 1) // 2, (h + 1) // 2
    per_view = bw * bh
    out = np.zeros((n, 2 * bh, 2 * bw, 4), np.uint8)
    out[..., 3] = 255
    k = np.arange(n * per_view).reshape(n, bh, bw)
    uniform = k % 3 == 2                      # every third block uniform: a corner, or a grey
    # the other blocks, numbered m = 0, 1, …: arrangement m·2731 mod 4096 (2731 is odd: any 4096 consecutive blocks hold every arrangement)
    mixed = ((k // 3 * 2 + k % 3) * 2731) % 4096
    for j in range(2):
        for i in range(2):
            pick = np.where(uniform, (k // 6) % 8, (mixed >> (3 * (2 * j + i))) & 7)
            colour = corners[pick]
            grey = ((k // 6) * 37 % 256).astype(np.uint8)
            is_grey = uniform & ((k // 3) % 2 == 1)
            colour = np.where(is_grey[..., None], grey[..., None], colour)
            out[:, j::2, i::2, :3] = colour
    return np.ascontiguousarray(out[:, :h, :w])
