"""The definition of lfi_upload_images_yuv420's conversion (include/lfi.h) — 8-bit YUV 4:2:0 frames to RGBA — restated in numpy int64.
Written from the definition; shares no code with the product.  tests/test_host_yuv_in.py holds the table against its derivation and the
properties the header states; the GPU tests compare the grid's bytes with `rgba` applied to the frames they uploaded, byte for byte."""
import numpy as np

BT709, BT601 = 0, 1
LIMITED, FULL = 0, 1
BILINEAR, NEAREST = 0, 1
FORMATS = [(m, r) for m in (BT709, BT601) for r in (LIMITED, FULL)]

# (matrix, range): (cY, rV, gU, gV, bU, y_off) — the literals of the header
TABLE = {
    (BT709, LIMITED): (76309, 117489, -13975, -34925, 138438, 16),
    (BT709, FULL): (65536, 103206, -12276, -30679, 121609, 0),
    (BT601, LIMITED): (76309, 104597, -25675, -53279, 132201, 16),
    (BT601, FULL): (65536, 91881, -22553, -46802, 116130, 0),
}
BRACKET_BOUND = 573_111_632   # |l + …| before the rounding term, over all byte triples (the header's figure)


def sizes(w, h):
    """(cw, ch, frame_bytes)"""
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    return cw, ch, w * h + 2 * cw * ch


def split(frame, w, h):
    """(Y [H][W], Cb [ch][cw], Cr [ch][cw]) of a frame's bytes, int64"""
    cw, ch, fb = sizes(w, h)
    f = np.asarray(frame)[:fb].astype(np.int64)
    return f[:w * h].reshape(h, w), f[w * h:w * h + cw * ch].reshape(ch, cw), f[w * h + cw * ch:].reshape(ch, cw)


def pack(y, cb, cr):
    """the frame's bytes of its three planes"""
    return np.concatenate([np.asarray(y).reshape(-1), np.asarray(cb).reshape(-1), np.asarray(cr).reshape(-1)]).astype(np.uint8)


def chroma16(plane, w, h, chroma):
    """the chroma of every pixel in sixteenths, [H][W] int64"""
    ch, cw = plane.shape
    x, y = np.arange(w), np.arange(h)
    cx, cy = x >> 1, y >> 1
    if chroma == NEAREST:
        return 16 * plane[cy[:, None], cx[None, :]]
    nx = np.clip(cx + np.where(x & 1, 1, -1), 0, cw - 1)
    ny = np.clip(cy + np.where(y & 1, 1, -1), 0, ch - 1)
    return (9 * plane[cy[:, None], cx[None, :]] + 3 * plane[cy[:, None], nx[None, :]] + 3 * plane[ny[:, None], cx[None, :]]
            + plane[ny[:, None], nx[None, :]])


def brackets(y, su, sv, matrix, rng):
    """the three brackets before the rounding term, int64 arrays of the inputs' shape"""
    c_y, r_v, g_u, g_v, b_u, y_off = TABLE[(matrix, rng)]
    l = 16 * c_y * (np.asarray(y, np.int64) - y_off)
    u, v = np.asarray(su, np.int64) - 2048, np.asarray(sv, np.int64) - 2048
    return l + r_v * v, l + g_u * u + g_v * v, l + b_u * u


def convert(y, su, sv, matrix, rng):
    """[..., 4] uint8 RGBA of luma codes and chroma in sixteenths"""
    out = [np.clip((b + (1 << 19)) >> 20, 0, 255) for b in brackets(y, su, sv, matrix, rng)]   # >> on int64 floors
    out.append(np.full_like(out[0], 255))
    return np.stack(out, axis=-1).astype(np.uint8)


def rgba(frame, w, h, matrix, rng, chroma=BILINEAR):
    """[H][W][4] uint8: the image of one frame"""
    y, cb, cr = split(frame, w, h)
    return convert(y, chroma16(cb, w, h, chroma), chroma16(cr, w, h, chroma), matrix, rng)


def images(frames, w, h, matrix, rng, chroma=BILINEAR):
    return np.stack([rgba(f, w, h, matrix, rng, chroma) for f in frames])


def extremes_frame(w, h):
    """a frame of 2x2 blocks with Y in {0, 16, 235, 255} x U, V in {0, 16, 128, 240, 255}: every combination where the frame has room for the
    100 of them, walked again from the start where it has more"""
    cw, ch, _ = sizes(w, h)
    ys, cs = np.array([0, 16, 235, 255]), np.array([0, 16, 128, 240, 255])
    k = np.arange(ch * cw).reshape(ch, cw)
    y = np.repeat(np.repeat(ys[k % 4], 2, axis=0), 2, axis=1)[:h, :w]
    return pack(y, cs[(k // 4) % 5], cs[(k // 20) % 5])
