"""The 10-bit YUV 4:2:0 definitions of include/lfi.h (LFI_YUV_I010, LFI_YUV_P010) restated in numpy int64: views -> frames and frames ->
images under both sitings, and where the samples of an I010 or P010 surface lie.  Written from the header's text; shares no code with the
product.  A frame is handled as its CODES: uint16 [W·H + 2·cw·ch], the Y plane, then Cb, then Cr (values 0 … 1023); `scatter` and `gather`
turn codes into the bytes of surfaces and back."""
from dataclasses import dataclass

import numpy as np

BT709, BT601 = 0, 1
LIMITED, FULL = 0, 1
BILINEAR, NEAREST = 0, 1
CENTRE, LEFT = 0, 1
FORMATS = [(m, r) for m in (BT709, BT601) for r in (LIMITED, FULL)]
I010, P010 = 0x100, 0x101   # LFI_YUV_I010, LFI_YUV_P010
HOST, DEVICE = 0, 1

# (matrix, range): (Y (R, G, B), Cb (R, G, B), Cr (R, G, B), y_off10) — the literals of the header, 14 fractional bits
OUT_TABLE = {
    (BT709, LIMITED): ((11966, 40254, 4064), (-6596, -22188, 28784), (28784, -26145, -2639), 64),
    (BT709, FULL): ((13974, 47009, 4746), (-7531, -25333, 32864), (32864, -29851, -3013), 0),
    (BT601, LIMITED): ((16829, 33039, 6416), (-9714, -19070, 28784), (28784, -24103, -4681), 64),
    (BT601, FULL): ((19653, 38583, 7493), (-11091, -21773, 32864), (32864, -27519, -5345), 0),
}
# (matrix, range): (cY, rV, gU, gV, bU, y_off) — the literals of the header, 16 fractional bits
IN_TABLE = {
    (BT709, LIMITED): (19077, 29372, -3494, -8731, 34610, 64),
    (BT709, FULL): (16336, 25726, -3060, -7647, 30313, 0),
    (BT601, LIMITED): (19077, 26149, -6419, -13320, 33050, 64),
    (BT601, FULL): (16336, 22903, -5622, -11666, 28947, 0),
}
BRACKET_BOUND = 576_213_136   # |l + … + 2^19| over all 10-bit code triples (the header's figure)


def sizes(w, h):
    """(cw, ch, samples of a frame)"""
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    return cw, ch, w * h + 2 * cw * ch


# ---- output: views -> frames ------------------------------------------------------------------------------------------------------------------

def luma(rgb, matrix, rng):
    """Y10 of [..., >= 3] R, G, B"""
    ky, _, _, y_off = OUT_TABLE[(matrix, rng)]
    p = np.asarray(rgb)[..., :3].astype(np.int64)
    return y_off + ((ky[0] * p[..., 0] + ky[1] * p[..., 1] + ky[2] * p[..., 2] + (1 << 13)) >> 14)


def sums(rgba, siting):
    """[ch][cw][3] int64: centre the sums over the 2 x 2 block (weight 4), left Σ_j [C(xl, y_j) + 2·C(xc, y_j) + C(xr, y_j)] (weight 8); an odd
    last column or row replicated"""
    p = np.asarray(rgba)[..., :3].astype(np.int64)
    h, w = p.shape[:2]
    cw, ch, _ = sizes(w, h)
    cx, cy = np.arange(cw), np.arange(ch)
    s = np.zeros((ch, cw, 3), np.int64)
    for j in range(2):
        rows = p[np.minimum(2 * cy + j, h - 1)]   # [ch][W][3]
        if siting == LEFT:
            s += rows[:, np.maximum(2 * cx - 1, 0)] + 2 * rows[:, 2 * cx] + rows[:, np.minimum(2 * cx + 1, w - 1)]
        else:
            s += rows[:, 2 * cx] + rows[:, np.minimum(2 * cx + 1, w - 1)]
    return s


def chroma(k, s, siting, clamp=True):
    """C10 of a coefficient row k and sums s"""
    s = np.asarray(s, np.int64)
    e = 1 if siting == LEFT else 0
    b = (1 << (25 + e)) + (1 << (15 + e)) + k[0] * s[..., 0] + k[1] * s[..., 1] + k[2] * s[..., 2]
    assert (b > 0).all() and (b <= 1 << (27 + e)).all()   # u32, as the header says
    c = b >> (16 + e)
    return np.minimum(c, 1023) if clamp else c


def codes(rgba, matrix, rng, siting=CENTRE):
    """the codes of one view's frame, uint16 [samples]"""
    _, kb, kr, _ = OUT_TABLE[(matrix, rng)]
    s = sums(rgba, siting)
    planes = [luma(rgba, matrix, rng), chroma(kb, s, siting), chroma(kr, s, siting)]
    return np.concatenate([p.reshape(-1) for p in planes]).astype(np.uint16)


def frames(views, matrix, rng, siting=CENTRE):
    return np.stack([codes(v, matrix, rng, siting) for v in views])


# ---- input: frames -> images ------------------------------------------------------------------------------------------------------------------

def split(frame, w, h):
    """(Y [H][W], Cb [ch][cw], Cr [ch][cw]) of a frame's codes, int64"""
    cw, ch, n = sizes(w, h)
    f = np.asarray(frame)[:n].astype(np.int64)
    return f[:w * h].reshape(h, w), f[w * h:w * h + cw * ch].reshape(ch, cw), f[w * h + cw * ch:].reshape(ch, cw)


def chroma16(plane, w, h, filt, siting):
    """the chroma of every pixel in sixteenths, [H][W] int64"""
    plane = np.asarray(plane, np.int64)
    ch, cw = plane.shape
    x, y = np.arange(w), np.arange(h)
    cx, cy = x >> 1, y >> 1
    if filt == NEAREST:
        return 16 * plane[cy[:, None], cx[None, :]]
    ny = np.clip(cy + np.where(y & 1, 1, -1), 0, ch - 1)
    if siting == LEFT:
        hrow = np.where((x & 1)[None, :] == 0, 4 * plane[:, cx], 2 * plane[:, cx] + 2 * plane[:, np.minimum(cx + 1, cw - 1)])   # [ch][W]
        return 3 * hrow[cy] + hrow[ny]
    nx = np.clip(cx + np.where(x & 1, 1, -1), 0, cw - 1)
    return (9 * plane[cy[:, None], cx[None, :]] + 3 * plane[cy[:, None], nx[None, :]] + 3 * plane[ny[:, None], cx[None, :]]
            + plane[ny[:, None], nx[None, :]])


def brackets(y, su, sv, matrix, rng):
    """the three brackets WITH the rounding term, int64"""
    c_y, r_v, g_u, g_v, b_u, y_off = IN_TABLE[(matrix, rng)]
    l = 16 * c_y * (np.asarray(y, np.int64) - y_off) + (1 << 19)
    u, v = np.asarray(su, np.int64) - 8192, np.asarray(sv, np.int64) - 8192
    return l + r_v * v, l + g_u * u + g_v * v, l + b_u * u


def convert(y, su, sv, matrix, rng):
    """[..., 4] uint8 RGBA of luma codes and chroma in sixteenths"""
    out = [np.clip(b >> 20, 0, 255) for b in brackets(y, su, sv, matrix, rng)]   # >> on int64 floors
    out.append(np.full_like(out[0], 255))
    return np.stack(out, axis=-1).astype(np.uint8)


def rgba(frame, w, h, matrix, rng, filt=BILINEAR, siting=CENTRE):
    """[H][W][4] uint8: the image of one frame's codes"""
    y, cb, cr = split(frame, w, h)
    return convert(y, chroma16(cb, w, h, filt, siting), chroma16(cr, w, h, filt, siting), matrix, rng)


def images(frames_, w, h, matrix, rng, filt=BILINEAR, siting=CENTRE):
    return np.stack([rgba(f, w, h, matrix, rng, filt, siting) for f in frames_])


def extremes_frame(w, h):
    """codes of 2x2 blocks with Y in {0, 64, 940, 1023} x U, V in {0, 64, 512, 960, 1023}: every combination where the frame has room for the
    100 of them, walked again from the start where it has more"""
    cw, ch, _ = sizes(w, h)
    ys, cs = np.array([0, 64, 940, 1023]), np.array([0, 64, 512, 960, 1023])
    k = np.arange(ch * cw).reshape(ch, cw)
    y = np.repeat(np.repeat(ys[k % 4], 2, axis=0), 2, axis=1)[:h, :w]
    return np.concatenate([y.reshape(-1), cs[(k // 4) % 5].reshape(-1), cs[(k // 20) % 5].reshape(-1)]).astype(np.uint16)


# ---- surfaces: where the samples lie ------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Layout:
    fmt: int
    w: int
    h: int
    y_pitch: int
    c_offset: int
    c_pitch: int
    cr_offset: int
    frame_stride: int

    @property
    def extent(self):
        """the end of a frame's last plane"""
        ch = (self.h + 1) >> 1
        return (self.c_offset if self.fmt == P010 else self.cr_offset) + ch * self.c_pitch


def _up(v, a):
    return (v + a - 1) // a * a


def tight(fmt, w, h):
    """what lfi_yuv_surfaces_packed describes: two bytes per sample, nothing between them"""
    cw, ch, n = sizes(w, h)
    return Layout(fmt, w, h, 2 * w, 2 * w * h, 4 * cw if fmt == P010 else 2 * cw, 0 if fmt == P010 else 2 * (w * h + cw * ch), 2 * n)


def pitched(fmt, w, h, align=256, gap=256, tail=256):
    """a decoder's surface: pitches rounded up to `align`, `gap` bytes between the planes, `tail` bytes behind the frame"""
    cw, ch, _ = sizes(w, h)
    y_pitch = _up(2 * w, align)
    c_pitch = _up(4 * cw if fmt == P010 else 2 * cw, align)
    c_offset = h * y_pitch + gap
    cr_offset = 0 if fmt == P010 else c_offset + ch * c_pitch + gap
    end = (c_offset if fmt == P010 else cr_offset) + ch * c_pitch
    return Layout(fmt, w, h, y_pitch, c_offset, c_pitch, cr_offset, end + tail)


def _sample_offsets(lay):
    """the byte offset inside a frame of every sample, in the order of the codes (Y, Cb, Cr), int64 [samples]"""
    cw, ch, _ = sizes(lay.w, lay.h)
    y = (np.arange(lay.h)[:, None] * lay.y_pitch + 2 * np.arange(lay.w)[None, :]).reshape(-1)
    rows, cols = np.arange(ch)[:, None] * lay.c_pitch, np.arange(cw)[None, :]
    if lay.fmt == P010:
        cb, cr = lay.c_offset + rows + 4 * cols, lay.c_offset + rows + 4 * cols + 2
    else:
        cb, cr = lay.c_offset + rows + 2 * cols, lay.cr_offset + rows + 2 * cols
    return np.concatenate([y, cb.reshape(-1), cr.reshape(-1)])


def own_mask(lay):
    """[frame_stride] bool: the bytes of a frame that carry samples"""
    m = np.zeros(lay.frame_stride, bool)
    off = _sample_offsets(lay)
    m[off] = m[off + 1] = True
    return m


def words(code, fmt, junk=None):
    """the 16-bit words of codes: I010 the code in bits 9..0, P010 in bits 15..6; junk (uint16 of the same shape): what the other six bits hold"""
    code = np.asarray(code).astype(np.uint16)
    if fmt == P010:
        return (code << 6) | (0 if junk is None else np.asarray(junk, np.uint16) & 0x3F)
    return code | (0 if junk is None else np.asarray(junk, np.uint16) & 0xFC00)


def scatter(frames_, lay, poison, junk=None):
    """[n][frame_stride] uint8: the codes [n][samples] as little-endian words in surfaces of layout lay; every other byte is `poison`"""
    frames_ = np.asarray(frames_)
    n = frames_.shape[0]
    out = np.full((n, lay.frame_stride), poison, np.uint8)
    w16 = words(frames_[:, :sizes(lay.w, lay.h)[2]], lay.fmt, junk)
    off = _sample_offsets(lay)
    out[:, off] = (w16 & 0xFF).astype(np.uint8)
    out[:, off + 1] = (w16 >> 8).astype(np.uint8)
    return out


def gather(surfaces, lay):
    """[n][samples] uint16: the WORDS of surfaces [n][>= extent] as they lie, unused bits included, in the order of the codes"""
    surfaces = np.asarray(surfaces, np.uint8)
    off = _sample_offsets(lay)
    return surfaces[:, off].astype(np.uint16) | (surfaces[:, off + 1].astype(np.uint16) << 8)


def padding_holds(surfaces, lay, poison):
    """every byte outside the planes' own still holds the poison"""
    surfaces = np.asarray(surfaces, np.uint8)
    return bool((surfaces[:, ~own_mask(lay)[:surfaces.shape[1]]] == poison).all())


def descriptor(native, lay, memory, base, keep=None):
    """the lfi_yuv_surfaces of layout lay at address base"""
    return native.YuvSurfaces.make(lay.fmt, memory, base, lay.frame_stride, lay.y_pitch, lay.c_offset, lay.c_pitch, lay.cr_offset, keep=keep)
