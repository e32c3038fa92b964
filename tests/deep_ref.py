"""Deep views (LFI_FLAG_DEEP_VIEWS, LFI_YUV_DEEP: include/lfi.h) restated in numpy: the 10-bit codes of both methods, the deep -> 10-bit YUV
definitions under both sitings, and the GBRP10 packing.  Written from the header's text; shares no code with the product.  A YUV frame is handled
as its CODES like tests/yuv10_ref.py's: uint16 [W·H + 2·cw·ch], the Y plane, then Cb, then Cr; that module's layouts, `gather`, `words` and
`padding_holds` say where the samples of an I010 / P010 surface lie, whatever made them."""
from fractions import Fraction

import numpy as np

BT709, BT601 = 0, 1
LIMITED, FULL = 0, 1
CENTRE, LEFT = 0, 1
FORMATS = [(m, r) for m in (BT709, BT601) for r in (LIMITED, FULL)]
DEEP = 0x200                                   # LFI_YUV_DEEP
I010_DEEP, P010_DEEP, GBRP10 = 0x300, 0x301, 0x304
FLAG_DEEP_VIEWS = 64                           # LFI_FLAG_DEEP_VIEWS
POISON_DEEP = 64                               # LFI_POISON_DEEP

# (matrix, range): (Y (R, G, B), Cb (R, G, B), Cr (R, G, B), y_off10) — the literals of the header, 16 fractional bits
TABLE = {
    (BT709, LIMITED): ((11931, 40137, 4052), (-6576, -22124, 28700), (28700, -26068, -2632), 64),
    (BT709, FULL): ((13933, 46871, 4732), (-7509, -25259, 32768), (32768, -29763, -3005), 0),
    (BT601, LIMITED): ((16780, 32942, 6398), (-9685, -19015, 28700), (28700, -24033, -4667), 64),
    (BT601, FULL): ((19595, 38470, 7471), (-11058, -21710, 32768), (32768, -27439, -5329), 0),
}
Y_SUM = {LIMITED: 56120, FULL: 65536}
# the header's bounds of the brackets: luma below 2^26; chroma in (0, 2^28] (centre) and (0, 2^29] (left), the upper ends reached
LUMA_BOUND = 1 << 26
CHROMA_BOUND = {CENTRE: 1 << 28, LEFT: 1 << 29}
KR_KB = {BT709: (Fraction(2126, 10000), Fraction(722, 10000)), BT601: (Fraction(299, 1000), Fraction(114, 1000))}


def _round(x):
    """round half away from zero of a Fraction"""
    return int(x + Fraction(1, 2)) if x >= 0 else -int(-x + Fraction(1, 2))


def rule(matrix, rng):
    """the header's rule: round(c · scale · 2^16), scale 876/1023 (limited luma), 896/1023 (limited chroma), 1 (full); G adjusted so that Y sums
    to 56120 / 65536 and Cb, Cr to 0"""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    sy, sc = (Fraction(876, 1023), Fraction(896, 1023)) if rng == LIMITED else (Fraction(1), Fraction(1))
    y = [_round(c * sy * 65536) for c in (kr, kg, kb)]
    cb = [_round(c * sc * 65536) for c in (-kr / (2 * (1 - kb)), -kg / (2 * (1 - kb)), Fraction(1, 2))]
    cr = [_round(c * sc * 65536) for c in (Fraction(1, 2), -kg / (2 * (1 - kr)), -kb / (2 * (1 - kr)))]
    y[1] = Y_SUM[rng] - y[0] - y[2]
    cb[1], cr[1] = -cb[0] - cb[2], -cr[0] - cr[2]
    return tuple(y), tuple(cb), tuple(cr), 64 if rng == LIMITED else 0


# ---- the codes --------------------------------------------------------------------------------------------------------------------------------

def q10_std(prequant):
    """D10 = min(1023, rn_even(4·s)) of the fp32 chain's value s (4·s is exact in fp32; np.rint rounds half to even)"""
    s = np.asarray(prequant, np.float32)
    return np.minimum(1023, np.rint(s * np.float32(4.0)).astype(np.int64)).astype(np.uint16)


def q10_ten(s):
    """q10(s) = min(1023, floor(4·fp16_RN(s))): float64 -> float16 (round to nearest even, one rounding), times four (exact), truncate.  Monotone;
    q10(s) >> 2 is the TEN_WM byte floor(min(fp16_RN(s), 255)) (tests/ten_interval.quantise)"""
    with np.errstate(over="ignore"):
        h = np.asarray(s, np.float64).astype(np.float16).astype(np.float64)
    return np.minimum(1023, np.floor(4.0 * np.maximum(h, 0.0))).astype(np.uint16)


def interval10(S, eps):
    """lo, hi (uint16, the shape of S): the codes q10 admits for a sum within eps ([V] or a scalar) of S"""
    e = np.asarray(eps, np.float64)
    e = e.reshape(e.shape + (1,) * (S.ndim - e.ndim))
    return q10_ten(S - e), q10_ten(S + e)


# ---- deep -> 10-bit YUV -------------------------------------------------------------------------------------------------------------------------

def sizes(w, h):
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    return cw, ch, w * h + 2 * cw * ch


def luma_bracket(rgb, matrix, rng):
    ky = TABLE[(matrix, rng)][0]
    p = np.asarray(rgb)[..., :3].astype(np.int64)
    return ky[0] * p[..., 0] + ky[1] * p[..., 1] + ky[2] * p[..., 2] + (1 << 15)


def luma(rgb, matrix, rng):
    """Y10 of [..., 3] R, G, B codes"""
    b = luma_bracket(rgb, matrix, rng)
    assert (b >= 0).all() and (b < LUMA_BOUND).all()
    return TABLE[(matrix, rng)][3] + (b >> 16)


def sums(rgb, siting):
    """[ch][cw][3] int64: centre the sums over the 2 x 2 block (weight 4), left Σ_j [C(xl, y_j) + 2·C(xc, y_j) + C(xr, y_j)] (weight 8); an odd
    last column or row replicated"""
    p = np.asarray(rgb)[..., :3].astype(np.int64)
    h, w = p.shape[:2]
    cw, ch, _ = sizes(w, h)
    cx, cy = np.arange(cw), np.arange(ch)
    s = np.zeros((ch, cw, 3), np.int64)
    for j in range(2):
        rows = p[np.minimum(2 * cy + j, h - 1)]
        if siting == LEFT:
            s += rows[:, np.maximum(2 * cx - 1, 0)] + 2 * rows[:, 2 * cx] + rows[:, np.minimum(2 * cx + 1, w - 1)]
        else:
            s += rows[:, 2 * cx] + rows[:, np.minimum(2 * cx + 1, w - 1)]
    return s


def chroma_bracket(k, s, siting):
    s = np.asarray(s, np.int64)
    e = 1 if siting == LEFT else 0
    return (1 << (27 + e)) + (1 << (17 + e)) + k[0] * s[..., 0] + k[1] * s[..., 1] + k[2] * s[..., 2]


def chroma(k, s, siting):
    """C10 of a coefficient row k and sums s"""
    b = chroma_bracket(k, s, siting)
    assert (b > 0).all() and (b <= CHROMA_BOUND[siting]).all()   # u32, as the header says
    return np.minimum(b >> (18 + (1 if siting == LEFT else 0)), 1023)


def codes(rgb, matrix, rng, siting=CENTRE):
    """the codes of one deep view's frame ([H][W][3] R, G, B codes), uint16 [samples]"""
    _, kb, kr, _ = TABLE[(matrix, rng)]
    s = sums(rgb, siting)
    planes = [luma(rgb, matrix, rng), chroma(kb, s, siting), chroma(kr, s, siting)]
    return np.concatenate([p.reshape(-1) for p in planes]).astype(np.uint16)


def frames(deep_views, matrix, rng, siting=CENTRE):
    return np.stack([codes(v, matrix, rng, siting) for v in deep_views])


# ---- GBRP10 ---------------------------------------------------------------------------------------------------------------------------------------

def gbrp10(deep_views):
    """[n][3: G, B, R][H][W] uint16 of [n][H][W][3: R, G, B]: ffmpeg's gbrp10le, the code in bits 9..0 and zeros above"""
    d = np.asarray(deep_views, np.uint16)
    return np.ascontiguousarray(d[..., [1, 2, 0]].transpose(0, 3, 1, 2))


def gbrp10_bytes(deep_views, y_pitch, c_offset, c_pitch, cr_offset, frame_stride, poison):
    """[n][frame_stride] uint8: the planes of gbrp10 as little-endian words in pitched surfaces; every other byte is `poison`"""
    planes = gbrp10(deep_views)
    n, _, h, w = planes.shape
    out = np.full((n, frame_stride), poison, np.uint8)
    for p, (off, pitch) in enumerate(((0, y_pitch), (c_offset, c_pitch), (cr_offset, c_pitch))):
        raw = planes[:, p].astype("<u2").view(np.uint8).reshape(n, h, 2 * w)
        for y in range(h):
            out[:, off + y * pitch:off + y * pitch + 2 * w] = raw[:, y]
    return out


# ---- the renders both test modules check (tests/test_host_deep.py on the oracle alone, tests/test_gpu_deep.py on the device) ------------------
# (name, cols, rows, W, H, views, trajectory, focus, aspect, effect).  W = 130: one 128-pixel tile plus two pixels; 64: half a tile.  2 x 2: a
# chunk of 16 images; 8 x 8: one full chunk; 9 x 8: two chunks, the second ragged (72 images, 80 padded); 16 x 16: four chunks.  3 views: a
# quarter of one wave's 16; 64: one pass; 70: a second view pass (one chunk: inside the launch; two chunks: a second launch)
CASES = [
    ("g2x2_130x5_v3", 2, 2, 130, 5, 3, "0,0,1,1", 0.23, 1.783, 3.0),
    ("g8x8_130x5_v64", 8, 8, 130, 5, 64, "0.0,0.0,1.0,1.0", 0.23, 1.783, 3.0),
    ("g8x8_64x5_v70", 8, 8, 64, 5, 70, "0.1,0.2,0.9,0.7", 0.31, 1.783, 3.0),
    ("g9x8_64x5_v70", 9, 8, 64, 5, 70, "0,0.5,1,0.5", 0.23, 1.783, 3.0),
    ("g16x16_64x4_v3", 16, 16, 64, 4, 3, "0.071,0.071,0.93,0.93", 0.23, 1.8266, 7.0),
    # persistent: 1100 tiles, more than the two workgroups per CU of the grid (512 on 256 CUs), so every workgroup walks on to a second and
    # a third tile — the buffer swap, the re-cleared accumulators and the t + G addressing across tiles — with one chunk and with two
    ("g2x2_64x1100_v3", 2, 2, 64, 1100, 3, "0,0,1,1", 0.23, 1.783, 3.0),
    ("g9x8_64x1100_v3", 9, 8, 64, 1100, 3, "0,0.5,1,0.5", 0.23, 1.783, 3.0),
]
CASE_IDS = [c[0] for c in CASES]
SEED = 0x1F1F
_inputs = {}


def inputs(L, oc, case):
    """(hp, lf) of a case: the host parameters and the synthetic light field the device fills itself with (seed SEED); computed once"""
    if case[0] not in _inputs:
        _, cols, rows, w, h, views, trajectory, focus, aspect, effect = case
        _inputs[case[0]] = (L.build_params(cols, rows, w, h, trajectory, focus, 0.0, effect, aspect, views), oc.synthetic_lf(cols * rows, w, h, SEED))
    return _inputs[case[0]]
