"""Linear-light blending (LFI_FLAG_LINEAR_LIGHT: include/lfi.h) restated in numpy, and the renders both test modules check (tests/test_host_linear.py
on the restatement and the oracle alone, tests/test_gpu_linear.py on the device).  Written from the header's text; shares no code with the product.

The tables come from the header's formulas in float64: D[b] = fp16_RN(255 eotf(b / 255)), T[b] = fp32_RN(255 eotf((b - 0.5) / 255)).

STD is float32 arithmetic throughout: an fp16 D times an fp16 weight is exact in fp32 (11 + 11 bits), so fmaf(D, w, s) IS the float32 addition of the
exact product, which numpy reproduces.  The byte is E(s) = #{b in 1 ... 255 : T[b] <= s}.

TEN_WM is an interval: the exact sum S in float64, the accumulation bound eps of tests/ten_interval.py (2^-15 per addend, k_pad addends), and the
admitted bytes [E(max(0, S - eps)), E(S + eps)]."""
import numpy as np

import ten_interval

FLAG_LINEAR_LIGHT = 256   # LFI_FLAG_LINEAR_LIGHT
SEED = 0x1F1F
TRAJECTORY = "0.1,0.2,0.9,0.7"


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------------

def eotf(u):
    """IEC 61966-2-1, float64"""
    u = np.asarray(u, np.float64)
    return np.where(u <= 0.04045, u / 12.92, ((u + 0.055) / 1.055) ** 2.4)


def decode_exact():
    """255 eotf(b / 255) for b = 0 ... 255 in float64: what D rounds"""
    return 255.0 * eotf(np.arange(256, dtype=np.float64) / 255.0)


def threshold_exact():
    """255 eotf((b - 0.5) / 255) for b = 0 ... 255 in float64: what T rounds (entry 0 has no meaning)"""
    return 255.0 * eotf((np.arange(256, dtype=np.float64) - 0.5) / 255.0)


D16 = decode_exact().astype(np.float16)          # D[0 ... 255]
T32 = threshold_exact().astype(np.float32)[1:]   # T[1 ... 255]: T32[b - 1] = T[b]
IDENTITY_D = np.arange(256, dtype=np.float16)    # the tables that make the definition the flag-free render's


def encode(s):
    """E(s) = #{b in 1 ... 255 : T[b] <= s}; s float32 or float64 (T widened exactly).  uint8, the shape of s"""
    return np.searchsorted(T32.astype(np.float64), np.asarray(s, np.float64), side="right").astype(np.uint8)


def encode_identity(s):
    """the flag-free STD byte: rint(s) & 0xff"""
    return (np.rint(s).astype(np.int64) & 0xff).astype(np.uint8)


# ---- the definition -----------------------------------------------------------------------------------------------------------------------------

def samples(lf, focused):
    """[N][H][W][3] uint8: image g at pixel + focused_offsets[g], clamped to the frame"""
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
    """s [V][H][W][3] float32 (the STD chain), bytes [V][H][W][3] uint8 (STD), S [V][H][W][3] float64 (the exact sum)"""


def restate(lf, hp, identity=False):
    """the definition; identity: D[b] = b and E = rint & 0xff — the flag-free render"""
    lf = np.asarray(lf, np.uint8)
    n = lf.shape[0]
    w32 = weights_f32(hp.weights)
    d32 = (IDENTITY_D if identity else D16).astype(np.float32)
    px = samples(lf, hp.focused_offsets)
    s = np.zeros((w32.shape[0],) + px.shape[1:], np.float32)
    S = np.zeros(s.shape, np.float64)
    for g in range(n):
        dec = d32[px[g]]                                       # [H][W][3] float32
        prod = dec[None] * w32[:, g, None, None, None]         # exact: 11 x 11 bits
        s = s + prod                                           # float32 addition of the exact product: fmaf(D, w, s)
        S += dec.astype(np.float64)[None] * w32[:, g].astype(np.float64)[:, None, None, None]
    assert s.dtype == np.float32
    out = Restated()
    out.s, out.S = s, S
    out.bytes = encode_identity(s) if identity else encode(s)
    return out


def ten_interval_of(res, hp, n_images):
    """lo, hi [V][H][W][3] uint8: the bytes a TEN_WM linear-light render may write"""
    eps = ten_interval.epsilon(hp.weights, n_images)[:, None, None, None]
    return encode(np.maximum(0.0, res.S - eps)), encode(res.S + eps)


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


CASES = [
    # a ragged second tile (130 = 128 + 2); offsets that clamp at every edge
    ("g2x2_130x12", 2, 2, 130, 12, 3, np.array([(1, 3), (-1, -3), (7, 3), (-7, -3)], np.int32)),
    # one chunk of 64 images; 70 views: a second view pass of ONE launch
    ("g8x8_130x12_v70", 8, 8, 130, 12, 70, _spread(8, 8, 10, 5)),
    # two chunks (72 images): a launch per 64 views
    ("g9x8_130x12_v70", 9, 8, 130, 12, 70, _spread(9, 8, 10, 5)),
    # four chunks, 256 images
    ("g16x16_130x10", 16, 16, 130, 10, 3, _spread(16, 16, 10, 4)),
    # W below the tile
    ("g8x8_64x10", 8, 8, 64, 10, 3, _spread(8, 8, 3, 2)),
    # 1100 tiles, more than 2 x CUs: every workgroup walks its tile loop
    ("g2x2_64x1100", 2, 2, 64, 1100, 3, np.array([(0, 3), (0, -3), (2, 3), (-2, -3)], np.int32)),
]
CASE_IDS = [c[0] for c in CASES]
RAGGED = CASES[0]
ONE_CHUNK_70 = CASES[1]
TWO_CHUNKS_70 = CASES[2]
# the TEN_WM interval's two-valued share: at most 2 % up to 72 images, 6 % on the 256-image case (eps grows with k_pad) — tests/inframe_ref.py's caps
TWO_VALUED_CAP = {c[0]: (0.06 if c[1] * c[2] > 72 else 0.02) for c in CASES}

_inputs, _restated = {}, {}


def with_weights(L, hp, weights):
    return L.host.HostParams(hp.focused_offsets, hp.offsets, weights, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)


def inputs(L, oc, case):
    """(hp, lf) of a case: the host parameters with the case's integer offsets, and the synthetic light field the device fills itself with"""
    if case[0] not in _inputs:
        _, cols, rows, w, h, views, offs = case
        hp = L.build_params(cols, rows, w, h, TRAJECTORY, 0.0, 0.0, 3.0, 1.783, views)
        hp = L.host.HostParams(np.ascontiguousarray(offs, np.int32), hp.offsets, hp.weights, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)
        _inputs[case[0]] = (hp, oc.synthetic_lf(cols * rows, w, h, SEED))
    return _inputs[case[0]]


def restated(L, oc, case):
    """the restatement of a case, computed once and shared; nobody writes into it"""
    if case[0] not in _restated:
        hp, lf = inputs(L, oc, case)
        _restated[case[0]] = restate(lf, hp)
    return _restated[case[0]]


ONE_HOT = ((0, 5), (1, 63))     # (view, image): weight 1.0
HALVES = ((2, 3, 40),)          # (view, image, image): weights 0.5 and 0.5


def exact_rows(L, oc):
    """(hp, lf): the one-chunk case with rows 0 and 1 one-hot and row 2 two halves — every product and partial sum of those rows is exact in fp32
    whatever the order; the other rows keep the trajectory's weights"""
    hp, lf = inputs(L, oc, ONE_CHUNK_70)
    w = hp.weights.copy()
    one, half = np.float16(1.0).view(np.uint16), np.float16(0.5).view(np.uint16)
    for v, g in ONE_HOT:
        w[v, :] = 0
        w[v, g] = one
    for v, g0, g1 in HALVES:
        w[v, :] = 0
        w[v, g0] = w[v, g1] = half
    return with_weights(L, hp, w), lf
