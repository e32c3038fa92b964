"""What a TEN_WM byte may be: the interval of the exact sum, instead of "within one LSB of M16".

Every TEN_WM kernel ends in the same quantisation q(s) = floor(min(fp16_RN(s), 255)) (epilogue_packed.hpp and the generic epilogue of
blend_ten.hpp), applied to a sum s that the matrix core accumulated in fp32.  q is monotone.  The exact sum S of fp16 weights × bytes over
at most 256 images has 41 bits and is exact in double (oracle: blend_f64).  If the accumulation error is at most ε, the kernel's s lies in
[S − ε, S + ε] and the only bytes it may write are [q(S − ε), q(S + ε)]: one value for ≥ 98.5 % of the bytes, two neighbours for the rest.

ε is not a new number: it is the analytic bound the STD band rests on (lfi_device.hpp std_accumulation_bound, LFI_FLAG_STD_ANALYTIC_BAND) —
one ulp of the largest partial sum per addend, "true of any accumulator that keeps 24 bits": 2^-15 per addend while the partial sums stay
below 512, k_pad addends (the zero-weight padding included).

A plain module like poison.py: `oc` is the oracle binding (oracle/lfi_oracle_c.py), `hp` the host parameters of lfi build_params.
"""
import numpy as np


def quantise(s):
    """q(s): float64 → float16 (round to nearest even, one rounding), saturate to [0, 255], truncate.  uint8, the shape of s."""
    with np.errstate(over="ignore"):
        h = np.asarray(s, np.float64).astype(np.float16)
    return np.floor(np.clip(h.astype(np.float64), 0.0, 255.0)).astype(np.uint8)


def weights_f64(weights_vn):
    """The fp16 bit patterns [V, n] of lfi_params.weights as doubles."""
    return np.ascontiguousarray(weights_vn, np.uint16).view(np.float16).astype(np.float64)


def epsilon(weights_vn, n_images):
    """The accumulation bound per view, [V] float64: k_pad · ulp_fp32(B_v), B_v = 255·Σ_k |w_vk| the largest partial sum a view's
    accumulation can reach (at least 512: below that the bound stays the STD band's 2^-15 per addend)."""
    k_pad = (int(n_images) + 15) // 16 * 16
    B = 255.0 * np.abs(weights_f64(weights_vn)).sum(axis=1)
    e = np.maximum(9, np.ceil(np.log2(np.maximum(B, 1.0)))).astype(np.int64)
    return k_pad * np.ldexp(1.0, e - 24)


def exact_sums(oc, lf, hp, v0=0, v1=None, all_focus=False, map_plane=None, focus=0.0, rng=0.0, threads=1):
    """S [V, H, W, 3] float64 (zero outside [v0, v1), like the oracle's blends) and ε [V]."""
    S = oc.blend_f64(lf, hp.focused_offsets, hp.offsets, hp.weights, v0=v0, v1=v1, all_focus=all_focus, map_plane=map_plane, focus=focus,
                     rng=rng, threads=threads)
    return S, epsilon(hp.weights, lf.shape[0])


def interval(S, eps):
    """lo, hi (uint8, the shape of S): the bytes q admits for a sum within eps ([V] or a scalar) of S."""
    e = np.asarray(eps, np.float64)
    e = e.reshape(e.shape + (1,) * (S.ndim - e.ndim))
    return quantise(S - e), quantise(S + e)


def bounds(oc, lf, hp, v0=0, v1=None, all_focus=False, map_plane=None, focus=0.0, rng=0.0, threads=1):
    """lo, hi [V, H, W, 3] uint8: the admissible bytes of a TEN_WM render of views [v0, v1) (the arguments of oc.blend_ten)."""
    return interval(*exact_sums(oc, lf, hp, v0=v0, v1=v1, all_focus=all_focus, map_plane=map_plane, focus=focus, rng=rng, threads=threads))


def outside(got, lo, hi):
    """Number of colour bytes of got [..., 4] outside [lo, hi] [..., 3]; alpha must be 255 everywhere."""
    assert got.shape[:-1] == lo.shape[:-1] == hi.shape[:-1] and got.shape[-1] == 4, (got.shape, lo.shape)
    assert (got[..., 3] == 255).all(), "alpha is not 255"
    c = got[..., :3]
    return int(((c < lo) | (c > hi)).sum())


def report(got, S, eps):
    """Diagnostics only.  For every colour byte of got [V, H, W, 4] outside the interval of S [V, H, W, 3] and eps [V] (in C order): the
    smallest |δ| with q(S + δ) == got, as a multiple of that view's ε (bisection on the failing bytes only; q is monotone and takes
    every integer).  Just above 1: the accumulation bound is at stake.  Tens or more: a kernel."""
    eps = np.broadcast_to(np.asarray(eps, np.float64).reshape(-1, 1, 1, 1), S.shape)
    lo, hi = interval(S, eps[:, 0, 0, 0])
    c = got[..., :3]
    sel = (c < lo) | (c > hi)
    g, s, e = c[sel].astype(np.float64), S[sel], eps[sel]
    sign = np.where(g > quantise(s), 1.0, -1.0)
    a, b = np.zeros_like(s), np.abs(g - s) + 1.0       # q(s + sign·a) is on the wrong side of g, q(s + sign·b) has reached it
    for _ in range(64):
        m = 0.5 * (a + b)
        reached = sign * (quantise(s + sign * m).astype(np.float64) - g) >= 0
        a, b = np.where(reached, a, m), np.where(reached, m, b)
    return b / e


def ties(S):
    """Number of sums (below the saturation at 255) that lie exactly half-way between two fp16 values: where RN-even decides."""
    s = np.asarray(S, np.float64)
    s = s[(s > 0) & (s < 255.0)]
    e = np.maximum(np.floor(np.log2(s)), -14.0).astype(np.int64)
    r = np.ldexp(s, 10 - e)                             # exact: in units of the fp16 spacing at s
    return int((r - np.floor(r) == 0.5).sum())
