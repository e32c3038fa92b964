"""The area resize of lfi_download_quilt_scaled restated in numpy, from the definition in include/lfi.h — not from the span arithmetic of
csrc/area_span.h, which the kernel runs and tests/test_host_scaled_quilt.py checks on its own.

Along one axis of `src` source and `dst` output pixels both images lie on a grid of src·dst units; source pixel s is the constant p[s] on
[s·dst, (s+1)·dst), and output pixel o is the INTEGRAL of that step function over [o·src, (o+1)·src) — the same number as Σ_s overlap(o, s)·p[s].
The integral from 0 to u is  F(u) = dst·(p[0] + … + p[i−1]) + (u − i·dst)·p[i]  with i = u // dst, so one cumulative sum gives every output
pixel as F((o+1)·src) − F(o·src), in uint64 throughout.  `resize_dense` is the definition as written — the overlap lengths as a weight matrix of
Python ints — for the sizes where that is affordable; the CPU tests hold the two against each other."""
import numpy as np


def _axis_integrals(a: np.ndarray, dst: int, axis: int) -> np.ndarray:
    """uint64 array -> the same with `axis` resized from src to dst entries: Σ_s overlap(o, s)·a[s] (the weights of one output sum to src)"""
    a = np.moveaxis(a.astype(np.uint64), axis, -1)
    src = a.shape[-1]
    assert 1 <= dst <= src
    zero = np.zeros(a.shape[:-1] + (1,), np.uint64)
    before = np.concatenate([zero, np.cumsum(a, axis=-1, dtype=np.uint64)], axis=-1)   # before[i] = a[0] + … + a[i−1]
    padded = np.concatenate([a, zero], axis=-1)                                         # u = src·dst: i = src, nothing of a[src] is taken
    u = np.arange(dst + 1, dtype=np.uint64) * np.uint64(src)
    i, part = (u // np.uint64(dst)).astype(np.int64), u % np.uint64(dst)
    F = np.uint64(dst) * before[..., i] + part * padded[..., i]
    return np.moveaxis(F[..., 1:] - F[..., :-1], -1, axis)


def area_sums(rgb: np.ndarray, tile_w: int, tile_h: int) -> np.ndarray:
    """[H][W][C] u8 -> [tile_h][tile_w][C] u64: Σ_sy Σ_sx wy·wx·p[sy][sx]"""
    return _axis_integrals(_axis_integrals(rgb, tile_w, 1), tile_h, 0)


def resize(view: np.ndarray, tile_w: int, tile_h: int) -> np.ndarray:
    """[H][W][4] u8 -> [tile_h][tile_w][4] u8: per colour channel (Σ wy·wx·p + W·H // 2) // (W·H), alpha 255"""
    H, W = view.shape[:2]
    area = np.uint64(W * H)
    out = np.full((tile_h, tile_w, 4), 255, np.uint8)
    out[..., :3] = ((area_sums(view[..., :3], tile_w, tile_h) + area // np.uint64(2)) // area).astype(np.uint8)
    return out


def overlaps(src: int, dst: int) -> np.ndarray:
    """[dst][src] int64: the length of [o·src, (o+1)·src) ∩ [s·dst, (s+1)·dst)"""
    o = np.arange(dst, dtype=np.int64)[:, None]
    s = np.arange(src, dtype=np.int64)[None, :]
    return np.maximum(np.minimum((o + 1) * src, (s + 1) * dst) - np.maximum(o * src, s * dst), 0)


def resize_dense(view: np.ndarray, tile_w: int, tile_h: int) -> np.ndarray:
    """`resize` as the definition is written: weight matrices of overlap lengths, Python-int arithmetic (small images only)"""
    H, W = view.shape[:2]
    wy, wx = overlaps(H, tile_h).astype(object), overlaps(W, tile_w).astype(object)
    out = np.full((tile_h, tile_w, 4), 255, np.uint8)
    for ch in range(3):
        sums = wy.dot(view[..., ch].astype(object)).dot(wx.T)
        out[..., ch] = ((sums + (W * H) // 2) // (W * H)).astype(np.uint8)
    return out


def quilt(views: np.ndarray, tiles_x: int, tiles_y: int, tile_w: int, tile_h: int) -> np.ndarray:
    """the first tiles_x·tiles_y of views [V][H][W][4], each resized, left to right, top to bottom"""
    out = np.zeros((tiles_y * tile_h, tiles_x * tile_w, 4), np.uint8)
    for i in range(tiles_x * tiles_y):
        ty, tx = divmod(i, tiles_x)
        out[ty * tile_h:(ty + 1) * tile_h, tx * tile_w:(tx + 1) * tile_w] = resize(views[i], tile_w, tile_h)
    return out
