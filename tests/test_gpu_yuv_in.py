"""GPU (-m gpu): YUV 4:2:0 input — lfi_upload_images_yuv420 (csrc/hip/yuv420_upload.hpp).

The conversion is defined in integers (include/lfi.h), so every comparison is `==` on all bytes: the grid's bytes after the call against
the numpy restatement (tests/yuv_in_ref.py, held against the definition by tests/test_host_yuv_in.py) of the frames that went in.  The grid
is a torch tensor attached with lfi_attach_grid and pre-filled with a pattern, read back with a device-to-host copy of the tensor; the
context's scratch buffers — the staged frames among them — are poisoned before the checked calls."""
import ctypes as C

import numpy as np
import pytest

import lfinterpolator_amd as L
import poison
import yuv_in_ref as ref
from conftest import SEED, SMALL_CASES

pytestmark = pytest.mark.gpu

PATTERN = 0x3C   # what the attached grid holds before a call
# (cols, rows, W, H): what each shape can break
ONE_BLOCK = (1, 1, 8, 2)        # one block, every chroma neighbour clamped
TIGHT = (3, 3, 16, 16)          # W a multiple of 8, H even: the staged frames are the host frames, one copy for the chunk
ODD = (4, 4, 33, 17)            # odd W and H: padded staging planes (three 2D copies per frame), the pixel-by-pixel stores, exactly one chunk of 16
WIDE = (1, 2, 520, 6)           # 65 blocks per row: chroma neighbours cross a workgroup's boundary (64 lanes x 8 columns)
CHUNKS = (5, 5, 24, 10)         # 25 frames: chunks of 16 + 9
ALL_FORMATS = [(m, r, c) for m, r in ref.FORMATS for c in (ref.BILINEAR, ref.NEAREST)]
CASES = [(s, f) for s in (ODD, WIDE) for f in ALL_FORMATS] + [(ONE_BLOCK, ALL_FORMATS[0]), (ONE_BLOCK, ALL_FORMATS[7]), (TIGHT, ALL_FORMATS[2]),
                                                              (CHUNKS, ALL_FORMATS[5])]


def _frames(shape, seed=0):
    """uniformly random bytes in all three planes — codes outside the nominal ranges hit both clamps — and, as the last frame, blocks of
    Y in {0, 16, 235, 255} x U, V in {0, 16, 128, 240, 255}"""
    cols, rows, w, h = shape
    n = cols * rows
    frames = np.random.default_rng(seed + w * 1000 + h).integers(0, 256, (n, ref.sizes(w, h)[2]), dtype=np.uint8)
    frames[-1] = ref.extremes_frame(w, h)
    return frames


def _attached(gpu, shape, window=None):
    """a context whose grid is a torch tensor holding PATTERN"""
    import torch
    cols, rows, w, h = shape
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, w, h)
    held = h
    if window:
        ctx.set_row_window(*window)
        held = window[3] - window[2]
    grid = torch.full((cols * rows, held, w, 4), PATTERN, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.attach_grid(grid.data_ptr(), grid.numel())
    return ctx, grid


def _read(ctx, grid):
    import torch
    ctx.upload_wait()
    ctx.sync()
    torch.cuda.synchronize()
    return grid.cpu().numpy()


@pytest.mark.parametrize("shape,fmt", CASES, ids=lambda v: "x".join(map(str, v)))
def test_grid_equals_the_restatement(shape, fmt, gpu):
    cols, rows, w, h = shape
    frames = _frames(shape)
    want = ref.images(frames, w, h, *fmt)
    assert want[..., :3].min() == 0 and want[..., :3].max() == 255   # both clamps are reached
    ctx, grid = _attached(gpu, shape)
    import torch
    got = []
    for byte in (0x00, 0xFF):   # the staged frames' padding differs between the two calls: no byte of it may reach the result
        grid.fill_(PATTERN)
        torch.cuda.synchronize()   # torch's stream and the context's know nothing of each other
        ctx.poison(L.LFI_POISON_SCRATCH, byte)
        ctx.upload_images_yuv420(frames, matrix=fmt[0], range=fmt[1], chroma=fmt[2])
        got.append(_read(ctx, grid))
        assert (got[-1] == want).all(), (shape, fmt, byte, int((got[-1] != want).sum()))
    assert (got[0][..., 3] == 255).all()
    ctx.close()
    del grid


def test_range_of_images_stride_and_pageable_or_pinned_frames(gpu):
    """g0 = 3, n = 20 of the 25 images, frames a gap apart (one copy per frame), from page-locked memory: the other images keep the pattern"""
    cols, rows, w, h = CHUNKS
    fb = ref.sizes(w, h)[2]
    frames = _frames(CHUNKS, seed=1)[:20]
    ctx, grid = _attached(gpu, CHUNKS)
    host = ctx.pinned_empty((20, fb + 13))
    host[...] = poison.SENTINEL
    host[:, :fb] = frames
    fmt = (ref.BT601, ref.LIMITED, ref.BILINEAR)
    want = ref.images(frames, w, h, *fmt)
    ctx.poison(L.LFI_POISON_SCRATCH, 0xA5)
    ctx.upload_images_yuv420(host, g0=3, matrix=fmt[0], range=fmt[1], chroma=fmt[2])
    got = _read(ctx, grid)
    assert (got[3:23] == want).all(), int((got[3:23] != want).sum())
    assert (got[:3] == PATTERN).all() and (got[23:] == PATTERN).all()
    assert (host[:, fb:] == poison.SENTINEL).all() and (host[:, :fb] == frames).all()
    # a padded shape with a gap, one image in the middle
    ctx.close()
    del grid
    cols, rows, w, h = ODD
    fb = ref.sizes(w, h)[2]
    frames = _frames(ODD, seed=2)
    gapped = np.full((3, fb + 7), poison.SENTINEL, np.uint8)
    gapped[:, :fb] = frames[:3]
    ctx, grid = _attached(gpu, ODD)
    ctx.upload_images_yuv420(gapped, g0=5, matrix="709", range="full", chroma="nearest")
    got = _read(ctx, grid)
    assert (got[5:8] == ref.images(frames[:3], w, h, ref.BT709, ref.FULL, ref.NEAREST)).all()
    assert (got[:5] == PATTERN).all() and (got[8:] == PATTERN).all()
    ctx.close()
    del grid


@pytest.mark.parametrize("size", [(21, 11), (24, 6)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_grid_equals_that_of_the_surface_call(size, gpu):
    """lfi_upload_images_yuv420 is lfi_upload_images_yuv from the equivalent descriptor — host memory, I420, tight planes, the array's frame
    stride: 3 frames 5 bytes apart into images 1 … 3 of 4 (21x11 padded staged planes, 24x6 the staged frame is the host frame), the
    whole grid byte for byte; the 5 bytes between the frames keep their poison"""
    import torch
    w, h = size
    shape = (2, 2, w, h)
    fb = ref.sizes(w, h)[2]
    frames = _frames(shape, seed=6)[:3]
    host = np.full((3, fb + 5), poison.SENTINEL, np.uint8)
    host[:, :fb] = frames
    fmt = (ref.BT601, ref.FULL, ref.BILINEAR)
    ctx, grid = _attached(gpu, shape)
    ctx.poison(L.LFI_POISON_SCRATCH, 0xA5)
    ctx.upload_images_yuv420(host, g0=1, matrix=fmt[0], range=fmt[1], chroma=fmt[2])
    first = _read(ctx, grid)
    grid.fill_(PATTERN)
    torch.cuda.synchronize()
    surfaces = ctx.yuv_surfaces_packed("i420", "host", host.ctypes.data, keep=host)
    surfaces.frame_stride = host.strides[0]
    ctx.poison(L.LFI_POISON_SCRATCH, 0x5A)
    ctx.upload_images_yuv(surfaces, 3, g0=1, matrix=fmt[0], range=fmt[1], chroma=fmt[2])
    second = _read(ctx, grid)
    assert (first == second).all(), int((first != second).sum())
    assert (first[1:] == ref.images(frames, w, h, *fmt)).all() and (first[0] == PATTERN).all()
    assert (host[:, fb:] == poison.SENTINEL).all() and (host[:, :fb] == frames).all()
    ctx.close()
    del grid


def test_the_staging_buffer_is_counted_and_kept(gpu):
    cols, rows, w, h = CHUNKS
    frames = _frames(CHUNKS)
    ctx, grid = _attached(gpu, CHUNKS)
    before = ctx.memory_info().workspace_bytes
    ctx.upload_images_yuv420(frames[:2])
    padded = 24 * 10 + 2 * 12 * 5
    assert ctx.memory_info().workspace_bytes == before + 2 * padded
    ctx.upload_images_yuv420(frames)            # 25 frames: a chunk is at most 16
    ctx.upload_images_yuv420(frames[:1])
    assert ctx.memory_info().workspace_bytes == before + 16 * padded
    assert (_read(ctx, grid)[1:] == ref.images(frames[1:], w, h, ref.BT709, ref.LIMITED)).all()
    ctx.close()
    del grid


# ---- renders from uploaded frames -------------------------------------------------------------------------------------------------------------

def test_renders_equal_those_of_the_restatements_rgba(gpu):
    """own planes, default routing, the g3x3_16x16_v8 golden's grid and parameters: views from YUV uploads equal, byte for byte, those of a
    context given the restatement's RGBA through lfi_upload_image — also after a second upload (a derived copy that was not invalidated
    would show), and a YUV upload issued right behind a render, without a sync, leaves that render's views what they were"""
    name, cols, rows, w, h, views, trajectory, focus, aspect, effect = SMALL_CASES[0]
    assert name == "g3x3_16x16_v8"
    hp = gpu.build_params(cols, rows, w, h, trajectory, focus, 0.0, effect, aspect, views)
    shape = (cols, rows, w, h)
    fmt = (ref.BT709, ref.LIMITED, ref.BILINEAR)
    first, second = _frames(shape, seed=3), _frames(shape, seed=4)
    yuv, rgba = gpu.Context(0), gpu.Context(0)
    for ctx in (yuv, rgba):
        ctx.set_grid(cols, rows, w, h)
        ctx.fill_synthetic(SEED)
        ctx.set_params(hp)
    want = {}
    for step, frames in enumerate((first, second)):
        yuv.upload_images_yuv420(frames, matrix=fmt[0], range=fmt[1], chroma=fmt[2])
        rgba.upload_grid(ref.images(frames, w, h, *fmt))
        for method in ("STD", "TEN_WM"):
            poison.render(yuv, method)
            poison.render(rgba, method)
            want[(step, method)] = rgba.download_views()
            got = yuv.download_views()
            assert (got == want[(step, method)]).all(), (step, method, poison.mismatch(got, want[(step, method)]))
    assert not (want[(0, "STD")] == want[(1, "STD")]).all()
    # the grid holds `second`; a render, and the upload of `first` behind it with no sync in between
    for method in ("STD", "TEN_WM"):
        yuv.upload_images_yuv420(second, matrix=fmt[0], range=fmt[1], chroma=fmt[2])
        yuv.poison(poison.RENDER, 0xA5)
        yuv.render(method)
        yuv.upload_images_yuv420(first, matrix=fmt[0], range=fmt[1], chroma=fmt[2])
        yuv.sync()
        assert (yuv.download_views() == want[(1, method)]).all(), method
        poison.render(yuv, method)
        assert (yuv.download_views() == want[(0, method)]).all(), method
    yuv.close()
    rgba.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------

def _raw(ctx, g0, n, matrix, rng, chroma, frames, stride):
    return ctx._lib.lfi_upload_images_yuv420(ctx._h, g0, n, matrix, rng, chroma, frames.ctypes.data_as(C.c_void_p) if frames is not None else None, stride)


def test_refusals_leave_the_grid_and_a_usable_context(gpu):
    cols, rows, w, h = ODD
    n = cols * rows
    fb = ref.sizes(w, h)[2]
    frames = _frames(ODD, seed=5)
    ctx, grid = _attached(gpu, ODD)
    before = ctx.memory_info().workspace_bytes
    refused = [
        ("n = 0", (0, 0, 0, 0, 0, frames, fb), "n >= 1"),
        ("n = -1", (0, -1, 0, 0, 0, frames, fb), "n >= 1"),
        ("g0 below 0", (-1, 2, 0, 0, 0, frames, fb), "inside"),
        ("g0 + n beyond the grid", (n - 1, 2, 0, 0, 0, frames, fb), "inside"),
        ("g0 = N", (n, 1, 0, 0, 0, frames, fb), "inside"),
        ("unknown matrix", (0, n, 2, 0, 0, frames, fb), "matrix"),
        ("negative matrix", (0, n, -1, 0, 0, frames, fb), "matrix"),
        ("unknown range", (0, n, 0, 2, 0, frames, fb), "range"),
        ("unknown chroma", (0, n, 0, 0, 2, frames, fb), "chroma"),
        ("negative chroma", (0, n, 0, 0, -1, frames, fb), "chroma"),
        ("frames NULL", (0, n, 0, 0, 0, None, fb), "NULL"),
        ("stride below the frame's bytes", (0, n, 0, 0, 0, frames, fb - 1), "frame_stride_bytes"),
        ("stride 0", (0, n, 0, 0, 0, frames, 0), "frame_stride_bytes"),
    ]
    for what, args, message in refused:
        assert _raw(ctx, *args) == -1, what                    # LFI_EINVAL
        assert message in ctx._lib.lfi_last_error(ctx._h).decode(), (what, ctx._lib.lfi_last_error(ctx._h).decode())
        assert (_read(ctx, grid) == PATTERN).all(), what
        assert ctx.memory_info().workspace_bytes == before, what   # the staging buffer was not touched
    ctx.upload_images_yuv420(frames)                              # … and the context goes on
    assert (_read(ctx, grid) == ref.images(frames, w, h, ref.BT709, ref.LIMITED)).all()
    ctx.close()
    del grid
    # no grid
    fresh = gpu.Context(0)
    assert _raw(fresh, 0, 1, 0, 0, 0, frames, fb) == -1 and "lfi_set_grid" in fresh._lib.lfi_last_error(fresh._h).decode()
    fresh.close()
    # a row window: a 2x2 block may straddle the band
    win, grid = _attached(gpu, ODD, window=(2, 9, 1, 12))
    assert _raw(win, 0, n, 0, 0, 0, frames, fb) == -1 and "row window" in win._lib.lfi_last_error(win._h).decode()
    assert (_read(win, grid) == PATTERN).all()
    win.close()
    del grid
    # released inputs
    hp = gpu.build_params(cols, rows, w, h, "0,0,1,1", 0.2, 0.0, 3.0, 1.0, 4)
    rel = gpu.Context(0)
    rel.set_grid(cols, rows, w, h)
    rel.fill_synthetic(SEED)
    rel.set_params(hp)
    poison.render(rel, "TEN_WM")
    views = rel.download_views()
    rel.release_inputs()
    assert _raw(rel, 0, n, 0, 0, 0, frames, fb) == -1 and "released" in rel._lib.lfi_last_error(rel._h).decode()
    poison.render(rel, "TEN_WM")
    assert (rel.download_views() == views).all()
    rel.close()


def test_one_frame_with_a_stride_below_the_frame_is_refused(gpu):
    """n = 1: no second frame starts a stride after the first, and a descriptor of surfaces says nothing about its stride then — the call
    refuses a frame_stride_bytes below the frame's bytes all the same, and the grid and the staging buffer stay untouched"""
    cols, rows, w, h = ODD
    fb = ref.sizes(w, h)[2]
    frames = _frames(ODD, seed=7)
    ctx, grid = _attached(gpu, ODD)
    before = ctx.memory_info().workspace_bytes
    assert _raw(ctx, 2, 1, 0, 0, 0, frames, fb - 1) == -1
    assert ctx._lib.lfi_last_error(ctx._h).decode() == ("lfi_upload_images_yuv420: the frames' pointer is NULL or frame_stride_bytes is below "
                                                        "W*H + 2*((W+1)/2)*((H+1)/2)")
    assert (_read(ctx, grid) == PATTERN).all() and ctx.memory_info().workspace_bytes == before
    assert _raw(ctx, 2, 1, 0, 0, 0, frames, fb) == 0
    got = _read(ctx, grid)
    assert (got[2] == ref.images(frames[:1], w, h, ref.BT709, ref.LIMITED)[0]).all() and (got[:2] == PATTERN).all() and (got[3:] == PATTERN).all()
    ctx.close()
    del grid
