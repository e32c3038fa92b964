"""Renders and focus maps under poison (lfi_debug_poison): the helper every GPU test that asserts output bytes goes through.

The views, the planar layout's RGBA scratch copy, the focus maps and the focus-map workspace belong to the context and persist between
calls.  A test that renders again into a buffer that already holds correct bytes checks only what the new launch happened to write: a
launch that skips a tile, a row, a view or the whole kernel leaves the earlier bytes in place and the test passes.  So every render here
first fills what it writes (views + scratch) with a poison byte, and every focus map fills the maps and the workspace.

One poison byte can equal the right answer (flat images, constant maps), so the bytes alternate from call to call: two calls under
POISON[0] and POISON[1] leave no byte that could be unwritten and correct under both.  Where the expected output can be constant, call
twice (`twice`); that also walks both sweep directions of the kernels that alternate them.
"""
import numpy as np

import lfinterpolator_amd as L

RENDER = L.LFI_POISON_VIEWS | L.LFI_POISON_SCRATCH
FOCUS = L.LFI_POISON_MAPS | L.LFI_POISON_FOCUS_WORKSPACE
ALL = RENDER | FOCUS | L.LFI_POISON_DERIVED
POISON = (0xA5, 0x5A)   # no byte equals both
SENTINEL = 0xC3         # initial fill of host arrays the library writes into (render_stream, quilts)

_calls = [0]


def _byte(byte):
    if byte is None:
        byte = POISON[_calls[0] & 1]
        _calls[0] += 1
    return byte


def render(ctx, method, all_focus=False, v0=0, v1=None, byte=None):
    """Poison the views and the scratch copy, render, synchronise.  Returns the poison byte."""
    b = _byte(byte)
    ctx.poison(RENDER, b)
    ctx.render(method, all_focus=all_focus, v0=v0, v1=v1)
    ctx.sync()
    return b


def focus_map(ctx, byte=None):
    """Poison both maps and the estimate's workspace, build the focus map, synchronise.  Returns the poison byte."""
    b = _byte(byte)
    ctx.poison(FOCUS, b)
    ctx.focus_map()
    ctx.sync()
    return b


def twice(fn):
    """Run fn(byte) under both poison bytes (and so both sweep directions of consecutive launches)."""
    for b in POISON:
        fn(b)


def untouched_view(ctx, byte):
    """What lfi_download_view returns for a view no launch wrote since the poison: every byte the poison in the RGBA layout; in the
    planar layout the colour planes hold it and the download re-creates alpha = 255.  Rows outside a row window stay zero."""
    out = np.zeros((ctx.height, ctx.width, 4), np.uint8)
    y0, y1 = ctx.out_rows
    out[y0:y1] = byte
    if ctx.view_layout().layout == L.LFI_LAYOUT_PLANAR_RGB:
        out[y0:y1, :, 3] = 255
    return out


def written_outside(ctx, v0, v1, byte, views=None):
    """Views outside [v0, v1) (all of them, or those listed in `views`) that no longer hold the poison — lfi_render's contract is that a
    launch writes views [v0, v1) only."""
    want = untouched_view(ctx, byte)
    cand = [v for v in (range(ctx.views) if views is None else views) if (v < v0 or v >= v1) and 0 <= v < ctx.views]
    return [v for v in cand if not (ctx.download_view(v) == want).all()]


def render_range(ctx, method, v0, v1, all_focus=False, byte=None, outside=None, inspect=None):
    """Render views [v0, v1) under poison, assert that every other view (or those in `outside`) still holds the poison, and return
    the rendered views [v0, v1).  inspect(): called after the render, before anything is downloaded."""
    b = render(ctx, method, all_focus=all_focus, v0=v0, v1=v1, byte=byte)
    if inspect:
        inspect()
    bad = written_outside(ctx, v0, v1, b, outside)
    assert not bad, (method, "views outside the range were written", v0, v1, bad[:8])
    return ctx.download_views(v0, v1)


def mismatch(got, want, tol=0):
    """Number of bytes of `got` further than `tol` from `want`."""
    return int((np.abs(got.astype(np.int32) - want.astype(np.int32)) > tol).sum())


def sentinel(shape):
    """A host array for the library to write into, filled with SENTINEL instead of zeros."""
    return np.full(shape, SENTINEL, np.uint8)
