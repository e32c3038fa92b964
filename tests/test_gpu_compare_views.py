"""GPU (-m gpu): batch view comparison — lfi_keep_views / lfi_compare_views (csrc/hip/quality_batch.hpp).

Every record is held against the numpy restatement of the definitions (tests/quality_ref.py, anchored by tests/test_host_compare_views.py) applied to
the views' own downloads: the integer fields and the MSE exactly (the MSE is one division of exact integers), SSIM to rtol 1e-9 and PSNR to 1e-9 dB —
the tolerances tests/test_gpu_plumbing.py::test_compare_view_psnr_ssim uses for the same expressions.  lfi_compare_view runs the same code for one view:
its result is held against the batch call's byte for byte."""
import ctypes
import math

import numpy as np
import pytest

import lfinterpolator_amd as L
import poison
from lfinterpolator_amd.abi import Quality
import quality_ref as ref

pytestmark = pytest.mark.gpu

COLS = ROWS = 4
V = 5
SHAPES = [(150, 61), (64, 32), (7, 40), (40, 7), (258, 130)]


def _light_field(w, h, seed=11):
    rng = np.random.default_rng(seed + w * 1000 + h)
    lf = rng.integers(0, 256, (COLS * ROWS, h, w, 4), dtype=np.uint8)
    lf[..., :3] = (lf[..., :3].astype(np.int32) // 3 + np.arange(w)[None, None, :, None] // 2).clip(0, 255).astype(np.uint8)   # some structure
    lf[..., 3] = 255
    return lf


def _params(gpu, w, h, focus=0.2, views=V):
    return gpu.build_params(COLS, ROWS, w, h, "0,0,1,1", focus, 0.0, 3.0, 1.5, views)


def _ctx(gpu, w, h, layout, lf=None, views=V):
    ctx = gpu.Context(0)
    ctx.set_grid(COLS, ROWS, w, h)
    ctx.upload_grid(_light_field(w, h) if lf is None else lf)
    ctx.set_params(_params(gpu, w, h, views=views))
    ctx.set_output_layout(layout)
    return ctx


def _padded(images, rng):
    """the images as [n][H][W][4] inside a larger array of random bytes: padded pitch and image stride, random alpha"""
    n, h, w = images.shape[:3]
    big = rng.integers(0, 256, (n + 1, h + 3, w + 5, 4), dtype=np.uint8)
    big[:n, :h, :w, :3] = images[..., :3]
    refs = big[:n, :h, :w]
    assert refs.strides == ((h + 3) * (w + 5) * 4, (w + 5) * 4, 4, 1)
    return refs


def _same(x, y, tol, relative):
    if math.isinf(x) or math.isinf(y):
        return x == y
    return abs(x - y) <= (tol * abs(y) if relative else tol)


def _check_quality(q, want, where):
    for c in range(3):
        assert q.mse[c] == want["mse"][c], (where, "mse", c, q.mse[c], want["mse"][c])
        assert _same(q.ssim[c], want["ssim"][c], 1e-9, True), (where, "ssim", c, q.ssim[c], want["ssim"][c])
        assert _same(q.psnr[c], want["psnr"][c], 1e-9, False), (where, "psnr", c, q.psnr[c], want["psnr"][c])
    assert _same(q.ssim_all, want["ssim_all"], 1e-9, True), (where, "ssim_all", q.ssim_all, want["ssim_all"])
    assert _same(q.psnr_all, want["psnr_all"], 1e-9, False), (where, "psnr_all", q.psnr_all, want["psnr_all"])


def _check(recs, agg, views, refs, where):
    """recs[k] / agg of compare_views against the restatement on views[k], refs[k]"""
    want = [ref.compare(views[k], refs[k]) for k in range(len(views))]
    for k, w in enumerate(want):
        r = recs[k]
        print(where, k, "psnr", r.q.psnr_all, w["psnr_all"], "ssim", r.q.ssim_all, w["ssim_all"], "sq_err", list(r.sq_err), w["sq_err"], "differing",
              r.differing_bytes, w["differing_bytes"], "windows", r.windows, w["windows"], "maxdiff", r.max_abs_diff, w["max_abs_diff"])
        assert list(r.sq_err) == w["sq_err"], (where, k, list(r.sq_err), w["sq_err"])
        assert (r.differing_bytes, r.windows, r.max_abs_diff) == (w["differing_bytes"], w["windows"], w["max_abs_diff"]), (where, k)
        _check_quality(r.q, w, (where, k))
    h, wd = views[0].shape[:2]
    _check_quality(agg, ref.aggregate(want, wd, h), (where, "all"))
    return want


def _bytes(recs, n):
    return ctypes.string_at(recs, ctypes.sizeof(L.ViewQuality) * n)


@pytest.mark.parametrize("layout", ["rgba", "planar"])
@pytest.mark.parametrize("w,h", SHAPES)
def test_compare_views_equals_the_restatement(w, h, layout, gpu):
    rng = np.random.default_rng(w + h)
    lf = _light_field(w, h)
    ctx = _ctx(gpu, w, h, layout, lf)
    poison.render(ctx, "STD")
    ctx.keep_views()
    std = ctx.download_views()
    poison.render(ctx, "TEN_WM")
    ten = ctx.download_views()
    assert ctx.memory_info().workspace_bytes >= V * ctx.view_layout().view_stride_bytes      # the kept views are counted

    # kept references: STD kept, TEN_WM compared — all views, then a range that starts after view 0
    recs, agg = ctx.compare_views()
    _check(recs, agg, ten, std, (w, h, layout, "kept"))
    first = _bytes(recs, V)
    recs, agg = ctx.compare_views(v0=1, n=3)
    _check(recs, agg, ten[1:4], std[1:4], (w, h, layout, "kept 1..3"))
    assert _bytes(recs, 3) == first[ctypes.sizeof(L.ViewQuality):4 * ctypes.sizeof(L.ViewQuality)]

    # two successive calls: the same bytes; and again with the scratch buffers poisoned in between
    recs, agg2 = ctx.compare_views()
    assert _bytes(recs, V) == first and bytes(agg2) == bytes(ctx.compare_views()[1])
    for _ in range(2):
        ctx.poison(L.LFI_POISON_SCRATCH, poison._byte(None))
        assert _bytes(ctx.compare_views()[0], V) == first

    # host references, padded pitch and stride, random alpha: the STD view, an unrelated image, the view itself — against views 1, 2, 3
    refs = _padded(np.stack([std[1], lf[3], ten[3]]), rng)
    recs, agg = ctx.compare_views(refs, v0=1)
    want = _check(recs, agg, ten[1:4], refs, (w, h, layout, "host"))
    host_first = _bytes(recs, 3)
    assert want[1]["max_abs_diff"] > 1
    assert recs[2].q.psnr_all == math.inf and list(recs[2].q.psnr) == [math.inf] * 3 and recs[2].differing_bytes == 0 and recs[2].max_abs_diff == 0
    assert list(recs[2].sq_err) == [0, 0, 0] and abs(recs[2].q.ssim_all - 1.0) < 1e-12
    if w < 8 or h < 8:
        assert all(r.windows == 0 and list(r.q.ssim) == [1.0, 1.0, 1.0] and r.q.ssim_all == 1.0 for r in recs)
    ctx.poison(L.LFI_POISON_SCRATCH, poison._byte(None))
    assert _bytes(ctx.compare_views(refs, v0=1)[0], 3) == host_first
    # the same numbers whether the STD view is the kept one or comes from the host
    assert _bytes(ctx.compare_views(v0=1, n=1)[0], 1) == host_first[:ctypes.sizeof(L.ViewQuality)]

    # each view's q against lfi_compare_view of the same view and reference: the same code, the same bytes
    for k in range(3):
        one = ctx.compare_view(1 + k, np.ascontiguousarray(refs[k]))
        assert bytes(one) == bytes(recs[k].q), (w, h, layout, k)
        if layout == "planar":
            # … and again with the scratch buffers poisoned between two calls
            ctx.poison(L.LFI_POISON_SCRATCH, poison._byte(None))
            assert bytes(ctx.compare_view(1 + k, np.ascontiguousarray(refs[k]))) == bytes(one), (w, h, k, "poisoned")

    # the call wrote no view and no kept view
    assert (ctx.download_views() == ten).all()
    assert _bytes(ctx.compare_views()[0], V) == first
    ctx.close()


@pytest.mark.parametrize("layout", ["rgba", "planar"])
def test_pinned_and_strided_host_references(layout, gpu):
    """40 views against 40 page-locked host references whose rows follow each other (one 2-D copy per chunk) and against the same images at a
    stride that is not pitch · H (one copy per image)"""
    w, h, views = 64, 32, 40
    ctx = _ctx(gpu, w, h, layout, views=views)
    poison.render(ctx, "TEN_WM")
    ten = ctx.download_views()
    rng = np.random.default_rng(3)
    noisy = (ten.astype(np.int32) + rng.integers(-2, 3, ten.shape)).clip(0, 255).astype(np.uint8)
    pinned = ctx.pinned_empty((views, h, w, 4))
    pinned[:] = noisy
    recs, agg = ctx.compare_views(pinned)
    _check(recs, agg, ten, noisy, (layout, "pinned"))
    dense = _bytes(recs, views)
    assert _bytes(ctx.compare_views(_padded(noisy, rng))[0], views) == dense
    ctx.close()


@pytest.mark.parametrize("layout", ["rgba", "planar"])
def test_a_render_leaves_the_kept_views_alone(layout, gpu):
    w, h = 150, 61
    ctx = _ctx(gpu, w, h, layout)
    poison.render(ctx, "STD")
    std = ctx.download_views()
    ctx.keep_views(1, 3)                                  # views 1, 2, 3
    ctx.set_params(_params(gpu, w, h, focus=0.35))        # as many views: the kept set stays
    poison.render(ctx, "TEN_WM")
    ten = ctx.download_views()
    assert (ten != std).any()
    recs, agg = ctx.compare_views(v0=1, n=3)
    _check(recs, agg, ten[1:4], std[1:4], (layout, "kept, other focus"))
    recs, agg = ctx.compare_views(v0=2, n=1)
    _check(recs, agg, ten[2:3], std[2:3], (layout, "kept, one view"))
    # keeping again replaces the set
    ctx.keep_views()
    recs, agg = ctx.compare_views()
    assert all(r.differing_bytes == 0 and r.q.psnr_all == math.inf for r in recs) and agg.psnr_all == math.inf
    ctx.close()


def test_refusals_leave_a_usable_context(gpu):
    w, h = 64, 32
    ctx = _ctx(gpu, w, h, "rgba")
    lib, handle = ctx._lib, ctx._h
    out = (L.ViewQuality * V)()
    refs = np.zeros((V, h, w, 4), np.uint8)
    raw = lambda v0, n, p, pitch, stride, o=out: lib.lfi_compare_views(handle, v0, n, p, pitch, stride, o, None)
    ptr = refs.ctypes.data_as(ctypes.c_void_p)
    # nothing rendered yet: no parameters, no views
    fresh = gpu.Context(0)
    assert lib.lfi_compare_views(fresh._h, 0, 1, ptr, w * 4, w * h * 4, out, None) == -1 and b"nothing rendered" in lib.lfi_last_error(fresh._h)
    with pytest.raises(gpu.LfiError, match="nothing rendered"):
        fresh.keep_views(0, 1)
    fresh.set_grid(COLS, ROWS, w, h)         # a grid, no parameters and no views yet
    with pytest.raises(gpu.LfiError, match="nothing rendered"):
        fresh.compare_views(refs)
    fresh.close()

    poison.render(ctx, "STD")
    std = ctx.download_views()

    def valid():
        recs, agg = ctx.compare_views(std)
        assert all(r.differing_bytes == 0 and r.q.psnr_all == math.inf for r in recs) and agg.psnr_all == math.inf

    valid()
    refused = [
        ("v0 < 0", lambda: raw(-1, 2, ptr, w * 4, w * h * 4)),
        ("n == 0", lambda: raw(0, 0, ptr, w * 4, w * h * 4)),
        ("n < 0", lambda: raw(0, -1, ptr, w * 4, w * h * 4)),
        ("past the views", lambda: raw(2, V - 1, ptr, w * 4, w * h * 4)),
        ("pitch too small", lambda: raw(0, V, ptr, w * 4 - 1, w * h * 4)),
        ("stride too small", lambda: raw(0, V, ptr, w * 4, w * h * 4 - 1)),
        ("stride below pitch * H", lambda: raw(0, 1, ptr, w * 4 + 16, w * h * 4)),
        ("out NULL", lambda: raw(0, V, ptr, w * 4, w * h * 4, None)),
        ("no kept set", lambda: raw(0, V, None, 0, 0)),
        ("keep past the views", lambda: lib.lfi_keep_views(handle, 3, V)),
        ("keep v0 < 0", lambda: lib.lfi_keep_views(handle, -1, 2)),
        ("keep n < 0", lambda: lib.lfi_keep_views(handle, 0, -2)),
    ]
    for what, call in refused:
        assert call() == -1, what
        assert lib.lfi_last_error(handle), what
        valid()
    # a kept set that does not cover the range
    ctx.keep_views(1, 3)
    for v0, n in ((0, 2), (3, 2), (0, V)):
        assert raw(v0, n, None, 0, 0) == -1, (v0, n)
        valid()
    assert raw(1, 3, None, 0, 0) == 0
    # one kept in another layout: dropped with the layout
    ctx.set_output_layout("planar")
    poison.render(ctx, "STD")
    assert raw(1, 3, None, 0, 0) == -1
    valid()
    ctx.keep_views(1, 3)
    assert raw(1, 3, None, 0, 0) == 0
    # … dropped by another number of views, by drop_kept_views, and by a new grid
    ctx.set_params(_params(gpu, w, h, views=V + 1))
    poison.render(ctx, "STD")
    assert raw(1, 3, None, 0, 0) == -1
    ctx.keep_views()
    assert lib.lfi_compare_views(handle, 0, V + 1, None, 0, 0, (L.ViewQuality * (V + 1))(), None) == 0
    ctx.drop_kept_views()
    assert raw(0, 1, None, 0, 0) == -1
    kept_before = ctx.memory_info().workspace_bytes
    ctx.keep_views()
    assert ctx.memory_info().workspace_bytes == kept_before + (V + 1) * ctx.view_layout().view_stride_bytes
    ctx.set_grid(COLS, ROWS, w, h)
    ctx.upload_grid(_light_field(w, h))
    ctx.set_params(_params(gpu, w, h))
    poison.render(ctx, "STD")
    assert raw(0, 1, None, 0, 0) == -1
    valid()
    ctx.close()
    # a row window
    hp = _params(gpu, w, h)
    win = gpu.Context(0)
    win.set_grid(COLS, ROWS, w, h)
    band = (8, 24)
    in_rows = gpu.input_rows(band, hp.focused_offsets, h)
    win.set_row_window(band[0], band[1], in_rows[0], in_rows[1])
    win.upload_grid(_light_field(w, h))
    win.set_params(hp)
    poison.render(win, "STD")
    with pytest.raises(gpu.LfiError, match="row window"):
        win.compare_views(refs)
    assert (win.download_view(0)[band[0]:band[1]] == std[0][band[0]:band[1]]).all()      # … and the context goes on
    win.close()


def test_compare_view_refusals(gpu):
    """lfi_compare_view's own checks, in its own words: nothing rendered, a bad index, a NULL reference, a short pitch, a row window — each
    leaves out untouched and the context usable"""
    w, h = 64, 32
    ctx = _ctx(gpu, w, h, "planar")
    lib, handle = ctx._lib, ctx._h
    ref_img = np.zeros((h, w, 4), np.uint8)
    ptr = ref_img.ctypes.data_as(ctypes.c_void_p)
    out = Quality()
    before = bytes(out)
    assert lib.lfi_compare_view(handle, 0, ptr, w * 4, None) == -1
    # nothing rendered yet: no grid; a grid but no parameters
    fresh = gpu.Context(0)
    assert lib.lfi_compare_view(fresh._h, 0, ptr, w * 4, ctypes.byref(out)) == -1 and lib.lfi_last_error(fresh._h) == b"nothing rendered yet"
    fresh.set_grid(COLS, ROWS, w, h)
    with pytest.raises(gpu.LfiError, match=": nothing rendered yet$"):
        fresh.compare_view(0, ref_img)
    fresh.close()

    poison.render(ctx, "STD")
    std = ctx.download_views()
    for what, args in (("v < 0", (-1, ptr, w * 4)), ("v == views", (V, ptr, w * 4)), ("NULL reference", (0, None, w * 4)),
                       ("short pitch", (0, ptr, w * 4 - 1))):
        assert lib.lfi_compare_view(handle, *args, ctypes.byref(out)) == -1, what
        assert lib.lfi_last_error(handle) == b"bad view index, pointer or pitch", what
        assert bytes(out) == before, what
        assert ctx.compare_view(2, std[2]).psnr_all == math.inf, what
    ctx.close()
    # a row window
    hp = _params(gpu, w, h)
    win = gpu.Context(0)
    win.set_grid(COLS, ROWS, w, h)
    band = (8, 24)
    in_rows = gpu.input_rows(band, hp.focused_offsets, h)
    win.set_row_window(band[0], band[1], in_rows[0], in_rows[1])
    win.upload_grid(_light_field(w, h))
    win.set_params(hp)
    win.set_output_layout("planar")
    poison.render(win, "STD")
    with pytest.raises(gpu.LfiError, match=r": lfi_compare_view needs the whole view \(no row window\)$"):
        win.compare_view(0, ref_img)
    assert lib.lfi_compare_view(win._h, V, ptr, w * 4, ctypes.byref(out)) == -1      # the index is looked at before the window
    assert lib.lfi_last_error(win._h) == b"bad view index, pointer or pitch" and bytes(out) == before
    assert (win.download_view(0)[band[0]:band[1]] == std[0][band[0]:band[1]]).all()      # … and the context goes on
    win.close()


def test_compare_on_a_callers_stream(gpu):
    """ordered after the work on the stream in use: a render enqueued on a caller's stream, compared without a synchronisation in between"""
    import torch
    w, h = 258, 130
    ctx = _ctx(gpu, w, h, "planar")
    poison.render(ctx, "STD")
    std = ctx.download_views()
    ctx.keep_views()
    stream = torch.cuda.Stream(device="cuda:0")
    ctx.set_stream(stream.cuda_stream)
    ctx.poison(poison.RENDER, poison._byte(None))
    ctx.render("TEN_WM")
    recs, agg = ctx.compare_views()          # no sync: the call orders itself
    ten = ctx.download_views()
    _check(recs, agg, ten, std, "caller's stream")
    ctx.set_stream(None)
    ctx.close()


def test_full_size_ten_wm_against_kept_std(gpu):
    """8 × 8 grid at 1080p, 64 views: TEN_WM against the kept STD views of the same parameters — the project's numerics contract read off the
    device — against the restatement on the downloaded views"""
    cols = rows = 8
    w, h, views = 1920, 1080, 64
    hp = gpu.build_params(cols, rows, w, h, "0,0,1,1", 0.1, 0.0, 3.0, 1.0, views)
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, w, h)
    ctx.fill_synthetic(0x1F1F)
    ctx.set_params(hp)
    ctx.set_output_layout("planar")
    poison.render(ctx, "STD")
    ctx.keep_views()
    std = ctx.download_views()
    poison.render(ctx, "TEN_WM")
    ten = ctx.download_views()
    ctx.poison(L.LFI_POISON_SCRATCH, poison._byte(None))
    recs, agg = ctx.compare_views()
    _check(recs, agg, ten, std, "full size")
    assert max(r.max_abs_diff for r in recs) <= 1                      # the TEN_WM contract: within one LSB of STD
    # … and against pinned host references: the same records
    pinned = ctx.pinned_empty((views, h, w, 4))
    pinned[:] = std
    assert _bytes(ctx.compare_views(pinned)[0], views) == _bytes(recs, views)
    ctx.close()
