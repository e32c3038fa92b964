"""GPU (-m gpu): YUV 4:2:0 video frames — lfi_download_views_yuv420 and lfi_render_stream_yuv420 (csrc/hip/yuv420.hpp).

The conversion is defined in integers (include/lfi.h), so every comparison is `==` on all bytes: the library's frames against the numpy
restatement (tests/yuv_ref.py, held against the definition by tests/test_host_yuv.py) applied to lfi_download_view's bytes of the same
views.  The context's scratch buffers — the device frames among them — are poisoned with 0xA5 before every checked call, and the host
frames are written into arrays pre-filled with poison.SENTINEL: bytes between the frames must stay untouched."""
import ctypes as C

import numpy as np
import pytest

import lfinterpolator_amd as L
import poison
import yuv_ref as ref
from conftest import SEED

pytestmark = pytest.mark.gpu

COLS = ROWS = 3
V = 5
# the kernel's constants (csrc/hip/yuv420.hpp): a lane owns YUV_BLOCK_W x 2 pixels, a workgroup is YUV_LANES_X lanes wide and YUV_BLOCK_ROWS
# block rows high.  One workgroup spans 64 * 8 = 512 columns and 4 * 2 = 8 rows
YUV_LANES_X, YUV_BLOCK_W, YUV_BLOCK_ROWS = 64, 8, 4
WIDE = YUV_LANES_X * YUV_BLOCK_W + 5   # 517: two workgroups per row, the second one lane wide and that lane's block ragged
# (W, H, bytes between the frames): 16x8 the aligned one-copy path; 24x6 with frame_stride_bytes > frame_bytes (one copy per frame); 17x9,
# 7x3, 1x1 ragged in both axes (three 2D copies per frame), the last two narrower than a lane's block; 17x9 is also two workgroups high
SHAPES = [(16, 8, 0), (24, 6, 11), (17, 9, 0), (7, 3, 3), (1, 1, 0), (WIDE, 5, 0)]
PAD = 0xA5


def _ctx(gpu, w, h, layout, views=V, focus_range=0.0):
    hp = gpu.build_params(COLS, ROWS, w, h, "0,0,1,1", 0.2, focus_range, 3.0, 1.0, views)
    ctx = gpu.Context(0)
    ctx.set_grid(COLS, ROWS, w, h)
    ctx.fill_synthetic(SEED)
    ctx.set_params(hp)
    ctx.set_output_layout(layout)
    return ctx, hp


def _frames(ctx, v0, n, fmt, gap=0):
    """the frames of views [v0, v0 + n) under poison, in a host array whose rows are `gap` bytes longer than a frame; asserts that the gap is
    untouched"""
    fb = ref.sizes(ctx.width, ctx.height)[2]
    assert ctx.yuv420_frame_bytes() == fb
    ctx.poison(L.LFI_POISON_SCRATCH, PAD)
    host = poison.sentinel((n, fb + gap))
    got = ctx.download_views_yuv420(v0, n, matrix=fmt[0], range=fmt[1], out=host)
    assert (host[:, fb:] == poison.SENTINEL).all(), "bytes between the frames were written"
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("layout", ["rgba", "planar"])
def test_frames_equal_the_restatement(layout, shape, gpu):
    w, h, gap = shape
    ctx, _ = _ctx(gpu, w, h, layout)
    for method in ("STD", "TEN_WM"):
        poison.render(ctx, method)
        views = ctx.download_views()
        assert (views[..., 3] == 255).all()
        for fmt in ref.FORMATS:
            want = ref.frames(views, *fmt)
            for v0, n in ((0, V), (1, 3), (V - 1, 1)):   # all views; sub-ranges v0 > 0, n < views
                got = _frames(ctx, v0, n, fmt, gap)
                assert got.shape == want[v0:v0 + n].shape and (got == want[v0:v0 + n]).all(), (layout, shape, method, fmt, v0, n,
                                                                                                  int((got != want[v0:v0 + n]).sum()))
        assert (ctx.download_views() == views).all()   # the call writes no view
    ctx.close()


def _attached(gpu, w, h, layout, content):
    """a context whose views are a torch buffer holding `content` ([n][h][w][4], alpha 255) in the layout's device form; planar padding
    bytes hold 0x77"""
    import torch
    n = content.shape[0]
    ctx, _ = _ctx(gpu, w, h, layout, views=n)
    vl = ctx.view_layout()
    if layout == "planar":
        pitch = vl.row_pitch_bytes
        assert vl.plane_stride_bytes == h * pitch and vl.view_stride_bytes == 3 * h * pitch
        dev = np.full((n, 3, h, pitch), 0x77, np.uint8)
        dev[:, :, :, :w] = content[..., :3].transpose(0, 3, 1, 2)
    else:
        assert vl.view_stride_bytes == w * h * 4
        dev = content
    buf = torch.from_numpy(np.ascontiguousarray(dev).reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    ctx.attach_views(buf.data_ptr(), buf.numel())
    return ctx, buf


@pytest.mark.parametrize("size", [(128, 66, 3), (21, 11, 2)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("layout", ["rgba", "planar"])
def test_attached_views_reach_the_extremes(layout, size, gpu):
    """views written directly into attached view memory: the 8 cube corners in every 2x2 arrangement (128x66x3: all 4096 of them,
    tests/test_host_yuv.py), uniform corners and greys — 16, 235, 240 and the 255 clamp"""
    w, h, n = size
    content = ref.corner_views(w, h, n)
    ctx, buf = _attached(gpu, w, h, layout, content)
    views = ctx.download_views()
    assert (views == content).all()
    for fmt in ref.FORMATS:
        want = ref.frames(views, *fmt)
        got = _frames(ctx, 0, n, fmt)
        assert (got == want).all(), (layout, size, fmt, int((got != want).sum()))
        if (w, h) == (128, 66):
            fb_y = w * h
            if fmt[1] == ref.LIMITED:
                assert (got[:, :fb_y].min(), got[:, :fb_y].max(), got[:, fb_y:].min(), got[:, fb_y:].max()) == (16, 235, 16, 240)
            else:
                assert (got[:, :fb_y].min(), got[:, :fb_y].max(), got[:, fb_y:].max()) == (0, 255, 255)
    ctx.close()
    del buf


def _raw_download(ctx, v0, n, matrix, rng, out, stride):
    return ctx._lib.lfi_download_views_yuv420(ctx._h, v0, n, matrix, rng, out.ctypes.data_as(C.c_void_p) if out is not None else None, stride)


def test_refusals_leave_a_usable_context(gpu):
    w, h = 17, 9
    ctx, hp = _ctx(gpu, w, h, "rgba")
    poison.render(ctx, "STD")
    views = ctx.download_views()
    fb = ref.sizes(w, h)[2]
    want = ref.frames(views, ref.BT601, ref.FULL)

    def valid():
        assert (_frames(ctx, 1, 3, (ref.BT601, ref.FULL), gap=2) == want[1:4]).all()

    valid()
    host = poison.sentinel((V, fb + 4))
    refused = [
        ("n = 0", (0, 0, 0, 0, host, fb + 4), "n >= 1"),
        ("n = -1", (0, -1, 0, 0, host, fb + 4), "n >= 1"),
        ("v0 below 0", (-1, 2, 0, 0, host, fb + 4), "inside"),
        ("v0 + n beyond the views", (3, 3, 0, 0, host, fb + 4), "inside"),
        ("v0 = views", (V, 1, 0, 0, host, fb + 4), "inside"),
        ("unknown matrix", (0, V, 2, 0, host, fb + 4), "matrix"),
        ("negative matrix", (0, V, -1, 0, host, fb + 4), "matrix"),
        ("unknown range", (0, V, 0, 2, host, fb + 4), "range"),
        ("out NULL", (0, V, 0, 0, None, fb + 4), "NULL"),
        ("stride below the frame's bytes", (0, V, 0, 0, host, fb - 1), "frame_stride_bytes"),
        ("stride 0", (0, V, 0, 0, host, 0), "frame_stride_bytes"),
    ]
    for what, args, message in refused:
        assert _raw_download(ctx, *args) == -1, what                    # LFI_EINVAL
        assert message in ctx._lib.lfi_last_error(ctx._h).decode(), (what, ctx._lib.lfi_last_error(ctx._h).decode())
        assert (host == poison.SENTINEL).all(), what
        valid()
    # the stream call refuses the same, and what lfi_render_stream refuses
    frames = poison.sentinel((7, fb))
    w16 = np.ascontiguousarray(np.tile(hp.weights, (2, 1))[:7])

    def raw_stream(weights=w16, total=7, matrix=0, rng=0, out=frames, stride=fb, method=L.LFI_METHOD_STD):
        return ctx._lib.lfi_render_stream_yuv420(ctx._h, method, 0, weights.ctypes.data_as(C.c_void_p) if weights is not None else None, total, matrix, rng,
                                                 out.ctypes.data_as(C.c_void_p) if out is not None else None, stride)

    for what, kw in [("unknown matrix", dict(matrix=3)), ("unknown range", dict(rng=-1)), ("host_out NULL", dict(out=None)), ("stride", dict(stride=fb - 1)),
                     ("weights NULL", dict(weights=None)), ("total_views 0", dict(total=0)), ("method", dict(method=7))]:
        assert raw_stream(**kw) == -1, what
        assert (frames == poison.SENTINEL).all(), what
        valid()
    ctx.set_view_offsets(np.zeros((V, COLS * ROWS, 2), np.int32))
    assert raw_stream() == -1 and "lfi_render_stream_yuv420" in ctx._lib.lfi_last_error(ctx._h).decode()
    ctx.set_view_offsets(None)
    assert (frames == poison.SENTINEL).all()
    assert (ctx.download_views() == views).all()
    valid()
    ctx.close()
    # a row window: a 2x2 block may straddle the band
    band = (2, 7)
    win = gpu.Context(0)
    win.set_grid(COLS, ROWS, w, h)
    in_rows = gpu.input_rows(band, hp.focused_offsets, h)
    win.set_row_window(band[0], band[1], in_rows[0], in_rows[1])
    win.fill_synthetic(SEED)
    win.set_params(hp)
    poison.render(win, "STD")
    with pytest.raises(gpu.LfiError, match="row window"):
        win.download_views_yuv420(out=host[:, :fb + 4])
    with pytest.raises(gpu.LfiError, match="row window"):
        win.render_stream_yuv420("STD", w16, out=frames)
    assert (host == poison.SENTINEL).all() and (frames == poison.SENTINEL).all()
    assert (win.download_view(0)[band[0]:band[1]] == views[0][band[0]:band[1]]).all()   # … and the context goes on
    win.close()
    # nothing rendered yet
    fresh = gpu.Context(0)
    with pytest.raises(gpu.LfiError, match="nothing rendered"):
        fresh.download_views_yuv420(0, 1, out=host[:1])
    assert (host == poison.SENTINEL).all()
    fresh.close()


@pytest.mark.parametrize("size", [(21, 11), (24, 6)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("layout", ["rgba", "planar"])
def test_frames_equal_those_of_the_surface_call(layout, size, gpu):
    """lfi_download_views_yuv420 is lfi_download_views_yuv into the equivalent descriptor — host memory, I420, tight planes, the array's frame
    stride: 3 views from view 1, frames 5 bytes apart (21x11 padded staged planes, 24x6 the staged frame is the host frame), byte for
    byte; the 5 bytes between the frames keep their poison under both"""
    w, h = size
    ctx, _ = _ctx(gpu, w, h, layout)
    poison.render(ctx, "TEN_WM")
    fb = ref.sizes(w, h)[2]
    fmt = (ref.BT601, ref.FULL)
    want = ref.frames(ctx.download_views(1, 4), *fmt)
    hosts = poison.sentinel((3, fb + 5)), poison.sentinel((3, fb + 5))
    ctx.poison(L.LFI_POISON_SCRATCH, PAD)
    ctx.download_views_yuv420(1, 3, matrix=fmt[0], range=fmt[1], out=hosts[0])
    surfaces = ctx.yuv_surfaces_packed("i420", "host", hosts[1].ctypes.data, keep=hosts[1])
    surfaces.frame_stride = hosts[1].strides[0]
    ctx.poison(L.LFI_POISON_SCRATCH, 0xFF ^ PAD)
    ctx.download_views_yuv(surfaces, 3, v0=1, matrix=fmt[0], range=fmt[1])
    assert (hosts[0] == hosts[1]).all(), int((hosts[0] != hosts[1]).sum())
    assert (hosts[0][:, :fb] == want).all()
    assert (hosts[0][:, fb:] == poison.SENTINEL).all()
    ctx.close()


def test_one_frame_with_a_stride_below_the_frame_is_refused(gpu):
    """n = 1: no second frame starts a stride after the first, and a descriptor of surfaces says nothing about its stride then — the call
    refuses a frame_stride_bytes below the frame's bytes all the same, and writes nothing"""
    w, h = 17, 9
    ctx, _ = _ctx(gpu, w, h, "rgba")
    poison.render(ctx, "STD")
    views = ctx.download_views()
    fb = ref.sizes(w, h)[2]
    host = poison.sentinel((1, fb))
    assert _raw_download(ctx, 2, 1, 0, 0, host, fb - 1) == -1
    assert ctx._lib.lfi_last_error(ctx._h).decode() == ("lfi_download_views_yuv420: the frames' pointer is NULL or frame_stride_bytes is below "
                                                        "W*H + 2*((W+1)/2)*((H+1)/2)")
    assert (host == poison.SENTINEL).all()
    assert _raw_download(ctx, 2, 1, 0, 0, host, fb) == 0 and (host == ref.frames(views[2:3], ref.BT709, ref.LIMITED)).all()
    ctx.close()


@pytest.mark.parametrize("layout", ["rgba", "planar"])
def test_the_buffers_are_counted_and_grow(layout, gpu):
    w, h = 17, 9
    ctx, _ = _ctx(gpu, w, h, layout)
    poison.render(ctx, "STD")
    before = ctx.memory_info().workspace_bytes
    _frames(ctx, 0, 2, ref.FORMATS[0])
    padded = 24 * 10 + 2 * 12 * 5   # Y pitch 24 (a multiple of 8) x 10 rows (even), chroma pitch 12 (a multiple of 4) x 5 rows
    assert ctx.memory_info().workspace_bytes == before + 2 * padded
    _frames(ctx, 0, V, ref.FORMATS[0])
    _frames(ctx, 0, 1, ref.FORMATS[0])
    assert ctx.memory_info().workspace_bytes == before + V * padded   # grows, is kept
    ctx.close()


STREAMS = [
    # (layout, method, all_focus, views per block, total views)
    ("rgba", "STD", False, 2, 7),       # four blocks, a short last one: both buffers of frames are reused
    ("planar", "TEN_WM", False, 2, 7),
    ("rgba", "TEN_WM", False, 3, 3),    # one block
    ("planar", "STD", False, 3, 3),
    ("rgba", "STD", True, 2, 7),        # all-focus
    ("planar", "TEN_WM", True, 2, 7),
]


@pytest.mark.parametrize("case", STREAMS, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("size", [(24, 6), (17, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_stream_equals_block_by_block_renders(size, case, gpu):
    layout, method, all_focus, block, total = case
    w, h = size
    fb = ref.sizes(w, h)[2]
    ctx, _ = _ctx(gpu, w, h, layout, views=block, focus_range=0.3 if all_focus else 0.0)
    hp_all = gpu.build_params(COLS, ROWS, w, h, "0,0,1,1", 0.2, 0.3 if all_focus else 0.0, 3.0, 1.0, total)
    views = np.zeros((total, h, w, 4), np.uint8)
    for b in range(0, total, block):
        hp = hp_all.rows(b, min(b + block, total))
        ctx.set_params(hp)
        if all_focus:
            poison.focus_map(ctx)
        poison.render(ctx, method, all_focus=all_focus)
        views[b:b + hp.weights.shape[0]] = ctx.download_views()
    ctx.set_params(hp_all.rows(0, block))   # the block size of the stream = the views of the parameters
    if all_focus:
        poison.focus_map(ctx)
    rgba_before = None
    if layout == "rgba":
        rgba_before = poison.sentinel((total, h, w, 4))
        ctx.render_stream(method, hp_all.weights, rgba_before, all_focus=all_focus)
        assert (rgba_before == views).all()
    for fmt in (ref.FORMATS[0], ref.FORMATS[3]):
        want = ref.frames(views, *fmt)
        ctx.poison(poison.RENDER, PAD)
        out = ctx.pinned_empty((total, fb + 8))
        out[...] = poison.SENTINEL
        got = ctx.render_stream_yuv420(method, hp_all.weights, out=out, all_focus=all_focus, matrix=fmt[0], range=fmt[1])
        assert (got == want).all(), (size, case, fmt, int((got != want).sum()))
        assert (out[:, fb:] == poison.SENTINEL).all()
        # the views of the last block remain on the device
        last = (total - 1) // block * block
        assert (ctx.download_views(0, total - last) == views[last:]).all()
    # lfi_render_stream and lfi_download_view give the bytes they gave before
    if layout == "rgba":
        again = poison.sentinel((total, h, w, 4))
        ctx.render_stream(method, hp_all.weights, again, all_focus=all_focus)
        assert (again == rgba_before).all()
    else:
        ctx.poison(poison.RENDER, PAD)
        ctx.render_stream(method, hp_all.weights, None, all_focus=all_focus)
        last = (total - 1) // block * block
        assert (ctx.download_views(0, total - last) == views[last:]).all()
    ctx.close()
