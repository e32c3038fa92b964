"""GPU (-m gpu): quilt video frames — lfi_download_quilt_yuv (csrc/hip/quilt_yuv.hpp for even tile sizes, quilt_scale + yuvs_convert for odd ones).

The frame is defined in integers (include/lfi.h), so every comparison is `==` on all bytes, against tests/quilt_yuv_ref.py — the restated
scaled quilt taken as one view by the restated YUV frame — applied to the views' own downloads; tests/yuv_surfaces_ref.py places the bytes.
The destination holds a poison before every call and every byte outside the planes must still hold it; the context's scratch buffers hold
another.  The shapes are the smallest at which each mechanism can break: tile origins 2, 4 and 6 past the frame's 8-column grid and a band
of 2 rows (18 x 10), everything aligned (16 x 8), the identity (50 x 22), a tile smaller than a block (2 x 2), blocks that straddle tiles
and odd frame sizes (17 x 9, 18 x 9, 25 x 11, 1 x 1: the staged path), three chunks per tile, several pieces per chunk."""
import ctypes as C

import numpy as np
import pytest

import lfinterpolator_amd as L
import poison
import quilt_yuv_ref as ref
import scaled_quilt_ref
import yuv_ref
import yuv_surfaces_ref as sref
from conftest import SEED
from test_gpu_yuv_surfaces import FORMAT_NAMES, FORMATS, MEMORIES, MEMORY_NAMES, _Surfaces

pytestmark = pytest.mark.gpu

COLS = ROWS = 3
W, H, V = 50, 22, 10            # as tests/test_gpu_scaled_quilt.py: a width that is not a multiple of four
LAYOUTS = ["rgba", "planar"]


def _ctx(gpu, layout, views=V, w=W, h=H):
    hp = gpu.build_params(COLS, ROWS, w, h, "0,0,1,1", 0.2, 0.0, 3.0, 1.0, views)
    ctx = gpu.Context(0)
    ctx.set_grid(COLS, ROWS, w, h)
    ctx.fill_synthetic(SEED)
    ctx.set_params(hp)
    ctx.set_output_layout(layout)
    return ctx


def _rendered(gpu, layout, views=V, w=W, h=H):
    ctx = _ctx(gpu, layout, views, w, h)
    poison.render(ctx, "STD")
    return ctx


def _frame(ctx, tx, ty, tw, th, conv, lay, memory, byte, v0=0, shift=0):
    """the call into a destination of layout lay that holds `byte`, the scratch buffers poisoned with another byte: the tight I420 frame; asserts
    that every byte outside the planes still holds `byte`"""
    dst = _Surfaces(ctx, lay, memory, np.full((1, lay.frame_stride), byte, np.uint8), shift=shift)
    ctx.poison(L.LFI_POISON_SCRATCH, byte ^ 0x5A)
    ctx.download_quilt_yuv(tx, ty, v0, tw, th, conv[0], conv[1], dst.desc)
    got = dst.read()
    assert sref.padding_holds(got, lay, byte), "bytes outside the planes were written"
    return sref.gather(got, lay)[0]


def _layouts(fmt, qw, qh):
    return {"tight": sref.tight(fmt, qw, qh), "pitched": sref.pitched(fmt, qw, qh, align=256, gap=256, tail=256)}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("quilt", [(4, 2, 18, 10), (3, 3, 17, 9)], ids=["fused-18x10", "staged-17x9"])
def test_every_destination_and_coefficient_set(quilt, layout, gpu):
    """{I420, NV12} x {host, device} x {tight, pitched} x the four coefficient sets, the destination poisoned with 0x00 and with 0xFF"""
    tx, ty, tw, th = quilt
    ctx = _rendered(gpu, layout)
    views = ctx.download_views()
    scaled = scaled_quilt_ref.quilt(views, tx, ty, tw, th)
    want = {conv: yuv_ref.frame(scaled, *conv) for conv in yuv_ref.FORMATS}
    assert (want[yuv_ref.FORMATS[0]] == ref.frame(views, tx, ty, tw, th, *yuv_ref.FORMATS[0])).all()
    for fmt in FORMATS:
        for memory in MEMORIES:
            for name, lay in _layouts(fmt, tx * tw, ty * th).items():
                for conv in yuv_ref.FORMATS:
                    for byte in (0x00, 0xFF):
                        got = _frame(ctx, tx, ty, tw, th, conv, lay, memory, byte)
                        assert (got == want[conv]).all(), (quilt, layout, FORMAT_NAMES[fmt], MEMORY_NAMES[memory], name, conv, byte,
                                                           int((got != want[conv]).sum()))
    ctx.close()


# (tiles_x, tiles_y, tile_w, tile_h, v0): fused — aligned, the identity, a tile smaller than a block, origins off the grid with v0 > 0;
# staged — straddling blocks in x and y, in y only, odd QW and QH, one pixel
SHAPES = [(4, 2, 16, 8, 0), (4, 2, 50, 22, 1), (4, 2, 2, 2, 0), (3, 3, 18, 10, 1), (1, 1, 18, 10, 7),
          (3, 3, 17, 9, 0), (3, 3, 18, 9, 1), (3, 3, 25, 11, 0), (1, 1, 1, 1, 9), (3, 3, 1, 1, 0)]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_frames_equal_the_restatement(layout, gpu):
    ctx = _rendered(gpu, layout)
    views = ctx.download_views()
    for k, (tx, ty, tw, th, v0) in enumerate(SHAPES):
        conv = yuv_ref.FORMATS[k % 4]
        want = ref.frame(views[v0:], tx, ty, tw, th, *conv)
        for fmt in FORMATS:
            cases = [(sref.HOST, sref.tight(fmt, tx * tw, ty * th), 0), (sref.DEVICE, sref.pitched(fmt, tx * tw, ty * th), 0),
                     (sref.DEVICE, sref.tight(fmt, tx * tw, ty * th), 1)]   # base + 1: not in place, the staged copies
            for memory, lay, shift in cases:
                for byte in poison.POISON:
                    got = _frame(ctx, tx, ty, tw, th, conv, lay, memory, byte, v0=v0, shift=shift)
                    assert (got == want).all(), (layout, (tx, ty, tw, th, v0), FORMAT_NAMES[fmt], MEMORY_NAMES[memory], shift, byte, int((got != want).sum()))
    # the views' own size: the frame of the unscaled quilt
    assert (ref.frame(views[1:], 4, 2, W, H, *yuv_ref.FORMATS[1]) == yuv_ref.frame(ctx.download_quilt(4, 2, v0=1), *yuv_ref.FORMATS[1])).all()
    ctx.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [(1040, 12, 1030, 6), (2100, 4, 2, 2)], ids=["three-chunks", "several-pieces"])
def test_wide_views(shape, layout, gpu):
    """two views of 1040 x 12 as tiles of 1030 x 6: three chunks of 344 columns per tile, the second tile's origin 6 past the 8-grid; two
    views of 2100 x 4 as tiles of 2 x 2: a chunk's source columns take three pieces of 1024"""
    w, h, tw, th = shape
    ctx = _rendered(gpu, layout, views=2, w=w, h=h)
    views = ctx.download_views()
    for k, fmt in enumerate(FORMATS):
        conv = yuv_ref.FORMATS[k + 1]
        want = ref.frame(views, 2, 1, tw, th, *conv)
        for memory, lay in ((sref.HOST, sref.tight(fmt, 2 * tw, th)), (sref.DEVICE, sref.pitched(fmt, 2 * tw, th))):
            for byte in poison.POISON:
                got = _frame(ctx, 2, 1, tw, th, conv, lay, memory, byte)
                assert (got == want).all(), (shape, layout, FORMAT_NAMES[fmt], MEMORY_NAMES[memory], byte, int((got != want).sum()))
    ctx.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_odd_tiles_of_small_views(layout, gpu):
    """four views of 13 x 7 as tiles of 5 x 3 in a 2 x 2 quilt: odd tile sizes take the RGBA quilt (quilt_scale, then yuvs_convert of the quilt as
    ONE view of 10 x 6).  QW = 10 is no multiple of 8: a tight host I420 frame is not the staged frame and leaves through the packed copy; a
    16-aligned device NV12 surface is written in place"""
    tx, ty, tw, th = 2, 2, 5, 3
    ctx = _rendered(gpu, layout, views=4, w=13, h=7)
    views = ctx.download_views()
    i420, nv12 = FORMATS
    cases = [(i420, sref.HOST, sref.tight(i420, tx * tw, ty * th)), (nv12, sref.DEVICE, sref.pitched(nv12, tx * tw, ty * th, align=16, gap=16, tail=16))]
    for k, (fmt, memory, lay) in enumerate(cases):
        assert memory == sref.HOST or (lay.y_pitch | lay.c_offset | lay.c_pitch | lay.frame_stride) % 16 == 0
        for conv in (yuv_ref.FORMATS[k], yuv_ref.FORMATS[k + 2]):
            want = ref.frame(views, tx, ty, tw, th, *conv)
            for byte in poison.POISON:
                got = _frame(ctx, tx, ty, tw, th, conv, lay, memory, byte)
                assert (got == want).all(), (layout, FORMAT_NAMES[fmt], MEMORY_NAMES[memory], conv, byte, int((got != want).sum()))
    ctx.close()


def _attached(gpu, layout, content):
    """a context whose views are a torch buffer that holds `content` ([n][h][w][4], alpha 255) in the layout's device form"""
    import torch
    n, h, w = content.shape[:3]
    ctx = _ctx(gpu, layout, views=n, w=w, h=h)
    vl = ctx.view_layout()
    if layout == "planar":
        pitch = vl.row_pitch_bytes
        dev = np.full((n, 3, h, pitch), 0x77, np.uint8)
        dev[:, :, :, :w] = content[..., :3].transpose(0, 3, 1, 2)
    else:
        dev = content
    buf = torch.from_numpy(np.ascontiguousarray(dev).reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    ctx.attach_views(buf.data_ptr(), buf.numel())
    return ctx, buf


@pytest.mark.parametrize("layout", LAYOUTS)
def test_identity_tiles_of_attached_views_reach_the_extremes(layout, gpu):
    """views written directly into attached view memory: the 8 cube corners in every 2 x 2 arrangement, uniform corners and greys (128 x 66 x 3
    holds all 4096 arrangements) — 16, 235, 240 and the 255 clamp, through the fused kernel at the views' own size"""
    w, h, n = 128, 66, 3
    content = yuv_ref.corner_views(w, h, n)
    ctx, buf = _attached(gpu, layout, content)
    assert (ctx.download_views() == content).all()
    for conv in yuv_ref.FORMATS:
        want = ref.frame(content, 3, 1, w, h, *conv)
        for fmt in FORMATS:
            got = _frame(ctx, 3, 1, w, h, conv, sref.pitched(fmt, 3 * w, h), sref.DEVICE, 0xA5)
            assert (got == want).all(), (layout, conv, FORMAT_NAMES[fmt])
        y, c = got[:3 * w * h], got[3 * w * h:]
        if conv[1] == yuv_ref.LIMITED:
            assert (y.min(), y.max(), c.min(), c.max()) == (16, 235, 16, 240)
        else:
            assert (y.min(), y.max(), c.max()) == (0, 255, 255)
    # … and scaled, with v0 > 0, from attached views
    want = ref.frame(content[1:], 2, 1, 18, 10, *yuv_ref.FORMATS[0])
    got = _frame(ctx, 2, 1, 18, 10, yuv_ref.FORMATS[0], sref.tight(sref.NV12, 36, 10), sref.HOST, 0x5A, v0=1)
    assert (got == want).all()
    ctx.close()
    del buf


def test_the_fused_path_makes_no_rgba_quilt(gpu):
    """a device surface written in place: even tiles need no buffer at all, 17 x 9 tiles the RGBA quilt of 51 x 27 pixels"""
    ctx = _rendered(gpu, "rgba")
    views = ctx.download_views()
    before = ctx.memory_info().workspace_bytes
    conv = yuv_ref.FORMATS[0]
    for tx, ty, tw, th in ((4, 2, 18, 10), (3, 3, 16, 8), (4, 2, 50, 22)):
        lay = sref.pitched(sref.NV12, tx * tw, ty * th)
        dst = _Surfaces(ctx, lay, sref.DEVICE, np.full((1, lay.frame_stride), 0x11, np.uint8))
        ctx.download_quilt_yuv(tx, ty, 0, tw, th, conv[0], conv[1], dst.desc)
        assert (sref.gather(dst.read(), lay)[0] == ref.frame(views, tx, ty, tw, th, *conv)).all()
        assert ctx.memory_info().workspace_bytes == before, (tx, ty, tw, th)
    lay = sref.pitched(sref.NV12, 51, 27)
    dst = _Surfaces(ctx, lay, sref.DEVICE, np.full((1, lay.frame_stride), 0x11, np.uint8))
    ctx.download_quilt_yuv(3, 3, 0, 17, 9, conv[0], conv[1], dst.desc)
    assert (sref.gather(dst.read(), lay)[0] == ref.frame(views, 3, 3, 17, 9, *conv)).all()
    assert ctx.memory_info().workspace_bytes == before + 51 * 27 * 4
    ctx.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_call_has_no_side_effects(layout, gpu):
    ctx = _rendered(gpu, layout)
    views = ctx.download_views()
    maps = [np.random.default_rng(k).integers(0, 256, (H, W, 4), dtype=np.uint8) for k in (0, 1)]
    for k in (0, 1):
        ctx.upload_map(k, maps[k])
    ctx.keep_views()
    scaled = ctx.download_quilt_scaled(3, 3, 17, 9)
    lay = sref.pitched(sref.I420, W, H)
    surf = _Surfaces(ctx, lay, sref.HOST, np.full((V, lay.frame_stride), 0x22, np.uint8))
    ctx.download_views_yuv(surf.desc)
    frames = surf.read().copy()
    conv = yuv_ref.FORMATS[2]
    first = {}
    for tx, ty, tw, th in ((4, 2, 18, 10), (3, 3, 17, 9)):
        for fmt in FORMATS:
            for memory in MEMORIES:
                first[(tx, tw, fmt, memory)] = _frame(ctx, tx, ty, tw, th, conv, sref.pitched(fmt, tx * tw, ty * th), memory, 0xA5)
    assert (ctx.download_views() == views).all()
    assert all((ctx.download_map(k) == maps[k]).all() for k in (0, 1))
    per_view, _ = ctx.compare_views(None)
    assert all(per_view[v].differing_bytes == 0 for v in range(V))   # the kept views are still the views
    ctx.poison(L.LFI_POISON_SCRATCH, 0x5A)
    assert (ctx.download_quilt_scaled(3, 3, 17, 9) == scaled).all()
    surf = _Surfaces(ctx, lay, sref.HOST, np.full((V, lay.frame_stride), 0x22, np.uint8))
    ctx.download_views_yuv(surf.desc)
    assert (surf.read() == frames).all()
    # two calls give the same bytes
    for tx, ty, tw, th in ((4, 2, 18, 10), (3, 3, 17, 9)):
        for fmt in FORMATS:
            for memory in MEMORIES:
                again = _frame(ctx, tx, ty, tw, th, conv, sref.pitched(fmt, tx * tw, ty * th), memory, 0x5A)
                assert (again == first[(tx, tw, fmt, memory)]).all()
    ctx.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_NAMES.get)
def test_refusals_leave_the_destination_and_the_workspace(fmt, gpu):
    import torch
    tx, ty, tw, th = 4, 2, 18, 10
    ctx = _rendered(gpu, "rgba")
    views = ctx.download_views()
    lay = sref.pitched(fmt, tx * tw, ty * th)
    host = poison.sentinel((1, lay.frame_stride))
    dev = torch.full((lay.frame_stride,), poison.SENTINEL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    good = sref.descriptor(L, lay, sref.HOST, host.ctypes.data, keep=host)
    good_dev = sref.descriptor(L, lay, sref.DEVICE, dev.data_ptr(), keep=dev)
    want = ref.frame(views, tx, ty, tw, th, yuv_ref.BT709, yuv_ref.LIMITED)
    odd = ref.frame(views, 3, 3, 17, 9, yuv_ref.BT709, yuv_ref.LIMITED)
    odd_lay = sref.tight(fmt, 51, 27)

    def valid():
        """the next valid calls are correct: fused into the host frame, staged into another"""
        ctx.download_quilt_yuv(tx, ty, 0, tw, th, 0, 0, good)
        assert (sref.gather(host, lay)[0] == want).all()
        host[...] = poison.SENTINEL
        assert (_frame(ctx, 3, 3, 17, 9, (0, 0), odd_lay, sref.HOST, 0xA5) == odd).all()

    valid()
    before = ctx.memory_info().workspace_bytes
    lib = ctx._lib

    def raw(a, b, v0, c, d, m, r, desc):
        return lib.lfi_download_quilt_yuv(ctx._h, a, b, v0, c, d, m, r, C.byref(desc) if desc is not None else None)

    def make(memory=sref.HOST, base=host.ctypes.data, **changes):
        d = dict(fmt=lay.fmt, frame_stride=lay.frame_stride, y_pitch=lay.y_pitch, c_offset=lay.c_offset, c_pitch=lay.c_pitch, cr_offset=lay.cr_offset)
        d.update(changes)
        return L.YuvSurfaces.make(d["fmt"], memory, base, d["frame_stride"], d["y_pitch"], d["c_offset"], d["c_pitch"], d["cr_offset"], keep=host)

    pinned = ctx.pinned_empty((4 * lay.frame_stride,))
    refused = []
    for d in (good, good_dev):
        refused += [
            ("too many tiles", (4, 3, 0, tw, th, 0, 0, d), "quilt needs"),
            ("no tiles", (0, 2, 0, tw, th, 0, 0, d), "quilt needs"),
            ("v0 + tiles beyond the views", (tx, ty, 3, tw, th, 0, 0, d), "quilt needs"),
            ("v0 below 0", (tx, ty, -1, tw, th, 0, 0, d), "quilt needs"),
            ("tile_w = W + 1", (1, 1, 0, W + 1, th, 0, 0, d), "scaled quilt tiles"),
            ("tile_h = H + 1", (1, 1, 0, tw, H + 1, 0, 0, d), "scaled quilt tiles"),
            ("tile_w = 0", (tx, ty, 0, 0, th, 0, 0, d), "scaled quilt tiles"),
            ("tile_h = 0", (tx, ty, 0, tw, 0, 0, 0, d), "scaled quilt tiles"),
            ("unknown matrix", (tx, ty, 0, tw, th, 2, 0, d), "matrix"),
            ("unknown range", (tx, ty, 0, tw, th, 0, -1, d), "range"),
        ]
    refused += [
        ("NULL descriptor", (tx, ty, 0, tw, th, 0, 0, None), "NULL"),
        ("NULL base", (tx, ty, 0, tw, th, 0, 0, make(base=None)), "NULL"),
        ("unknown format", (tx, ty, 0, tw, th, 0, 0, make(fmt=2)), "format"),
        ("unknown memory", (tx, ty, 0, tw, th, 0, 0, make(memory=2)), "memory"),
        ("y_pitch below QW", (tx, ty, 0, tw, th, 0, 0, make(y_pitch=tx * tw - 1)), "pitch"),
        ("c_pitch below its minimum", (tx, ty, 0, tw, th, 0, 0, make(c_pitch=tx * tw // 2 - 1)), "pitch"),
        ("chroma inside the Y plane", (tx, ty, 0, tw, th, 0, 0, make(c_offset=ty * th * lay.y_pitch - 1)), "overlap"),
        ("Cr inside Cb / cr_offset with NV12", (tx, ty, 0, tw, th, 0, 0, make(cr_offset=lay.c_offset + 1)), "cr_offset"),
        ("a host pointer as LFI_MEM_DEVICE", (tx, ty, 0, tw, th, 0, 0, make(memory=sref.DEVICE)), "device memory"),
        ("page-locked host memory as LFI_MEM_DEVICE", (tx, ty, 0, tw, th, 0, 0, make(memory=sref.DEVICE, base=pinned.ctypes.data)), "device memory"),
    ]
    for what, args, word in refused:
        assert raw(*args) == -1, what   # LFI_EINVAL
        assert word in lib.lfi_last_error(ctx._h).decode(), (what, lib.lfi_last_error(ctx._h).decode())
        assert (host == poison.SENTINEL).all(), what
        assert ctx.memory_info().workspace_bytes == before, what
    torch.cuda.synchronize()
    assert (dev.cpu().numpy() == poison.SENTINEL).all()
    valid()
    ctx.download_quilt_yuv(tx, ty, 0, tw, th, 0, 0, good_dev)   # … and into the device frame
    torch.cuda.synchronize()
    assert (sref.gather(dev.cpu().numpy().reshape(1, lay.frame_stride), lay)[0] == want).all()
    ctx.close()
    # nothing rendered yet
    fresh = gpu.Context(0)
    fresh.set_grid(COLS, ROWS, W, H)
    assert lib.lfi_download_quilt_yuv(fresh._h, tx, ty, 0, tw, th, 0, 0, C.byref(good)) == -1 and "nothing rendered" in lib.lfi_last_error(fresh._h).decode()
    fresh.close()
    # a row window: a tile's rows average source rows the band does not hold
    hp = gpu.build_params(COLS, ROWS, W, H, "0,0,1,1", 0.2, 0.0, 3.0, 1.0, V)
    band = (4, 12)
    win = gpu.Context(0)
    win.set_grid(COLS, ROWS, W, H)
    in_rows = gpu.input_rows(band, hp.focused_offsets, H)
    win.set_row_window(band[0], band[1], in_rows[0], in_rows[1])
    win.fill_synthetic(SEED)
    win.set_params(hp)
    poison.render(win, "STD")
    assert lib.lfi_download_quilt_yuv(win._h, tx, ty, 0, tw, th, 0, 0, C.byref(good)) == -1 and "row window" in lib.lfi_last_error(win._h).decode()
    got = np.zeros((2 * H, 3 * W, 4), np.uint8)   # … and the context goes on: the unscaled quilt of the band
    win.download_quilt_tiles(got, 3, 2, 0, 6)
    assert (got[band[0]:band[1], :W] == views[0][band[0]:band[1]]).all()
    win.close()
    assert (host == poison.SENTINEL).all()


@pytest.mark.parametrize("size", [(65536, 2), (2, 65536)], ids=["width-65536", "height-65536"])
def test_an_axis_above_65535_is_refused(size, gpu):
    """views of 65536 pixels along one axis (attached: nothing of that shape needs to be rendered): the area filter's spans are 32-bit products
    of up to 65535², so the call refuses them as lfi_download_quilt_scaled does, before it looks at the destination"""
    import torch
    w, h = size
    content = np.random.default_rng(w).integers(0, 256, (1, h, w, 4), dtype=np.uint8)
    content[..., 3] = 255
    ctx, buf = _attached(gpu, "rgba", content)
    lay = sref.tight(sref.NV12, 2, 2)
    host = poison.sentinel((1, 64))
    dev = torch.full((64,), poison.SENTINEL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    before = ctx.memory_info().workspace_bytes
    lib = ctx._lib
    for d in (sref.descriptor(L, lay, sref.HOST, host.ctypes.data, keep=host), sref.descriptor(L, lay, sref.DEVICE, dev.data_ptr(), keep=dev)):
        for _ in range(2):
            assert lib.lfi_download_quilt_yuv(ctx._h, 1, 1, 0, 2, 2, 0, 0, C.byref(d)) == -1   # LFI_EINVAL
            assert "65535" in lib.lfi_last_error(ctx._h).decode(), lib.lfi_last_error(ctx._h).decode()
            assert ctx.memory_info().workspace_bytes == before
    torch.cuda.synchronize()
    assert (host == poison.SENTINEL).all() and (dev.cpu().numpy() == poison.SENTINEL).all()
    with pytest.raises(gpu.LfiError, match="65535"):   # the RGBA call's refusal, word for word
        ctx.download_quilt_scaled(1, 1, 2, 2)
    assert (ctx.download_views() == content).all()   # … and the context goes on
    assert ctx.memory_info().workspace_bytes >= before
    ctx.close()
    del buf
