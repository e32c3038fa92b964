"""GPU (-m gpu): RGB-D video frames — lfi_download_rgbd_yuv (csrc/hip/rgbd_yuv.hpp): a view and a focus map side by side in one YUV 4:2:0 frame.

The frame is defined in integers (include/lfi.h), so every comparison is `==` on all bytes, against tests/rgbd_yuv_ref.py — the restated quilt
video frame of the 2 x 1 quilt {view, grey image of the depth} — applied to the views' and the maps' own downloads; tests/yuv_surfaces_ref.py
places the bytes.  The maps are injected: random bytes in ALL four channels, so that "the depth is the R byte" is pinned.  The destination
holds a poison before every call and every byte outside the planes must still hold it; the context's scratch buffers hold another.  The
shapes are the smallest at which each mechanism can break: the depth half 2 past the frame's 8-column grid and a band of 2 rows (18 x 10),
everything aligned (16 x 8), the identity (50 x 22), a tile smaller than a block (2 x 2), one frame and three from view 1 on, three chunks
per tile, several pieces per chunk."""
import ctypes as C

import numpy as np
import pytest

import lfinterpolator_amd as L
import poison
import rgbd_yuv_ref as ref
import yuv_ref
import yuv_surfaces_ref as sref
from conftest import SEED
from test_gpu_view_centres import CASES
from test_gpu_view_maps import _estimate, _setup
from test_gpu_yuv_surfaces import FORMAT_NAMES, FORMATS, MEMORIES, MEMORY_NAMES, _Surfaces

pytestmark = pytest.mark.gpu

COLS = ROWS = 3
W, H, V = 50, 22, 10            # as tests/test_gpu_quilt_yuv.py: a width that is not a multiple of four
LAYOUTS = ["rgba", "planar"]
TILES = [(18, 10), (16, 8), (50, 22), (2, 2)]
INVERT, VIEW_MAPS = L.LFI_RGBD_INVERT, L.LFI_RGBD_VIEW_MAPS


def _maps(w, h, seed=0):
    """two maps of random bytes in all four channels: G, B and A differ from R"""
    return [np.random.default_rng(seed * 2 + k + 1).integers(0, 256, (h, w, 4), dtype=np.uint8) for k in (0, 1)]


def _rendered(gpu, layout, views=V, w=W, h=H):
    hp = gpu.build_params(COLS, ROWS, w, h, "0,0,1,1", 0.2, 0.0, 3.0, 1.0, views)
    ctx = gpu.Context(0)
    ctx.set_grid(COLS, ROWS, w, h)
    ctx.fill_synthetic(SEED)
    ctx.set_params(hp)
    ctx.set_output_layout(layout)
    poison.render(ctx, "STD")
    maps = _maps(w, h, seed=w)
    for k in (0, 1):
        ctx.upload_map(k, maps[k])
    return ctx, maps


def _frames(ctx, v0, n, map_k, flags, tw, th, conv, lay, memory, byte, shift=0):
    """the call into n surfaces of layout lay that hold `byte`, the scratch buffers poisoned with another byte: the tight I420 frames [n][frame
    bytes]; asserts that every byte outside the planes still holds `byte`"""
    dst = _Surfaces(ctx, lay, memory, np.full((n, lay.frame_stride), byte, np.uint8), shift=shift)
    ctx.poison(L.LFI_POISON_SCRATCH, byte ^ 0x5A)
    ctx.download_rgbd_yuv(v0, n, map_k, flags, tw, th, conv[0], conv[1], dst.desc)
    got = dst.read()
    assert sref.padding_holds(got, lay, byte), "bytes outside the planes were written"
    return sref.gather(got, lay)


def _want(views, v0, n, depth, tw, th, invert, conv):
    """depth: one map for every frame, or a list with one map per view"""
    return np.stack([ref.frame(views[v], depth[v] if isinstance(depth, list) else depth, tw, th, invert, *conv) for v in range(v0, v0 + n)])


def _layouts(fmt, fw, fh):
    return {"tight": sref.tight(fmt, fw, fh), "pitched": sref.pitched(fmt, fw, fh, align=256, gap=256, tail=256)}


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_destination_and_coefficient_set(layout, gpu):
    """{I420, NV12} x {host, device} x {tight, pitched} x the four coefficient sets x both maps x invert on and off, three frames from view 1 on,
    the destination poisoned with 0x00 and with 0xFF"""
    tw, th, v0, n = 18, 10, 1, 3
    ctx, maps = _rendered(gpu, layout)
    views = ctx.download_views()
    assert all((ctx.download_map(k) == maps[k]).all() for k in (0, 1))
    want = {(conv, k, inv): _want(views, v0, n, maps[k], tw, th, inv, conv) for conv in yuv_ref.FORMATS for k in (0, 1) for inv in (False, True)}
    assert not (want[(yuv_ref.FORMATS[0], 0, False)] == want[(yuv_ref.FORMATS[0], 1, False)]).all()
    assert not (want[(yuv_ref.FORMATS[0], 0, False)] == want[(yuv_ref.FORMATS[0], 0, True)]).all()
    case = 0
    for fmt in FORMATS:
        for memory in MEMORIES:
            for name, lay in _layouts(fmt, 2 * tw, th).items():
                for conv in yuv_ref.FORMATS:
                    for byte in (0x00, 0xFF):
                        k, inv = case & 1, bool(case >> 1 & 1)   # every (conv, map, invert) occurs with every destination pair over the loop
                        case += 1
                        got = _frames(ctx, v0, n, k, INVERT if inv else 0, tw, th, conv, lay, memory, byte)
                        assert (got == want[(conv, k, inv)]).all(), (layout, FORMAT_NAMES[fmt], MEMORY_NAMES[memory], name, conv, k, inv, byte,
                                                                     int((got != want[(conv, k, inv)]).sum()))
    ctx.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("tile", TILES, ids=lambda t: f"{t[0]}x{t[1]}")
def test_frames_equal_the_restatement(tile, layout, gpu):
    """one frame, and three from view 1 on: into a tight host frame (staged), pitched device surfaces (in place) and a device base shifted by
    1 (staged, device-to-device copies)"""
    tw, th = tile
    ctx, maps = _rendered(gpu, layout)
    views = ctx.download_views()
    case = TILES.index(tile)
    for v0, n in ((0, 1), (1, 3), (V - 1, 1)):
        for fmt in FORMATS:
            cases = [(sref.HOST, sref.tight(fmt, 2 * tw, th), 0), (sref.DEVICE, sref.pitched(fmt, 2 * tw, th), 0),
                     (sref.DEVICE, sref.tight(fmt, 2 * tw, th), 1)]
            for memory, lay, shift in cases:
                conv, k, inv = yuv_ref.FORMATS[case % 4], case >> 2 & 1, bool(case >> 3 & 1)
                case += 5
                want = _want(views, v0, n, maps[k], tw, th, inv, conv)
                for byte in poison.POISON:
                    got = _frames(ctx, v0, n, k, INVERT if inv else 0, tw, th, conv, lay, memory, byte, shift=shift)
                    assert (got == want).all(), (layout, tile, v0, n, FORMAT_NAMES[fmt], MEMORY_NAMES[memory], shift, conv, k, inv, byte,
                                                 int((got != want).sum()))
    ctx.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [(1040, 12, 1030, 6), (2100, 4, 2, 2)], ids=["three-chunks", "several-pieces"])
def test_wide_views(shape, layout, gpu):
    """two views of 1040 x 12 as tiles of 1030 x 6: three chunks of 344 columns per half, the depth half 6 past the 8-grid; two views of
    2100 x 4 as tiles of 2 x 2: a chunk's source columns take three pieces of 1024"""
    w, h, tw, th = shape
    ctx, maps = _rendered(gpu, layout, views=2, w=w, h=h)
    views = ctx.download_views()
    for i, fmt in enumerate(FORMATS):
        conv, k, inv = yuv_ref.FORMATS[i + 1], i, bool(i)
        want = _want(views, 0, 2, maps[k], tw, th, inv, conv)
        for memory, lay in ((sref.HOST, sref.tight(fmt, 2 * tw, th)), (sref.DEVICE, sref.pitched(fmt, 2 * tw, th))):
            for byte in poison.POISON:
                got = _frames(ctx, 0, 2, k, INVERT if inv else 0, tw, th, conv, lay, memory, byte)
                assert (got == want).all(), (shape, layout, FORMAT_NAMES[fmt], MEMORY_NAMES[memory], byte, int((got != want).sum()))
    ctx.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_call_has_no_side_effects_and_repeats(layout, gpu):
    """in place the call reserves nothing; the views and the maps are what they were; a second call gives the same bytes"""
    ctx, maps = _rendered(gpu, layout)
    views = ctx.download_views()
    conv = yuv_ref.FORMATS[2]
    before = ctx.memory_info().workspace_bytes
    lay = sref.pitched(sref.NV12, 36, 10)
    dst = _Surfaces(ctx, lay, sref.DEVICE, np.full((V, lay.frame_stride), 0x11, np.uint8))
    ctx.download_rgbd_yuv(0, V, 1, 0, 18, 10, conv[0], conv[1], dst.desc)
    assert (sref.gather(dst.read(), lay) == _want(views, 0, V, maps[1], 18, 10, False, conv)).all()
    assert ctx.memory_info().workspace_bytes == before
    first = {}
    for fmt in FORMATS:
        for memory in MEMORIES:
            first[(fmt, memory)] = _frames(ctx, 2, 4, 0, INVERT, 18, 10, conv, sref.pitched(fmt, 36, 10), memory, 0xA5)
    assert (ctx.download_views() == views).all()
    assert all((ctx.download_map(k) == maps[k]).all() for k in (0, 1))
    for fmt in FORMATS:
        for memory in MEMORIES:
            again = _frames(ctx, 2, 4, 0, INVERT, 18, 10, conv, sref.pitched(fmt, 36, 10), memory, 0x5A)
            assert (again == first[(fmt, memory)]).all()
    ctx.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_per_view_maps(layout, gpu, oracle_c):
    """lfi_view_focus_maps on a small view-centred setup (33 x 17, five views): with LFI_RGBD_VIEW_MAPS frame k's depth is view v0 + k's own
    map, what lfi_download_view_map delivers; without the flag every frame shows the context's map"""
    case = next(c for c in CASES if c[0] == "diag_3x3_oddW")
    ctx, hp, O, ids, lf = _setup(gpu, oracle_c, case, layout=layout)
    w, h, views_n = case[3], case[4], case[8]
    _estimate(ctx, ids)
    poison.render(ctx, "STD", all_focus=True)
    own = _maps(w, h, seed=7)
    for k in (0, 1):
        ctx.upload_map(k, own[k])
    views = ctx.download_views()
    per_view = [[ctx.download_view_map(v, k) for v in range(views_n)] for k in (0, 1)]
    assert not (per_view[1][0] == per_view[1][views_n - 1]).all()   # the cameras see different maps
    case_no = 0
    for tw, th in ((16, 8), (32, 16), (2, 2)):
        for v0, n in ((0, views_n), (2, 2)):
            for fmt in FORMATS:
                for memory, lay in ((sref.HOST, sref.tight(fmt, 2 * tw, th)), (sref.DEVICE, sref.pitched(fmt, 2 * tw, th))):
                    conv, k, inv = yuv_ref.FORMATS[case_no % 4], case_no >> 1 & 1, bool(case_no >> 2 & 1)
                    case_no += 1
                    flags = INVERT if inv else 0
                    got = _frames(ctx, v0, n, k, flags | VIEW_MAPS, tw, th, conv, lay, memory, poison.POISON[case_no & 1])
                    assert (got == _want(views, v0, n, per_view[k], tw, th, inv, conv)).all(), ("view maps", layout, tw, th, v0, n, fmt, memory, k, inv)
                    got = _frames(ctx, v0, n, k, flags, tw, th, conv, lay, memory, poison.POISON[case_no & 1])
                    assert (got == _want(views, v0, n, own[k], tw, th, inv, conv)).all(), ("context map", layout, tw, th, v0, n, fmt, memory, k, inv)
    ctx.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_NAMES.get)
def test_refusals_leave_the_destination_and_the_workspace(fmt, gpu):
    import torch
    tw, th, n = 18, 10, 2
    ctx, maps = _rendered(gpu, "rgba")
    views = ctx.download_views()
    lay = sref.pitched(fmt, 2 * tw, th)
    host = poison.sentinel((n, lay.frame_stride))
    dev = torch.full((n * lay.frame_stride,), poison.SENTINEL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    good = sref.descriptor(L, lay, sref.HOST, host.ctypes.data, keep=host)
    good_dev = sref.descriptor(L, lay, sref.DEVICE, dev.data_ptr(), keep=dev)
    want = _want(views, 1, n, maps[1], tw, th, False, (yuv_ref.BT709, yuv_ref.LIMITED))

    def valid():
        """the next valid call is correct"""
        ctx.download_rgbd_yuv(1, n, 1, 0, tw, th, 0, 0, good)
        assert (sref.gather(host, lay) == want).all()
        host[...] = poison.SENTINEL

    valid()
    before = ctx.memory_info().workspace_bytes
    lib = ctx._lib

    def raw(handle, v0, n_, k, flags, a, b, m, r, desc):
        return lib.lfi_download_rgbd_yuv(handle, v0, n_, k, flags, a, b, m, r, C.byref(desc) if desc is not None else None)

    def make(memory=sref.HOST, base=host.ctypes.data, **changes):
        d = dict(fmt=lay.fmt, frame_stride=lay.frame_stride, y_pitch=lay.y_pitch, c_offset=lay.c_offset, c_pitch=lay.c_pitch, cr_offset=lay.cr_offset)
        d.update(changes)
        return L.YuvSurfaces.make(d["fmt"], memory, base, d["frame_stride"], d["y_pitch"], d["c_offset"], d["c_pitch"], d["cr_offset"], keep=host)

    pinned = ctx.pinned_empty((4 * lay.frame_stride,))
    refused = []
    for d in (good, good_dev):
        refused += [
            ("n = 0", (1, 0, 1, 0, tw, th, 0, 0, d), "views"),
            ("n below 0", (1, -1, 1, 0, tw, th, 0, 0, d), "views"),
            ("v0 below 0", (-1, n, 1, 0, tw, th, 0, 0, d), "views"),
            ("v0 + n beyond the views", (V - 1, n, 1, 0, tw, th, 0, 0, d), "views"),
            ("odd tile_w", (1, n, 1, 0, tw - 1, th, 0, 0, d), "even"),
            ("odd tile_h", (1, n, 1, 0, tw, th - 1, 0, 0, d), "even"),
            ("tile_w = W + 2", (1, n, 1, 0, W + 2, th, 0, 0, d), "scaled quilt tiles"),
            ("tile_h = H + 2", (1, n, 1, 0, tw, H + 2, 0, 0, d), "scaled quilt tiles"),
            ("tile_w = 0", (1, n, 1, 0, 0, th, 0, 0, d), "scaled quilt tiles"),
            ("tile_h below 0", (1, n, 1, 0, tw, -2, 0, 0, d), "scaled quilt tiles"),
            ("map_k = 2", (1, n, 2, 0, tw, th, 0, 0, d), "map index"),
            ("map_k below 0", (1, n, -1, 0, tw, th, 0, 0, d), "map index"),
            ("an unknown flag bit", (1, n, 1, 4, tw, th, 0, 0, d), "flags"),
            ("all flag bits", (1, n, 1, 0xFFFFFFFF, tw, th, 0, 0, d), "flags"),
            ("per-view maps that are not in use", (1, n, 1, VIEW_MAPS, tw, th, 0, 0, d), "lfi_view_focus_maps"),
            ("unknown matrix", (1, n, 1, 0, tw, th, 2, 0, d), "matrix"),
            ("unknown range", (1, n, 1, 0, tw, th, 0, -1, d), "range"),
        ]
    refused += [
        ("NULL descriptor", (1, n, 1, 0, tw, th, 0, 0, None), "NULL"),
        ("NULL base", (1, n, 1, 0, tw, th, 0, 0, make(base=None)), "NULL"),
        ("unknown format", (1, n, 1, 0, tw, th, 0, 0, make(fmt=2)), "format"),
        ("unknown memory", (1, n, 1, 0, tw, th, 0, 0, make(memory=2)), "memory"),
        ("y_pitch below 2*tile_w", (1, n, 1, 0, tw, th, 0, 0, make(y_pitch=2 * tw - 1)), "pitch"),
        ("a frame for ONE tile", (1, n, 1, 0, tw, th, 0, 0, make(y_pitch=tw, c_pitch=tw)), "pitch"),
        ("c_pitch below its minimum", (1, n, 1, 0, tw, th, 0, 0, make(c_pitch=tw - 1)), "pitch"),
        ("chroma inside the Y plane", (1, n, 1, 0, tw, th, 0, 0, make(c_offset=th * lay.y_pitch - 1)), "overlap"),
        ("frame_stride below a frame's extent", (1, n, 1, 0, tw, th, 0, 0, make(frame_stride=lay.extent - 1)), "frame_stride"),
        ("a host pointer as LFI_MEM_DEVICE", (1, n, 1, 0, tw, th, 0, 0, make(memory=sref.DEVICE)), "device memory"),
        ("page-locked host memory as LFI_MEM_DEVICE", (1, n, 1, 0, tw, th, 0, 0, make(memory=sref.DEVICE, base=pinned.ctypes.data)), "device memory"),
    ]
    for what, args, word in refused:
        assert raw(ctx._h, *args) == -1, what   # LFI_EINVAL
        assert word in lib.lfi_last_error(ctx._h).decode(), (what, lib.lfi_last_error(ctx._h).decode())
        assert (host == poison.SENTINEL).all(), what
        assert ctx.memory_info().workspace_bytes == before, what
    torch.cuda.synchronize()
    assert (dev.cpu().numpy() == poison.SENTINEL).all()
    valid()
    ctx.download_rgbd_yuv(1, n, 1, 0, tw, th, 0, 0, good_dev)   # … and into the device frames
    torch.cuda.synchronize()
    assert (sref.gather(dev.cpu().numpy().reshape(n, lay.frame_stride), lay) == want).all()
    ctx.close()
    # nothing rendered yet
    fresh = gpu.Context(0)
    fresh.set_grid(COLS, ROWS, W, H)
    assert raw(fresh._h, 0, 1, 1, 0, tw, th, 0, 0, good) == -1 and "nothing rendered" in lib.lfi_last_error(fresh._h).decode()
    fresh.close()
    # a row window: a 2 x 2 block may straddle the band, a tile's rows average rows it does not hold
    hp = gpu.build_params(COLS, ROWS, W, H, "0,0,1,1", 0.2, 0.0, 3.0, 1.0, V)
    band = (4, 12)
    win = gpu.Context(0)
    win.set_grid(COLS, ROWS, W, H)
    in_rows = gpu.input_rows(band, hp.focused_offsets, H)
    win.set_row_window(band[0], band[1], in_rows[0], in_rows[1])
    win.fill_synthetic(SEED)
    win.set_params(hp)
    poison.render(win, "STD")
    assert raw(win._h, 0, 1, 1, 0, tw, th, 0, 0, good) == -1 and "row window" in lib.lfi_last_error(win._h).decode()
    assert (win.download_view(0)[band[0]:band[1]] == views[0][band[0]:band[1]]).all()   # … and the context goes on
    win.close()
    assert (host == poison.SENTINEL).all()
