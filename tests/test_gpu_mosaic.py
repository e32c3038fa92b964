"""GPU (-m gpu): mosaic input — lfi_upload_mosaic_yuv (csrc/hip/yuv_mosaic.hpp) and lfi_upload_mosaic: ONE frame that holds the grid's images
as tiles, split on the device.  The conversion is defined in integers (include/lfi.h), so every comparison is `==` on all bytes of the grid,
against tests/mosaic_ref.py — which only crops the tiles and hands them to tests/yuv_in_ref.py / tests/yuv_left_ref.py as they are.  The grid
is poisoned first; tiles hold independent random bytes, so a neighbouring tile's chroma or a wrong origin changes the result; every case runs
twice, with different bytes in the pitch padding and in the tiles outside the call's range, and both runs must give the same grid.

The staged route's chunking (more than 256 MiB of tile rows) is not run here — no frame of a few seconds exceeds the cap; its plan is covered
on the CPU (tests/test_host_mosaic.py: test_chunks_are_whole_tile_rows_under_the_cap), and every staged case below runs the one-chunk loop."""
import ctypes as C

import numpy as np
import pytest

import lfinterpolator_amd as L
import mosaic_ref as mref
import poison
import yuv_in_ref as in_ref
import yuv_surfaces_ref as sref
from conftest import SEED
from test_gpu_yuv_surfaces import FORMAT_NAMES, FORMATS, PATTERN, _attached, _read, _reset, _Surfaces

pytestmark = pytest.mark.gpu

# (matrix, range, chroma filter, left-sited): the four coefficient sets, both filters, both sitings
CONVERSIONS = [
    (in_ref.BT709, in_ref.LIMITED, in_ref.BILINEAR, False),
    (in_ref.BT709, in_ref.FULL, in_ref.NEAREST, False),
    (in_ref.BT601, in_ref.LIMITED, in_ref.BILINEAR, True),
    (in_ref.BT601, in_ref.FULL, in_ref.BILINEAR, False),
    (in_ref.BT709, in_ref.FULL, in_ref.BILINEAR, True),
    (in_ref.BT601, in_ref.LIMITED, in_ref.NEAREST, True),
]

# name: (tiles_x, tiles_y, W, H, order, bottom_up, first_tile, n, g0) — each chosen for what it can break:
CASES = {
    # Y origins 0, 6, 12, 18, 24 and I420 chroma origins 0, 3, 6, 9, 12: every byte phase of the unaligned path, one ragged block per tile
    "5x1_6x2_rows": (5, 1, 6, 2, "rows", False, 0, 5, 0),
    # … of which tiles 2 and 3 only, into images 1 and 2 of five: the others keep their poison, the other tiles' bytes reach nothing
    "5x1_6x2_rows_tiles_2_3": (5, 1, 6, 2, "rows", False, 2, 2, 1),
    # a full block plus a ragged one, two tile rows, chroma row clamps at inner tile edges, the column-major mapping
    "3x2_10x4_grid": (3, 2, 10, 4, "grid", False, 0, 6, 0),
    "3x2_10x4_grid_bottom_up": (3, 2, 10, 4, "grid", True, 0, 6, 0),
    # the aligned path, a tile wider than a wave's 512 columns; the second tile starts mid-wave at column 520
    "2x2_520x4_grid": (2, 2, 520, 4, "grid", False, 0, 4, 0),
    # one block per tile
    "2x1_8x2_rows": (2, 1, 8, 2, "rows", False, 0, 2, 0),
    # the minimum size
    "2x1_2x2_rows": (2, 1, 2, 2, "rows", False, 0, 2, 0),
    # unaligned tiles wider than a wave: 65 blocks, the last one ragged, the second tile at byte phase 2
    "2x1_514x2_rows": (2, 1, 514, 2, "rows", False, 0, 2, 0),
}


def _grid_of(case):
    tiles_x, tiles_y, w, h, order, bottom_up, first_tile, n, g0 = case
    return (tiles_x, tiles_y) if order == "grid" else (tiles_x * tiles_y, 1)


def _frame(mw, mh, seed):
    return np.random.default_rng(seed).integers(0, 256, in_ref.sizes(mw, mh)[2], dtype=np.uint8)


def _other_outside(frame, mw, mh, w, h, tiles, seed):
    """the frame with other random bytes in every tile that is not one of `tiles`"""
    y, cb, cr = (p.copy() for p in in_ref.split(frame, mw, mh))
    other = [p for p in in_ref.split(_frame(mw, mh, seed), mw, mh)]
    keep_y, keep_c = np.zeros(y.shape, bool), np.zeros(cb.shape, bool)
    for tx, ty, _ in tiles:
        keep_y[ty * h:(ty + 1) * h, tx * w:(tx + 1) * w] = True
        keep_c[ty * h // 2:(ty + 1) * h // 2, tx * w // 2:(tx + 1) * w // 2] = True
    return in_ref.pack(np.where(keep_y, y, other[0]), np.where(keep_c, cb, other[1]), np.where(keep_c, cr, other[2]))


def _ways(fmt, mw, mh):
    """(name, layout, memory, shift, in place): the four ways a frame reaches the call"""
    return [("device in place", sref.pitched(fmt, mw, mh), sref.DEVICE, 0, True), ("device at base + 2", sref.tight(fmt, mw, mh), sref.DEVICE, 2, False),
            ("host tight", sref.tight(fmt, mw, mh), sref.HOST, 0, False), ("host pitched", sref.pitched(fmt, mw, mh), sref.HOST, 0, False)]


def _want(frame, case, conv, n_images):
    tiles_x, tiles_y, w, h, order, bottom_up, first_tile, n, g0 = case
    cols, rows = _grid_of(case)
    tiles = mref.mosaic_map(tiles_x, tiles_y, first_tile, n, mref.GRID if order == "grid" else mref.ROWS, mref.BOTTOM_UP if bottom_up else 0, cols, rows, g0)
    want = np.full((n_images, h, w, 4), PATTERN, np.uint8)
    for g, image in mref.expand(frame, tiles_x * w, tiles_y * h, w, h, tiles, conv[0], conv[1], conv[2], conv[3]).items():
        want[g] = image
    return want, tiles


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_NAMES.get)
@pytest.mark.parametrize("name", list(CASES))
def test_grid_equals_the_restatement(name, fmt, gpu):
    case = CASES[name]
    tiles_x, tiles_y, w, h, order, bottom_up, first_tile, n, g0 = case
    cols, rows = _grid_of(case)
    mw, mh = tiles_x * w, tiles_y * h
    ctx, grid = _attached(gpu, cols, rows, w, h)
    mosaic = L.Mosaic.make(tiles_x, tiles_y, order, bottom_up, first_tile, n)
    frame = _frame(mw, mh, 7)
    _, tiles = _want(frame, case, CONVERSIONS[0], cols * rows)
    runs = [(frame, 0x00), (_other_outside(frame, mw, mh, w, h, tiles, 8), 0xFF)]
    assert n == tiles_x * tiles_y or not (runs[0][0] == runs[1][0]).all()
    for conv in CONVERSIONS:
        want, _ = _want(frame, case, conv, cols * rows)
        assert (_want(runs[1][0], case, conv, cols * rows)[0] == want).all()   # the restatement itself reads no other tile
        ctx.set_yuv_siting("left" if conv[3] else "centre", "centre")
        for way, lay, memory, shift, in_place in _ways(fmt, mw, mh):
            for content, byte in runs:
                surfaces = _Surfaces(ctx, lay, memory, sref.scatter(content[None], lay, byte), shift=shift)
                _reset(grid)
                ctx.poison(L.LFI_POISON_SCRATCH, byte ^ 0x5A)
                before = ctx.memory_info().workspace_bytes
                ctx.upload_mosaic_yuv(mosaic, surfaces.desc, g0, matrix=conv[0], range=conv[1], chroma=conv[2])
                got = _read(ctx, grid)
                assert (got == want).all(), (name, FORMAT_NAMES[fmt], way, conv, byte, int((got != want).sum()), np.argwhere((got != want).any(axis=(1, 2, 3))).ravel().tolist())
                assert (surfaces.read()[0] == sref.scatter(content[None], lay, byte)[0]).all(), "the source frame was written"
                if in_place:
                    assert ctx.memory_info().workspace_bytes == before, way   # read where it lies: no staging buffer
    ctx.close()
    del grid


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_NAMES.get)
def test_one_tile_is_upload_images_yuv_of_the_frame(fmt, gpu):
    """1 x 1 of 24 x 10, call against call: the same grid as lfi_upload_images_yuv of the same surfaces, under every conversion and way"""
    w, h = 24, 10
    ctx, grid = _attached(gpu, 1, 1, w, h)
    frame = _frame(w, h, 9)
    for conv in CONVERSIONS:
        ctx.set_yuv_siting("left" if conv[3] else "centre", "centre")
        for way, lay, memory, shift, _ in _ways(fmt, w, h):
            surfaces = _Surfaces(ctx, lay, memory, sref.scatter(frame[None], lay, 0xA5), shift=shift)
            _reset(grid)
            ctx.upload_images_yuv(surfaces.desc, 1, matrix=conv[0], range=conv[1], chroma=conv[2])
            want = _read(ctx, grid)
            assert not (want == PATTERN).all()
            _reset(grid)
            ctx.upload_mosaic_yuv(L.Mosaic.make(1, 1, "rows"), surfaces.desc, matrix=conv[0], range=conv[1], chroma=conv[2])
            assert (_read(ctx, grid) == want).all(), (way, conv)
            _reset(grid)
            ctx.upload_mosaic_yuv(L.Mosaic.make(1, 1, "grid", bottom_up=True), surfaces.desc, matrix=conv[0], range=conv[1], chroma=conv[2])
            assert (_read(ctx, grid) == want).all(), (way, conv)
    ctx.close()
    del grid


def test_a_rendered_quilt_frame_comes_back_as_the_views_own_frames(gpu):
    """render; lfi_download_quilt_yuv with tile = W x H into a device surface; lfi_upload_mosaic_yuv of that surface into a second context: the
    images are lfi_upload_images_yuv of the same views' own frames from lfi_download_views_yuv.  Nothing leaves the card in between"""
    cols, rows, w, h, views = 3, 3, 16, 8, 4
    hp = gpu.build_params(cols, rows, w, h, "0,0,1,1", 0.2, 0.0, 3.0, 1.0, views)
    src = gpu.Context(0)
    src.set_grid(cols, rows, w, h)
    src.fill_synthetic(SEED)
    src.set_params(hp)
    poison.render(src, "STD")
    for fmt in FORMATS:
        quilt_lay, view_lay = sref.pitched(fmt, 2 * w, 2 * h), sref.pitched(fmt, w, h)
        quilt = _Surfaces(src, quilt_lay, sref.DEVICE, np.full((1, quilt_lay.frame_stride), 0x11, np.uint8))
        own = _Surfaces(src, view_lay, sref.DEVICE, np.full((views, view_lay.frame_stride), 0x22, np.uint8))
        src.download_quilt_yuv(2, 2, 0, w, h, "601", "full", quilt.desc)
        src.download_views_yuv(own.desc, matrix="601", range="full")
        src.sync()
        dst, grid = _attached(gpu, views, 1, w, h)
        dst.upload_images_yuv(own.desc, views, matrix="601", range="full")
        want = _read(dst, grid)
        assert not (want == PATTERN).all(axis=(1, 2, 3)).any()   # every image was written
        _reset(grid)
        dst.upload_mosaic_yuv(L.Mosaic.make(2, 2, "rows"), quilt.desc, matrix="601", range="full")
        assert (_read(dst, grid) == want).all(), FORMAT_NAMES[fmt]
        dst.close()
        del grid
    src.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_NAMES.get)
def test_refusals_leave_the_grid_and_the_staging_buffer(fmt, gpu):
    tiles_x, tiles_y, w, h = 3, 2, 10, 4
    mw, mh = tiles_x * w, tiles_y * h
    frame = _frame(mw, mh, 11)
    lay = sref.pitched(fmt, mw, mh)
    host = sref.scatter(frame[None], lay, 0)
    ctx, grid = _attached(gpu, tiles_x, tiles_y, w, h)
    good = sref.descriptor(L, lay, sref.HOST, host.ctypes.data, keep=host)
    good_mosaic = L.Mosaic.make(tiles_x, tiles_y, "grid")
    deep = L.YuvSurfaces.make(fmt | L.LFI_YUV_10BIT, sref.HOST, host.ctypes.data, lay.frame_stride, lay.y_pitch, lay.c_offset, lay.c_pitch, lay.cr_offset, keep=host)

    def desc(memory=sref.HOST, base=host.ctypes.data, **changes):
        d = dict(fmt=lay.fmt, y_pitch=lay.y_pitch, c_offset=lay.c_offset, c_pitch=lay.c_pitch, cr_offset=lay.cr_offset)
        d.update(changes)
        return L.YuvSurfaces.make(d["fmt"], memory, base, lay.frame_stride, d["y_pitch"], d["c_offset"], d["c_pitch"], d["cr_offset"], keep=host)

    # device memory that ends before the frame does: another context's own grid (16 KiB) under a descriptor whose rows are 1 MiB apart —
    # the frame's extent is above 8 MiB, whatever the allocator rounds 16 KiB up to
    other = gpu.Context(0)
    other.set_grid(1, 1, 64, 64)
    big = 1 << 20
    early = desc(memory=sref.DEVICE, base=other.grid_device_ptr()[0], y_pitch=big, c_offset=mh * big, c_pitch=big,
                 cr_offset=0 if fmt == sref.NV12 else mh * big + (mh // 2) * big)
    assert early.check(mw, mh, 1)
    before = ctx.memory_info().workspace_bytes
    lib = ctx._lib
    raw = lambda m, g0, mat, rng, chroma, d: lib.lfi_upload_mosaic_yuv(ctx._h, C.byref(m) if m is not None else None, g0, mat, rng, chroma,
                                                                         C.byref(d) if d is not None else None)
    refused = [
        ("NULL mosaic", (None, 0, 0, 0, 0, good), "NULL"),
        ("NULL descriptor", (good_mosaic, 0, 0, 0, 0, None), "NULL"),
        ("NULL base", (good_mosaic, 0, 0, 0, 0, desc(base=None)), "NULL"),
        ("GRID with a partial range", (L.Mosaic.make(tiles_x, tiles_y, "grid", n=5), 0, 0, 0, 0, good), "LFI_MOSAIC_GRID"),
        ("GRID with another grid", (L.Mosaic.make(tiles_y, tiles_x, "grid"), 0, 0, 0, 0, good), "LFI_MOSAIC_GRID"),
        ("tiles past the last tile", (L.Mosaic.make(tiles_x, tiles_y, "rows", first_tile=4, n=3), 0, 0, 0, 0, good), "first_tile"),
        ("images past the last image", (L.Mosaic.make(tiles_x, tiles_y, "rows"), 1, 0, 0, 0, good), "inside"),
        ("unknown order", (L.Mosaic(tiles_x, tiles_y, 0, 6, 2, 0), 0, 0, 0, 0, good), "order"),
        ("unknown flag", (L.Mosaic(tiles_x, tiles_y, 0, 6, 1, 2), 0, 0, 0, 0, good), "flags"),
        ("unknown matrix", (good_mosaic, 0, 2, 0, 0, good), "matrix"),
        ("unknown range", (good_mosaic, 0, 0, 2, 0, good), "range"),
        ("unknown chroma", (good_mosaic, 0, 0, 0, 2, good), "chroma"),
        ("a 10-bit format", (good_mosaic, 0, 0, 0, 0, deep), "10-bit"),
        ("y_pitch below the frame's width", (good_mosaic, 0, 0, 0, 0, desc(y_pitch=mw - 1)), "pitch"),
        ("a descriptor of one tile", (good_mosaic, 0, 0, 0, 0, desc(c_offset=h * lay.y_pitch)), "overlap"),
        ("a host pointer as LFI_MEM_DEVICE", (good_mosaic, 0, 0, 0, 0, desc(memory=sref.DEVICE)), "device memory"),
        ("a device allocation that ends early", (good_mosaic, 0, 0, 0, 0, early), "allocation ends"),
    ]
    for what, args, word in refused:
        assert raw(*args) == -1, what   # LFI_EINVAL
        assert word in lib.lfi_last_error(ctx._h).decode(), (what, lib.lfi_last_error(ctx._h).decode())
        assert (_read(ctx, grid) == PATTERN).all(), what
        assert ctx.memory_info().workspace_bytes == before, what
    # … and the context goes on: the mosaic, then an 8-bit lfi_upload_images_yuv as on a fresh context
    ctx.upload_mosaic_yuv(good_mosaic, good)
    want = np.full((6, h, w, 4), PATTERN, np.uint8)
    tiles = mref.mosaic_map(tiles_x, tiles_y, 0, 6, mref.GRID, 0, tiles_x, tiles_y, 0)
    for g, image in mref.expand(frame, mw, mh, w, h, tiles, in_ref.BT709, in_ref.LIMITED).items():
        want[g] = image
    assert (_read(ctx, grid) == want).all()
    frames = np.random.default_rng(12).integers(0, 256, (6, in_ref.sizes(w, h)[2]), dtype=np.uint8)
    view_lay = sref.pitched(fmt, w, h)
    own = _Surfaces(ctx, view_lay, sref.HOST, sref.scatter(frames, view_lay, 0x5A))
    ctx.upload_images_yuv(own.desc, 6)
    assert (_read(ctx, grid) == in_ref.images(frames, w, h, in_ref.BT709, in_ref.LIMITED)).all()
    ctx.close()
    other.close()
    del grid
    # an odd image size; no grid; a row window; released inputs
    for cw, chh in ((5, 4), (10, 3)):
        odd = gpu.Context(0)
        odd.set_grid(tiles_x, tiles_y, cw, chh)
        assert odd._lib.lfi_upload_mosaic_yuv(odd._h, C.byref(good_mosaic), 0, 0, 0, 0, C.byref(good)) == -1
        assert "even" in odd._lib.lfi_last_error(odd._h).decode()
        odd.close()
    fresh = gpu.Context(0)
    assert fresh._lib.lfi_upload_mosaic_yuv(fresh._h, C.byref(good_mosaic), 0, 0, 0, 0, C.byref(good)) == -1
    assert "lfi_set_grid" in fresh._lib.lfi_last_error(fresh._h).decode()
    fresh.close()
    win = gpu.Context(0)
    win.set_grid(tiles_x, tiles_y, w, h)
    win.set_row_window(1, 3, 0, 4)
    assert win._lib.lfi_upload_mosaic_yuv(win._h, C.byref(good_mosaic), 0, 0, 0, 0, C.byref(good)) == -1 and "row window" in win._lib.lfi_last_error(win._h).decode()
    win.close()
    hp = gpu.build_params(tiles_x, tiles_y, w, h, "0,0,1,1", 0.2, 0.0, 3.0, 1.0, 4)
    rel = gpu.Context(0)
    rel.set_grid(tiles_x, tiles_y, w, h)
    rel.fill_synthetic(SEED)
    rel.set_params(hp)
    poison.render(rel, "TEN_WM")
    views = rel.download_views()
    rel.release_inputs()
    assert rel._lib.lfi_upload_mosaic_yuv(rel._h, C.byref(good_mosaic), 0, 0, 0, 0, C.byref(good)) == -1 and "released" in rel._lib.lfi_last_error(rel._h).decode()
    poison.render(rel, "TEN_WM")
    assert (rel.download_views() == views).all()
    rel.close()


def test_renders_are_ordered_around_a_mosaic_upload(gpu):
    """a render issued right after the upload, without a host wait, reads the mosaic's images; the next upload right behind it does not
    disturb it"""
    cols, rows, w, h, views = 3, 2, 16, 8, 4
    hp = gpu.build_params(cols, rows, w, h, "0,0,1,1", 0.2, 0.0, 3.0, 1.0, views)
    mw, mh = cols * w, rows * h
    lay = sref.pitched(sref.NV12, mw, mh)
    frames = [_frame(mw, mh, 20), _frame(mw, mh, 21)]
    tiles = mref.mosaic_map(cols, rows, 0, cols * rows, mref.GRID, 0, cols, rows, 0)
    yuv, rgba = gpu.Context(0), gpu.Context(0)
    for ctx in (yuv, rgba):
        ctx.set_grid(cols, rows, w, h)
        ctx.fill_synthetic(SEED)
        ctx.set_params(hp)
    want = []
    for frame in frames:
        images = mref.expand(frame, mw, mh, w, h, tiles, in_ref.BT709, in_ref.LIMITED)
        rgba.upload_grid(np.stack([images[g] for g in range(cols * rows)]))
        poison.render(rgba, "STD")
        want.append(rgba.download_views())
    assert not (want[0] == want[1]).all()
    surfaces = [_Surfaces(yuv, lay, sref.HOST, sref.scatter(f[None], lay, 0xFF)) for f in frames]
    mosaic = L.Mosaic.make(cols, rows, "grid")
    for step in (0, 1, 0):
        yuv.poison(poison.RENDER, 0xA5)
        yuv.upload_mosaic_yuv(mosaic, surfaces[step].desc)
        yuv.render("STD")                                            # no host wait in between
        yuv.upload_mosaic_yuv(mosaic, surfaces[1 - step].desc)       # … and the next upload right behind the render
        yuv.sync()
        assert (yuv.download_views() == want[step]).all(), step
        poison.render(yuv, "STD")
        assert (yuv.download_views() == want[1 - step]).all(), step
    yuv.close()
    rgba.close()


# ---- lfi_upload_mosaic: RGBA ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [(3, 2, 5, 3, "grid", False), (3, 2, 4, 2, "rows", True)], ids=["3x2_5x3_grid", "3x2_4x2_rows_bottom_up"])
def test_rgba_mosaic_equals_the_crops(case, gpu):
    tiles_x, tiles_y, w, h, order, bottom_up = case
    cols, rows = (tiles_x, tiles_y) if order == "grid" else (tiles_x * tiles_y, 1)
    ctx, grid = _attached(gpu, cols, rows, w, h)
    tiles = mref.mosaic_map(tiles_x, tiles_y, 0, tiles_x * tiles_y, mref.GRID if order == "grid" else mref.ROWS, mref.BOTTOM_UP if bottom_up else 0, cols, rows, 0)
    for pad in (0, 3):   # tight rows, and rows with a pitch of three pixels more
        image = np.random.default_rng(30 + pad).integers(0, 256, (tiles_y * h, tiles_x * w + pad, 4), dtype=np.uint8)
        pinned = ctx.pinned_empty(image.shape)
        pinned[...] = image
        for source in (image, pinned):
            _reset(grid)
            ctx.upload_mosaic(L.Mosaic.make(tiles_x, tiles_y, order, bottom_up), source)
            got = _read(ctx, grid)
            for g, crop in mref.rgba_tiles(image, w, h, tiles).items():
                assert (got[g] == crop).all(), (case, pad, g)
    # a sub-range: tiles 1 and 2 into images 3 and 4 of a row of images; the others keep the pattern
    if order == "rows":
        _reset(grid)
        ctx.upload_mosaic(L.Mosaic.make(tiles_x, tiles_y, order, bottom_up, first_tile=1, n=2), image, g0=3)
        got = _read(ctx, grid)
        part = mref.mosaic_map(tiles_x, tiles_y, 1, 2, mref.ROWS, mref.BOTTOM_UP, cols, rows, 3)
        assert [int(g) for _, _, g in part] == [3, 4]
        for g, crop in mref.rgba_tiles(image, w, h, part).items():
            assert (got[g] == crop).all(), g
        assert (got[:3] == PATTERN).all() and (got[5:] == PATTERN).all()
    # refusals
    lib = ctx._lib
    m = L.Mosaic.make(tiles_x, tiles_y, order, bottom_up)
    _reset(grid)
    assert lib.lfi_upload_mosaic(ctx._h, C.byref(m), 0, None, image.strides[0]) == -1
    assert lib.lfi_upload_mosaic(ctx._h, C.byref(m), 0, image.ctypes.data, tiles_x * w * 4 - 1) == -1 and "pitch" in lib.lfi_last_error(ctx._h).decode()
    assert lib.lfi_upload_mosaic(ctx._h, None, 0, image.ctypes.data, image.strides[0]) == -1
    assert lib.lfi_upload_mosaic(ctx._h, C.byref(m), 1, image.ctypes.data, image.strides[0]) == -1
    assert (_read(ctx, grid) == PATTERN).all()
    ctx.close()
    del grid
