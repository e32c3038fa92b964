"""GPU (-m gpu): lfi_upload_mosaic_yuv_derived (csrc/hip/yuv_mosaic_derived.hpp) — ONE YUV 4:2:0 frame that holds the grid's images as tiles,
split straight into the derived planar copy of a context whose RGBA inputs were released; and lfi_debug_set_mosaic_chunk_cap, which lets a
small frame run the staged route of both mosaic YUV calls with more than one chunk.

Everything is integers, so every comparison is `==` on all bytes: the whole copy, padding included, against the composition
derived_ref.planes(mosaic_ref.expand(...)) (checked by hand in tests/test_host_mosaic_derived.py), and against a twin context that took the
same mosaic through lfi_upload_mosaic_yuv BEFORE its release; renders against the twin's.  Before every call the copy holds the target's
images with every colour byte XOR 0x80, so no byte of it — image or padding — can be left unwritten and pass; images the call does not map
hold random images and must keep them.  Every case runs twice, with different bytes in the pitch padding and in the tiles
outside the call's range, and both runs must give the same copy."""
import ctypes as C

import numpy as np
import pytest

import lfinterpolator_amd as L
import derived_ref
import mosaic_ref as mref
import poison
import yuv_in_ref as in_ref
import yuv_surfaces_ref as sref
from test_gpu_mosaic import CONVERSIONS, _frame, _grid_of, _other_outside, _ways
from test_gpu_yuv_surfaces import FORMAT_NAMES, FORMATS, PATTERN, _attached, _read, _reset, _Surfaces

pytestmark = pytest.mark.gpu

SPAN = L.LFI_YUV_DERIVED_SPAN   # bytes (= pixels) of a plane row per workgroup of the kernel
VIEWS = 4
# a staged tile row of the 1 x 3 mosaic of 24 x 4 tiles is 24 * 4 * 3/2 = 144 bytes: a cap below one row gives one row per chunk, a cap of
# two rows two chunks (tests/test_host_mosaic_derived.py asserts the plans)
CAP_ONE_ROW, CAP_TWO_ROWS = 1, 288
# name: ((tiles_x, tiles_y, W, H, order, bottom_up, first_tile, n, g0), focus, chunk cap) — each chosen for what it can break; the focus of
# each gives padx + phase[g] of both parities and three residues mod 4 (two images: two), asserted on the CPU
CASES = {
    # every byte phase of the unaligned loads, a tile narrower than a block, the whole image inside one span's padding logic
    "5x1_6x2_rows": ((5, 1, 6, 2, "rows", False, 0, 5, 0), 0.23, 0),
    # … of which tiles 2 and 3 only, into images 1 and 2 of five: the others keep their poison, the other tiles' bytes reach nothing
    "5x1_6x2_rows_tiles_2_3": ((5, 1, 6, 2, "rows", False, 2, 2, 1), 0.23, 0),
    # g = tx * rows + r is not contiguous: phase[g] and the plane address come from g; chroma row clamps at inner tile edges
    "3x2_10x4_grid": ((3, 2, 10, 4, "grid", False, 0, 6, 0), 0.23, 0),
    "3x2_10x4_grid_bottom_up": ((3, 2, 10, 4, "grid", True, 0, 6, 0), 0.23, 0),
    # aligned, a span boundary inside the image, a block both neighbouring workgroups compute, six block rows: a second blockIdx.y
    "2x1_span8x12_rows": ((2, 1, SPAN + 8, 12, "rows", False, 0, 2, 0), 0.23, 0),
    # the same for the unaligned kernel, the second tile at byte phase 2
    "2x1_span10x12_rows": ((2, 1, SPAN + 10, 12, "rows", False, 0, 2, 0), 0.23, 0),
    # the minimum size
    "2x1_2x2_rows": ((2, 1, 2, 2, "rows", False, 0, 2, 0), 1.1, 0),
    # the staged route in three chunks of one tile row, and bottom-up in two: ty_bias != 0
    "1x3_24x4_rows_three_chunks": ((1, 3, 24, 4, "rows", False, 0, 3, 0), 0.1, CAP_ONE_ROW),
    "1x3_24x4_rows_bottom_up_two_chunks": ((1, 3, 24, 4, "rows", True, 0, 3, 0), 0.1, CAP_TWO_ROWS),
}
CAPPED = [name for name in CASES if CASES[name][2]]


def params(case, focus):
    cols, rows = _grid_of(case)
    return L.build_params(cols, rows, case[2], case[3], "0,0,1,1", focus, 0.0, 3.0, 1.0, VIEWS)


def _inverse(rgba):
    out = rgba.copy()
    out[..., :3] ^= 0x80
    return out


def _before(want, case):
    """the images a context holds before the call: the mapped ones with every colour byte XOR 0x80, the others what they stay"""
    out = want.copy()
    for g in _tiles(case)[:, 2]:
        out[int(g)] = _inverse(want[int(g)])
    return out


def _tiles(case):
    tiles_x, tiles_y, w, h, order, bottom_up, first_tile, n, g0 = case
    cols, rows = _grid_of(case)
    return mref.mosaic_map(tiles_x, tiles_y, first_tile, n, mref.GRID if order == "grid" else mref.ROWS, mref.BOTTOM_UP if bottom_up else 0, cols, rows, g0)


def want_images(frame, case, conv):
    """[N][H][W][4]: what the grid's images are after the call — the mapped ones from the frame (tests/mosaic_ref.py), the others random"""
    tiles_x, tiles_y, w, h = case[:4]
    cols, rows = _grid_of(case)
    images = np.random.default_rng(5).integers(0, 256, (cols * rows, h, w, 4), dtype=np.uint8)
    for g, image in mref.expand(frame, tiles_x * w, tiles_y * h, w, h, _tiles(case), conv[0], conv[1], conv[2], conv[3]).items():
        images[g] = image
    return images


def restatement(frame, case, conv, layout, phases):
    """the copy after the call: derived_ref.planes over mosaic_ref.expand"""
    return derived_ref.planes(want_images(frame, case, conv), layout, phases)


def _lean(gpu, case, focus, images, cap=0):
    """a context of this case's grid whose copy was built from `images` and whose RGBA planes were released"""
    cols, rows = _grid_of(case)
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, case[2], case[3])
    ctx.upload_grid(images)
    ctx.set_params(params(case, focus))
    ctx.release_inputs()
    ctx.set_mosaic_chunk_cap(cap)
    return ctx


def _poison_copy(ctx, images):
    for g in range(images.shape[0]):
        ctx.upload_image(g, images[g])   # through the one-image staging plane and planar_build


_twins = {}


def _twin(gpu, name, conv):
    """(frame, want images, layout, planes, {method: views}) of a context that held the images of _before, took the mosaic through
    lfi_upload_mosaic_yuv and THEN released its inputs; once per case and conversion"""
    key = (name, conv)
    if key not in _twins:
        case, focus, _ = CASES[name]
        tiles_x, tiles_y, w, h, order, bottom_up, first_tile, n, g0 = case
        cols, rows = _grid_of(case)
        mw, mh = tiles_x * w, tiles_y * h
        frame = _frame(mw, mh, 7)
        want = want_images(frame, case, conv)
        ctx = gpu.Context(0)
        ctx.set_grid(cols, rows, w, h)
        ctx.set_yuv_siting("left" if conv[3] else "centre", "centre")
        ctx.upload_grid(_before(want, case))
        lay = sref.tight(sref.I420, mw, mh)
        surfaces = _Surfaces(ctx, lay, sref.HOST, sref.scatter(frame[None], lay, 0))
        ctx.upload_mosaic_yuv(L.Mosaic.make(tiles_x, tiles_y, order, bottom_up, first_tile, n), surfaces.desc, g0, matrix=conv[0], range=conv[1], chroma=conv[2])
        ctx.upload_wait()
        ctx.set_params(params(case, focus))
        ctx.release_inputs()
        layout, planes = ctx.derived_layout(), ctx.download_derived()
        views = {}
        for method in ("TEN_WM", "STD"):
            poison.render(ctx, method)
            views[method] = ctx.download_views()
        ctx.close()
        _twins[key] = (frame, want, layout, planes, views)
    return _twins[key]


# ---- 1: every byte, and the renders ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_NAMES.get)
@pytest.mark.parametrize("name", list(CASES))
def test_every_byte_of_the_copy_and_the_renders(name, fmt, gpu):
    case, focus, cap = CASES[name]
    tiles_x, tiles_y, w, h, order, bottom_up, first_tile, n, g0 = case
    cols, rows = _grid_of(case)
    mw, mh = tiles_x * w, tiles_y * h
    mosaic = L.Mosaic.make(tiles_x, tiles_y, order, bottom_up, first_tile, n)
    tiles = _tiles(case)
    ctx = None
    for conv in CONVERSIONS:
        frame, want_rgba, twin_lay, twin_planes, twin_views = _twin(gpu, name, conv)
        inverse = _before(want_rgba, case)
        mapped = sorted(int(g) for g in tiles[:, 2])
        if ctx is None:
            ctx = _lean(gpu, case, focus, inverse, cap)
            lay = ctx.derived_layout()
            assert lay == twin_lay, "the two contexts laid their copies out differently"
            assert (lay.rows, lay.n) == (h, cols * rows) and lay.pitch_bytes % 128 == 0
        ctx.set_yuv_siting("left" if conv[3] else "centre", "centre")
        want = restatement(frame, case, conv, lay, lay.phases)
        assert (twin_planes == want).all(), conv   # the path from before: yuvs_mosaic_expand, then planar_build
        poisoned = derived_ref.planes(inverse, lay, lay.phases)
        assert (poisoned[mapped] != want[mapped]).all() and (np.delete(poisoned, mapped, 0) == np.delete(want, mapped, 0)).all()
        runs = [(frame, 0x00), (_other_outside(frame, mw, mh, w, h, tiles, 8), 0xFF)]
        assert n == tiles_x * tiles_y or not (runs[0][0] == runs[1][0]).all()
        assert (restatement(runs[1][0], case, conv, lay, lay.phases) == want).all()   # the restatement itself reads no other tile
        for way, surface_layout, memory, shift, in_place in _ways(fmt, mw, mh):
            for content, byte in runs:
                scattered = sref.scatter(content[None], surface_layout, byte)
                surfaces = _Surfaces(ctx, surface_layout, memory, scattered, shift=shift)
                _poison_copy(ctx, inverse)
                assert (ctx.download_derived() == poisoned).all()
                ctx.poison(L.LFI_POISON_SCRATCH, byte ^ 0x5A)
                before = ctx.memory_info().workspace_bytes
                ctx.upload_mosaic_yuv_derived(mosaic, surfaces.desc, g0, matrix=conv[0], range=conv[1], chroma=conv[2])
                got = ctx.download_derived()
                what = (name, FORMAT_NAMES[fmt], way, conv, byte)
                assert (got == want).all(), (what, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
                assert (got == twin_planes).all(), what
                assert (surfaces.read()[0] == scattered[0]).all(), "the source frame was written"
                if in_place:
                    assert ctx.memory_info().workspace_bytes == before, way   # read where it lies: no staging buffer
                assert ctx.derived_layout() == lay
        for method in ("TEN_WM", "STD"):
            poison.render(ctx, method)
            assert (ctx.download_views() == twin_views[method]).all(), (name, conv, method)
    ctx.close()


# ---- 2: the cap is shared: the same chunks through lfi_upload_mosaic_yuv -------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_NAMES.get)
@pytest.mark.parametrize("name", CAPPED)
def test_the_rgba_call_honours_the_cap(name, fmt, gpu):
    case, _, cap = CASES[name]
    tiles_x, tiles_y, w, h, order, bottom_up, first_tile, n, g0 = case
    cols, rows = _grid_of(case)
    mw, mh = tiles_x * w, tiles_y * h
    ctx, grid = _attached(gpu, cols, rows, w, h)
    ctx.set_mosaic_chunk_cap(cap)
    mosaic = L.Mosaic.make(tiles_x, tiles_y, order, bottom_up, first_tile, n)
    frame = _frame(mw, mh, 7)
    for conv in CONVERSIONS:
        want = np.full((cols * rows, h, w, 4), PATTERN, np.uint8)
        for g, image in mref.expand(frame, mw, mh, w, h, _tiles(case), conv[0], conv[1], conv[2], conv[3]).items():
            want[g] = image
        ctx.set_yuv_siting("left" if conv[3] else "centre", "centre")
        for way, lay, memory, shift, _ in _ways(fmt, mw, mh):
            surfaces = _Surfaces(ctx, lay, memory, sref.scatter(frame[None], lay, 0xFF), shift=shift)
            _reset(grid)
            ctx.upload_mosaic_yuv(mosaic, surfaces.desc, g0, matrix=conv[0], range=conv[1], chroma=conv[2])
            got = _read(ctx, grid)
            assert (got == want).all(), (name, FORMAT_NAMES[fmt], way, conv, int((got != want).sum()))
    # … and cap 0 is the call's own again
    ctx.set_mosaic_chunk_cap(0)
    _reset(grid)
    ctx.upload_mosaic_yuv(mosaic, surfaces.desc, g0, matrix=conv[0], range=conv[1], chroma=conv[2])
    assert (_read(ctx, grid) == want).all()
    ctx.close()
    del grid


# ---- 3: one tile is the frame call ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_NAMES.get)
def test_one_tile_is_upload_images_yuv_derived_of_the_frame(fmt, gpu):
    """1 x 1 of 24 x 10, call against call: the same copy as lfi_upload_images_yuv_derived of the same surfaces, under every conversion and way"""
    case, w, h = (1, 1, 24, 10, "rows", False, 0, 1, 0), 24, 10
    frame = _frame(w, h, 9)
    images = np.random.default_rng(6).integers(0, 256, (1, h, w, 4), dtype=np.uint8)
    ctx = _lean(gpu, case, 0.5, images)
    lay = ctx.derived_layout()
    poisoned = derived_ref.planes(images, lay, lay.phases)
    for conv in CONVERSIONS:
        ctx.set_yuv_siting("left" if conv[3] else "centre", "centre")
        for way, surface_layout, memory, shift, _ in _ways(fmt, w, h):
            surfaces = _Surfaces(ctx, surface_layout, memory, sref.scatter(frame[None], surface_layout, 0xA5), shift=shift)
            ctx.upload_images_yuv_derived(surfaces.desc, 1, matrix=conv[0], range=conv[1], chroma=conv[2])
            want = ctx.download_derived()
            assert not (want == poisoned).all()
            for mosaic in (L.Mosaic.make(1, 1, "rows"), L.Mosaic.make(1, 1, "grid", bottom_up=True)):
                _poison_copy(ctx, images)
                assert (ctx.download_derived() == poisoned).all()
                ctx.upload_mosaic_yuv_derived(mosaic, surfaces.desc, matrix=conv[0], range=conv[1], chroma=conv[2])
                assert (ctx.download_derived() == want).all(), (way, conv)
    ctx.close()


# ---- 4: ordering ----------------------------------------------------------------------------------------------------------------------------------

ORDER_CASE, ORDER_FOCUS = (3, 2, 16, 8, "grid", False, 0, 6, 0), 0.23


@pytest.mark.parametrize("memory", [sref.HOST, sref.DEVICE], ids=["host", "device"])
def test_renders_are_ordered_around_the_call(memory, gpu):
    """render, call, render without a host wait in between: the render issued before the call shows the old frame, the one behind it the new"""
    case = ORDER_CASE
    cols, rows, w, h = case[:4]
    mw, mh = cols * w, rows * h
    conv = CONVERSIONS[0]
    frames = [_frame(mw, mh, 20), _frame(mw, mh, 21)]
    hp = params(case, ORDER_FOCUS)
    rgba = gpu.Context(0)
    rgba.set_grid(cols, rows, w, h)
    rgba.set_params(hp)
    want = []
    for frame in frames:
        rgba.upload_grid(want_images(frame, case, conv))
        poison.render(rgba, "STD")
        want.append(rgba.download_views())
    rgba.close()
    assert not (want[0] == want[1]).all()
    lean = _lean(gpu, case, ORDER_FOCUS, want_images(frames[1], case, conv))
    lay = sref.pitched(sref.NV12, mw, mh)
    surfaces = [_Surfaces(lean, lay, memory, sref.scatter(f[None], lay, 0xFF)) for f in frames]
    mosaic = L.Mosaic.make(cols, rows, "grid")
    for step in (0, 1, 0):
        lean.poison(poison.RENDER, 0xA5)
        lean.upload_mosaic_yuv_derived(mosaic, surfaces[step].desc)
        lean.render("STD")                                                   # no host wait in between
        lean.upload_mosaic_yuv_derived(mosaic, surfaces[1 - step].desc)      # … and the next call right behind the render
        lean.sync()
        assert (lean.download_views() == want[step]).all(), step
        poison.render(lean, "STD")
        assert (lean.download_views() == want[1 - step]).all(), step
    lean.close()


# ---- 5: refusals ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_NAMES.get)
def test_refusals_leave_the_copy_and_the_staging_buffer(fmt, gpu):
    case, focus = (3, 2, 10, 4, "grid", False, 0, 6, 0), 0.23
    tiles_x, tiles_y, w, h = case[:4]
    mw, mh = tiles_x * w, tiles_y * h
    conv = CONVERSIONS[0]
    frame = _frame(mw, mh, 11)
    lay = sref.pitched(fmt, mw, mh)
    host = sref.scatter(frame[None], lay, 0)
    good = sref.descriptor(L, lay, sref.HOST, host.ctypes.data, keep=host)
    good_mosaic = L.Mosaic.make(tiles_x, tiles_y, "grid")
    deep = L.YuvSurfaces.make(fmt | L.LFI_YUV_10BIT, sref.HOST, host.ctypes.data, lay.frame_stride, lay.y_pitch, lay.c_offset, lay.c_pitch, lay.cr_offset, keep=host)

    def desc(memory=sref.HOST, base=host.ctypes.data, **changes):
        d = dict(fmt=lay.fmt, y_pitch=lay.y_pitch, c_offset=lay.c_offset, c_pitch=lay.c_pitch, cr_offset=lay.cr_offset)
        d.update(changes)
        return L.YuvSurfaces.make(d["fmt"], memory, base, lay.frame_stride, d["y_pitch"], d["c_offset"], d["c_pitch"], d["cr_offset"], keep=host)

    want_rgba = want_images(frame, case, conv)
    ctx = _lean(gpu, case, focus, _inverse(want_rgba))
    layout = ctx.derived_layout()
    was = ctx.download_derived()
    # device memory that ends before the frame does: another context's own grid (16 KiB) under a descriptor whose rows are 1 MiB apart
    other = gpu.Context(0)
    other.set_grid(1, 1, 64, 64)
    big = 1 << 20
    early = desc(memory=sref.DEVICE, base=other.grid_device_ptr()[0], y_pitch=big, c_offset=mh * big, c_pitch=big,
                 cr_offset=0 if fmt == sref.NV12 else mh * big + (mh // 2) * big)
    assert early.check(mw, mh, 1)
    before = ctx.memory_info().workspace_bytes
    lib = ctx._lib
    raw = lambda m, g0, mat, rng, chroma, d: lib.lfi_upload_mosaic_yuv_derived(ctx._h, C.byref(m) if m is not None else None, g0, mat, rng, chroma,
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
        ("a frame too wide for 31 bits", (L.Mosaic(1 << 29, 1, 0, 6, 0, 0), 0, 0, 0, 0, good), "31 bits"),
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
        assert ctx.memory_info().workspace_bytes == before, what
        assert (ctx.download_derived() == was).all(), what
    # the calls beside it keep their refusals
    assert lib.lfi_upload_mosaic_yuv(ctx._h, C.byref(good_mosaic), 0, 0, 0, 0, C.byref(good)) == -1 and "released" in lib.lfi_last_error(ctx._h).decode()
    tile_lay = sref.pitched(fmt, w, h)
    tile_host = np.zeros((6, tile_lay.frame_stride), np.uint8)
    deep_tiles = L.YuvSurfaces.make(fmt | L.LFI_YUV_10BIT, sref.HOST, tile_host.ctypes.data, tile_lay.frame_stride, 2 * tile_lay.y_pitch, 2 * tile_lay.c_offset,
                                    2 * tile_lay.c_pitch, 2 * tile_lay.cr_offset, keep=tile_host)
    assert lib.lfi_upload_images_yuv_derived(ctx._h, 0, 1, 0, 0, 0, C.byref(deep_tiles)) == -1
    assert ctx.memory_info().workspace_bytes == before and (ctx.download_derived() == was).all()
    # … and the context goes on
    ctx.upload_mosaic_yuv_derived(good_mosaic, good)
    assert (ctx.download_derived() == restatement(frame, case, conv, layout, layout.phases)).all()
    ctx.close()
    other.close()
    # an odd image size
    for ow, oh in ((5, 4), (10, 3)):
        odd_case = (tiles_x, tiles_y, ow, oh, "grid", False, 0, 6, 0)
        odd = _lean(gpu, odd_case, focus, np.zeros((6, oh, ow, 4), np.uint8))
        assert odd._lib.lfi_upload_mosaic_yuv_derived(odd._h, C.byref(good_mosaic), 0, 0, 0, 0, C.byref(good)) == -1
        assert "even" in odd._lib.lfi_last_error(odd._h).decode()
        odd.close()
    # no grid
    fresh = gpu.Context(0)
    assert fresh._lib.lfi_upload_mosaic_yuv_derived(fresh._h, C.byref(good_mosaic), 0, 0, 0, 0, C.byref(good)) == -1
    assert "lfi_set_grid" in fresh._lib.lfi_last_error(fresh._h).decode()
    fresh.close()
    # a row window: lfi_set_row_window gives a lean context its RGBA planes back, so the window comes first; where such a context can
    # release its inputs at all, the call names the window
    win = gpu.Context(0)
    win.set_grid(tiles_x, tiles_y, w, h)
    win.set_row_window(1, 3, 0, 4)
    try:
        win.fill_synthetic(11)
        win.set_params(params(case, focus))
        win.release_inputs()
        lean_window = True
    except L.LfiError:
        lean_window = False
    assert win._lib.lfi_upload_mosaic_yuv_derived(win._h, C.byref(good_mosaic), 0, 0, 0, 0, C.byref(good)) == -1
    message = win._lib.lfi_last_error(win._h).decode()
    assert ("row window" in message) if lean_window else ("lfi_release_inputs" in message), message
    win.close()
    # a context that still holds its RGBA planes: refused in these words, and its copy (current after a render that reads it) stays what it was
    kept = gpu.Context(0)
    kept.set_grid(tiles_x, tiles_y, w, h)
    kept.upload_grid(_inverse(want_rgba))
    kept.set_params(params(case, focus))
    poison.render(kept, "TEN_WM")
    kept_was = kept.download_derived()
    before = kept.memory_info().workspace_bytes
    assert kept._lib.lfi_upload_mosaic_yuv_derived(kept._h, C.byref(good_mosaic), 0, 0, 0, 0, C.byref(good)) == -1
    message = kept._lib.lfi_last_error(kept._h).decode()
    assert "RGBA inputs" in message and "lfi_release_inputs" in message and "released" not in message, message
    assert kept.memory_info().workspace_bytes == before and (kept.download_derived() == kept_was).all()
    kept.release_inputs()
    kept.upload_mosaic_yuv_derived(good_mosaic, good)   # … and after the release it is served
    lay2 = kept.derived_layout()
    assert (kept.download_derived() == restatement(frame, case, conv, lay2, lay2.phases)).all()
    kept.close()
