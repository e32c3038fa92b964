"""GPU (-m gpu): left-sited chroma (lfi_set_yuv_siting) — yuvs_convert_left, yuvs_expand_left (csrc/hip/yuv_surfaces.hpp) and
yuvs_derived_expand_left (csrc/hip/yuv_derived.hpp) behind the calls the setting governs.

Both definitions are integers (include/lfi.h), so every comparison is `==` on all bytes, against tests/yuv_left_ref.py applied to the views'
own downloads and to the frames that were uploaded; tests/yuv_surfaces_ref.py places the bytes.  Every byte the frames do not own holds a
poison: two poisons must give the same grid, and a download must leave every one of them as it was."""
import ctypes as C

import numpy as np
import pytest

import lfinterpolator_amd as L
import derived_ref
import poison
import scaled_quilt_ref
import yuv_in_ref as in_ref
import yuv_left_ref as left
import yuv_ref as out_ref
import yuv_surfaces_ref as sref
from conftest import SEED
from test_gpu_yuv_derived import _inverse, _lean, params as derived_params
from test_gpu_yuv_surfaces import FORMAT_NAMES, FORMATS, V, _Surfaces, _attached, _frames, _read, _rendered, _reset

pytestmark = pytest.mark.gpu

# W x H, where the left-sited kernels can go wrong: the smallest frame; the smallest even one; one whole block; ragged blocks of one and of
# two columns with an odd H; a second workgroup along y; the neighbour's value crosses a 16-lane DPP row at x = 128; the first lane of a
# second wave (x = 512) loads pixel column 511 itself
SIZES = [(1, 1), (2, 2), (8, 2), (17, 5), (18, 5), (24, 10), (130, 4), (520, 6)]
SIZE_IDS = [f"{w}x{h}" for w, h in SIZES]
ALL_FOUR = (18, 5)   # the shape that takes all four coefficient rows; the others take two, rotating


def _rows(size):
    if size == ALL_FOUR:
        return list(out_ref.FORMATS)
    k = SIZES.index(size)
    return [out_ref.FORMATS[k % 4], out_ref.FORMATS[(k + 2) % 4]]


def _layouts(fmt, w, h):
    """host frames: tight (staged); device surfaces: pitches of 256, read and written in place"""
    return [(sref.HOST, "host tight", sref.tight(fmt, w, h)), (sref.DEVICE, "device in place", sref.pitched(fmt, w, h))]


# ---- output ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["rgba", "planar"])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_frames_equal_the_restatement_and_padding_keeps_its_poison(size, layout, gpu):
    w, h = size
    ctx = _rendered(gpu, w, h, layout)
    views = ctx.download_views()
    ctx.set_yuv_siting("centre", "left")
    assert ctx.yuv_siting() == ("centre", "left")
    for conv in _rows(size):
        want = left.frames(views, *conv)
        ctx.poison(L.LFI_POISON_SCRATCH, 0xA5)
        assert (ctx.download_views_yuv420(matrix=conv[0], range=conv[1]) == want).all(), (size, layout, conv)
        for fmt in FORMATS:
            for memory, name, lay in _layouts(fmt, w, h):
                for byte in poison.POISON:
                    dst = _Surfaces(ctx, lay, memory, np.full((V, lay.frame_stride), byte, np.uint8))
                    ctx.poison(L.LFI_POISON_SCRATCH, byte ^ 0xFF)
                    ctx.download_views_yuv(dst.desc, matrix=conv[0], range=conv[1])
                    got = dst.read()
                    what = (size, layout, conv, FORMAT_NAMES[fmt], name, byte)
                    assert (sref.gather(got, lay) == want).all(), what
                    assert sref.padding_holds(got, lay, byte), what
    assert (ctx.download_views() == views).all()   # the call writes no view
    ctx.close()


def test_random_attached_views(gpu):
    """views of random bytes in attached memory, 520 x 6 and 130 x 4: every column's neighbour differs from it, in both view layouts"""
    from test_gpu_yuv import _attached as attached_views
    for w, h in ((520, 6), (130, 4)):
        content = np.random.default_rng(w).integers(0, 256, (3, h, w, 4), dtype=np.uint8)
        content[..., 3] = 255
        for layout in ("rgba", "planar"):
            ctx, buf = attached_views(gpu, w, h, layout, content)
            ctx.set_yuv_siting("centre", "left")
            for conv in (out_ref.FORMATS[1], out_ref.FORMATS[2]):
                got = ctx.download_views_yuv420(matrix=conv[0], range=conv[1])
                assert (got == left.frames(content, *conv)).all(), (w, h, layout, conv)
            ctx.close()
            del buf


# ---- input ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_NAMES.get)
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_grid_equals_the_restatement(size, fmt, gpu):
    """random chroma and, as the last frame, the extremes; host frames (staged) and device surfaces in place, the padding poisoned with 0x00
    and then with 0xFF; NEAREST under left siting is NEAREST"""
    w, h = size
    n = 2
    frames = _frames(w, h, n, seed=7)
    ctx, grid = _attached(gpu, n, 1, w, h)
    ctx.set_yuv_siting("left", "centre")
    conversions = [(*row, in_ref.BILINEAR) for row in _rows(size)] + [(in_ref.BT709, in_ref.LIMITED, in_ref.NEAREST)]
    for conv in conversions:
        want = left.images(frames, w, h, *conv)
        if conv[2] == in_ref.NEAREST:
            assert (want == in_ref.images(frames, w, h, *conv)).all()
        _reset(grid)
        ctx.upload_images_yuv420(frames, matrix=conv[0], range=conv[1], chroma=conv[2])
        assert (_read(ctx, grid) == want).all(), (size, conv)
        for memory, name, lay in _layouts(fmt, w, h):
            for byte in (0x00, 0xFF):
                content = sref.scatter(frames, lay, byte)
                surfaces = _Surfaces(ctx, lay, memory, content)
                _reset(grid)
                ctx.poison(L.LFI_POISON_SCRATCH, byte ^ 0x5A)
                ctx.upload_images_yuv(surfaces.desc, n, matrix=conv[0], range=conv[1], chroma=conv[2])
                got = _read(ctx, grid)
                assert (got == want).all(), (size, FORMAT_NAMES[fmt], name, conv, byte, int((got != want).sum()))
                assert (surfaces.read() == content).all(), "the source surfaces were written"
    ctx.close()
    del grid


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_NAMES.get)
@pytest.mark.parametrize("shape", [(5, 4, 18, 5, 0.9), (2, 1, 520, 6, 0.23)], ids=["5x4_18x5", "2x1_520x6"])
def test_derived_upload_equals_upload_and_rebuild(shape, fmt, gpu):
    """lfi_upload_images_yuv_derived under left siting: every byte of the planar copy, padding included, is what a twin context holds that
    took the frames left-sited through lfi_upload_images_yuv before its release — and what tests/derived_ref.py makes of the restated images"""
    cols, rows, w, h, _ = shape
    n = cols * rows
    conv = (in_ref.BT601, in_ref.LIMITED, in_ref.BILINEAR)
    frames = _frames(w, h, n, seed=13)
    twin = gpu.Context(0)
    twin.set_grid(cols, rows, w, h)
    twin.set_yuv_siting("left", "centre")
    twin.upload_images_yuv(twin.yuv_surfaces_packed("i420", "host", frames.ctypes.data, keep=frames), n, matrix=conv[0], range=conv[1], chroma=conv[2])
    twin.set_params(derived_params(shape))
    twin.release_inputs()
    twin_lay, twin_planes = twin.derived_layout(), twin.download_derived()
    twin.close()
    want_rgba = left.images(frames, w, h, *conv)
    ctx = _lean(gpu, shape, _inverse(want_rgba))
    lay = ctx.derived_layout()
    assert lay == twin_lay
    want = derived_ref.planes(want_rgba, lay, lay.phases)
    assert (twin_planes == want).all()
    assert (ctx.download_derived() != want).all()
    ctx.set_yuv_siting("left", "centre")
    for memory, name, surface_layout in _layouts(fmt, w, h):
        for g in range(n):
            ctx.upload_image(g, _inverse(want_rgba)[g])
        content = sref.scatter(frames, surface_layout, 0xFF if memory == sref.HOST else 0x00)
        surfaces = _Surfaces(ctx, surface_layout, memory, content)
        ctx.upload_images_yuv_derived(surfaces.desc, n, matrix=conv[0], range=conv[1], chroma=conv[2])
        got = ctx.download_derived()
        assert (got == want).all(), (name, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
        assert (surfaces.read() == content).all()
    # NEAREST under left siting is the nearest kernel's copy
    want_nearest = derived_ref.planes(in_ref.images(frames, w, h, conv[0], conv[1], in_ref.NEAREST), lay, lay.phases)
    ctx.upload_images_yuv_derived(surfaces.desc, n, matrix=conv[0], range=conv[1], chroma=in_ref.NEAREST)
    assert (ctx.download_derived() == want_nearest).all()
    ctx.close()


# ---- the stream and the quilt ---------------------------------------------------------------------------------------------------------------------

def test_stream_of_six_views_in_blocks_of_four(gpu):
    w, h, block, total = 18, 5, 4, 6
    fb = out_ref.sizes(w, h)[2]
    hp_all = gpu.build_params(3, 3, w, h, "0,0,1,1", 0.2, 0.0, 3.0, 1.0, total)
    ctx = gpu.Context(0)
    ctx.set_grid(3, 3, w, h)
    ctx.fill_synthetic(SEED)
    views = np.zeros((total, h, w, 4), np.uint8)
    for b in range(0, total, block):
        hp = hp_all.rows(b, min(b + block, total))
        ctx.set_params(hp)
        poison.render(ctx, "STD")
        views[b:b + hp.weights.shape[0]] = ctx.download_views()
    ctx.set_params(hp_all.rows(0, block))
    ctx.set_yuv_siting("centre", "left")
    for conv in (out_ref.FORMATS[0], out_ref.FORMATS[3]):
        ctx.poison(poison.RENDER, 0xA5)
        out = ctx.pinned_empty((total, fb + 8))
        out[...] = poison.SENTINEL
        got = ctx.render_stream_yuv420("STD", hp_all.weights, out=out, matrix=conv[0], range=conv[1])
        assert (got == left.frames(views, *conv)).all(), conv
        assert (out[:, fb:] == poison.SENTINEL).all()
    ctx.close()


@pytest.mark.parametrize("layout", ["rgba", "planar"])
@pytest.mark.parametrize("quilt", [(4, 2, 18, 10), (3, 3, 17, 9)], ids=["even-18x10", "odd-17x9"])
def test_quilt_frame_is_the_left_sited_frame_of_the_scaled_quilt(quilt, layout, gpu):
    """the definition: lfi_download_quilt_scaled's image taken as one view — chroma filters across tile edges.  Even tile sizes take the
    two-launch route too: the quilt buffer is reserved (the fused centre-sited kernel needs none)"""
    from test_gpu_quilt_yuv import _frame, _rendered as rendered_quilt
    tx, ty, tw, th = quilt
    ctx = rendered_quilt(gpu, layout)
    views = ctx.download_views()
    scaled = ctx.download_quilt_scaled(tx, ty, tw, th)
    assert (scaled == scaled_quilt_ref.quilt(views, tx, ty, tw, th)).all()
    fresh = rendered_quilt(gpu, layout)          # a context whose quilt buffer has not been reserved yet
    fresh.set_yuv_siting("centre", "left")
    before = fresh.memory_info().workspace_bytes
    for fmt in FORMATS:
        for memory, name, lay in _layouts(fmt, tx * tw, ty * th):
            for conv in (out_ref.FORMATS[0], out_ref.FORMATS[3]):
                for byte in (0x00, 0xFF):
                    got = _frame(fresh, tx, ty, tw, th, conv, lay, memory, byte)
                    assert (got == left.frame(scaled, *conv)).all(), (quilt, layout, FORMAT_NAMES[fmt], name, conv, byte)
    assert fresh.memory_info().workspace_bytes >= before + tx * tw * ty * th * 4   # quilt_scale's RGBA quilt, for even tiles too
    # left-sited differs from centre-sited here, and the centre-sited call is what it was
    fresh.set_yuv_siting("centre", "centre")
    lay = sref.tight(sref.I420, tx * tw, ty * th)
    centre = _frame(fresh, tx, ty, tw, th, out_ref.FORMATS[0], lay, sref.HOST, 0x00)
    assert (centre == out_ref.frame(scaled, *out_ref.FORMATS[0])).all() and not (centre == left.frame(scaled, *out_ref.FORMATS[0])).all()
    ctx.close()
    fresh.close()


# ---- the setting ----------------------------------------------------------------------------------------------------------------------------------

def test_setting_and_refusals(gpu):
    w, h = 18, 6
    ctx = _rendered(gpu, w, h, "rgba")
    lib = ctx._lib
    assert ctx.yuv_siting() == ("centre", "centre")
    ctx.set_yuv_siting("left", "centre")
    for bad in ((2, 0), (0, 2), (-1, 0), (1, -1), (7, 7)):
        assert lib.lfi_set_yuv_siting(ctx._h, *bad) == -1, bad
        assert "siting" in lib.lfi_last_error(ctx._h).decode()
        assert ctx.yuv_siting() == ("left", "centre"), bad                       # the setting is kept
    a = C.c_int(5)
    assert lib.lfi_yuv_siting(ctx._h, None, C.byref(a)) == -1 and lib.lfi_yuv_siting(ctx._h, C.byref(a), None) == -1 and a.value == 5
    with pytest.raises(L.LfiError, match="siting"):
        ctx.set_yuv_siting(3, "left")
    # RGB-D under left output is refused before anything is written, and the context goes on
    ctx.set_yuv_siting("centre", "left")
    lay = sref.tight(sref.I420, 2 * w, h)
    host = poison.sentinel((1, lay.frame_stride))
    desc = sref.descriptor(L, lay, sref.HOST, host.ctypes.data, keep=host)
    before = ctx.memory_info().workspace_bytes
    assert lib.lfi_download_rgbd_yuv(ctx._h, 0, 1, 0, 0, w, h, 0, 0, C.byref(desc)) == -1
    assert "left" in lib.lfi_last_error(ctx._h).decode() and "lfi_download_rgbd_yuv" in lib.lfi_last_error(ctx._h).decode()
    assert (host == poison.SENTINEL).all() and ctx.memory_info().workspace_bytes == before
    views = ctx.download_views()
    assert (ctx.download_views_yuv420() == left.frames(views, out_ref.BT709, out_ref.LIMITED)).all()
    # … and under centre output it is served as before: a map, then the frame
    ctx.set_yuv_siting("left", "centre")
    ctx.upload_map(0, np.full((h, w, 4), 200, np.uint8))
    ctx.download_rgbd_yuv(0, 1, 0, 0, w, h, 0, 0, desc)
    assert (host[0, :2 * w * h].reshape(h, 2 * w)[:, :w] == out_ref.planes(views[0], 0, 0)[0]).all()
    # the setting survives lfi_set_params and lfi_set_grid
    ctx.set_yuv_siting("left", "left")
    ctx.set_params(gpu.build_params(3, 3, w, h, "0,0,1,1", 0.3, 0.0, 3.0, 1.0, V))
    assert ctx.yuv_siting() == ("left", "left")
    ctx.set_grid(2, 1, w, h)
    assert ctx.yuv_siting() == ("left", "left")
    ctx.close()


def test_back_to_centre_is_a_fresh_context(gpu):
    """after left/left and back, both directions give the bytes of a context that never heard of the setting"""
    w, h = 18, 5
    frames = _frames(w, h, 2, seed=21)
    switched, fresh = _rendered(gpu, w, h, "planar"), _rendered(gpu, w, h, "planar")
    switched.set_yuv_siting("left", "left")
    left_out = switched.download_views_yuv420()
    switched.set_yuv_siting("centre", "centre")
    views = fresh.download_views()
    assert (switched.download_views() == views).all()
    want = out_ref.frames(views, out_ref.BT709, out_ref.LIMITED)
    assert (fresh.download_views_yuv420() == want).all() and (switched.download_views_yuv420() == want).all()
    assert (left_out == left.frames(views, out_ref.BT709, out_ref.LIMITED)).all() and not (left_out == want).all()
    switched.close()
    fresh.close()
    grids = []
    for visit_left in (True, False):
        ctx, grid = _attached(gpu, 2, 1, w, h)
        if visit_left:
            ctx.set_yuv_siting("left", "left")
            ctx.upload_images_yuv420(frames)
            assert (_read(ctx, grid) == left.images(frames, w, h, in_ref.BT709, in_ref.LIMITED)).all()
            ctx.set_yuv_siting("centre", "centre")
            _reset(grid)
        ctx.upload_images_yuv420(frames)
        grids.append(_read(ctx, grid).copy())
        ctx.close()
        del grid
    assert (grids[0] == grids[1]).all() and (grids[0] == in_ref.images(frames, w, h, in_ref.BT709, in_ref.LIMITED)).all()
