"""GPU (-m gpu): lfi_upload_images_yuv_derived (csrc/hip/yuv_derived.hpp) — YUV 4:2:0 frames expanded straight into the derived planar copy of
a context whose RGBA inputs were released.

Everything is integers, so every comparison is `==` on all bytes: the whole copy, padding included, against tests/derived_ref.py over the RGBA
of tests/yuv_in_ref.py, and against a twin context that took the same frames through lfi_upload_images_yuv before its release; renders
against the twin's and the CPU oracle's.  Before every call the copy holds the target's images with every colour byte XOR 0x80, so no byte of
it — image or padding — can be left unwritten and pass."""
import ctypes as C

import numpy as np
import pytest

import lfinterpolator_amd as L
import derived_ref
import poison
import yuv_in_ref as in_ref
import yuv_surfaces_ref as sref
from test_gpu_yuv_surfaces import _Surfaces, _bad_descriptors, _frames

pytestmark = pytest.mark.gpu

SPAN = L.LFI_YUV_DERIVED_SPAN   # bytes (= pixels) of a plane row per workgroup of the kernel
VIEWS = 4
# (cols, rows, W, H, focus).  20 frames: two staged chunks, W % 8 = 2, odd cw and odd H; W < 8 and one row; two (as the issue has it) and
# three images a span + 10 wide: a span boundary inside the image and a block both neighbours compute, whatever the span.  The focus of each:
# the integer x offsets -D[g] are what padx + phase[g] is congruent to mod 128 (checked on the CPU below, from derived_layout() on the GPU)
SHAPES = [(5, 4, 18, 5, 0.9), (3, 1, 7, 1, 1.3), (2, 1, SPAN + 10, 3, 0.23), (3, 1, SPAN + 10, 3, 0.1)]
SHAPE_IDS = [f"{c}x{r}_{w}x{h}" for c, r, w, h, _ in SHAPES]
FORMATS = {"i420": sref.I420, "nv12": sref.NV12}
# source: (memory, layout, bytes into the allocation)
SOURCES = {"host_tight": (sref.HOST, sref.tight, 0), "host_pitched": (sref.HOST, sref.pitched, 0),
           "device_in_place": (sref.DEVICE, sref.pitched, 0), "device_off_alignment": (sref.DEVICE, sref.tight, 1)}
CONVERSIONS = {"bilinear": (in_ref.BT709, in_ref.LIMITED, in_ref.BILINEAR), "nearest": (in_ref.BT709, in_ref.LIMITED, in_ref.NEAREST),
               "601_full": (in_ref.BT601, in_ref.FULL, in_ref.BILINEAR)}


def params(shape):
    cols, rows, w, h, focus = shape
    return L.build_params(cols, rows, w, h, "0,0,1,1", focus, 0.0, 3.0, 1.0, VIEWS)


def firsts_are_varied(firsts):
    """padx + phase[g] over the images: both parities and at least three residues mod 4 — all that two images can show is two residues"""
    firsts = np.asarray(firsts)
    if firsts.size < 3:
        return len(set(firsts % 4)) == 2
    return len(set(firsts % 2)) == 2 and len(set(firsts % 4)) >= 3


def _lean(gpu, shape, images):
    """a context of this shape whose copy was built from `images` and whose RGBA planes were released"""
    cols, rows, w, h, _ = shape
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, w, h)
    ctx.upload_grid(images)
    ctx.set_params(params(shape))
    ctx.release_inputs()
    return ctx


_twins = {}


def _twin(gpu, shape, conv):
    """(frames, want_rgba, layout, planes, {method: views}) of a context that took the frames through lfi_upload_images_yuv BEFORE its
    release; computed once per shape and conversion"""
    key = (shape, conv)
    if key not in _twins:
        cols, rows, w, h, _ = shape
        n = cols * rows
        frames = _frames(w, h, n, seed=11)
        ctx = gpu.Context(0)
        ctx.set_grid(cols, rows, w, h)
        ctx.upload_images_yuv(ctx.yuv_surfaces_packed("i420", "host", frames.ctypes.data, keep=frames), n, matrix=conv[0], range=conv[1], chroma=conv[2])
        ctx.set_params(params(shape))
        ctx.release_inputs()
        lay, planes = ctx.derived_layout(), ctx.download_derived()
        views = {}
        for method in ("TEN_WM", "STD"):
            poison.render(ctx, method)
            views[method] = ctx.download_views()
        ctx.close()
        _twins[key] = (frames, in_ref.images(frames, w, h, *conv), lay, planes, views)
    return _twins[key]


def _inverse(rgba):
    out = rgba.copy()
    out[..., :3] ^= 0x80
    return out


# ---- 1: every byte ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("conv", CONVERSIONS, ids=list(CONVERSIONS))
@pytest.mark.parametrize("source", SOURCES, ids=list(SOURCES))
@pytest.mark.parametrize("fmt", FORMATS, ids=list(FORMATS))
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_every_byte_of_the_copy(shape, fmt, source, conv, gpu):
    cols, rows, w, h, _ = shape
    n = cols * rows
    conv = CONVERSIONS[conv]
    memory, layout_of, shift = SOURCES[source]
    frames, want_rgba, twin_lay, twin_planes, _ = _twin(gpu, shape, conv)
    inverse = _inverse(want_rgba)
    ctx = _lean(gpu, shape, inverse)
    lay = ctx.derived_layout()
    assert lay == twin_lay, "the two contexts laid their copies out differently"
    assert firsts_are_varied(lay.padx + lay.phases) and (lay.rows, lay.n) == (h, n) and lay.pitch_bytes % 128 == 0
    want = derived_ref.planes(want_rgba, lay, lay.phases)
    assert (twin_planes == want).all()   # the path from before: yuvs_expand, then planar_build
    assert (ctx.download_derived() == derived_ref.planes(inverse, lay, lay.phases)).all()
    assert (ctx.download_derived() != want).all()
    surface_layout = layout_of(FORMATS[fmt], w, h)
    for byte in (0x00, 0xFF):
        if byte:
            for g in range(n):
                ctx.upload_image(g, inverse[g])   # through the one-image staging plane and planar_build: every byte differs again
        content = sref.scatter(frames, surface_layout, byte)
        surfaces = _Surfaces(ctx, surface_layout, memory, content, shift=shift)
        ctx.poison(L.LFI_POISON_SCRATCH, byte ^ 0x5A)
        before = ctx.memory_info().workspace_bytes
        ctx.upload_images_yuv_derived(surfaces.desc, n, matrix=conv[0], range=conv[1], chroma=conv[2])
        got = ctx.download_derived()
        assert (got == want).all(), (byte, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
        assert (surfaces.read() == content).all(), "the source surfaces were written"
        if source == "device_in_place":
            assert ctx.memory_info().workspace_bytes == before   # read in place: no staging buffer
        assert ctx.derived_layout() == lay
    ctx.close()


# ---- 2: a subset --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("source", ["host_pitched", "device_in_place"])
def test_a_subset_rewrites_its_own_images_only(source, gpu):
    shape = SHAPES[0]
    cols, rows, w, h, _ = shape
    conv = CONVERSIONS["bilinear"]
    memory, layout_of, shift = SOURCES[source]
    frames, want_rgba, _, _, _ = _twin(gpu, shape, conv)
    inverse = _inverse(want_rgba)
    ctx = _lean(gpu, shape, inverse)
    lay = ctx.derived_layout()
    was = ctx.download_derived()
    surface_layout = layout_of(sref.NV12, w, h)
    surfaces = _Surfaces(ctx, surface_layout, memory, sref.scatter(frames[:2], surface_layout, 0xFF), shift=shift)
    ctx.upload_images_yuv_derived(surfaces.desc, 2, g0=3)
    got = ctx.download_derived()
    mixed = inverse.copy()
    mixed[3:5] = in_ref.images(frames[:2], w, h, *conv)
    assert (got[3:5] == derived_ref.planes(mixed, lay, lay.phases)[3:5]).all()
    assert (got[:3] == was[:3]).all() and (got[5:] == was[5:]).all()
    assert (ctx.download_derived(3, 2) == got[3:5]).all()
    ctx.close()


# ---- 3: renders ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=[SHAPE_IDS[0], SHAPE_IDS[3]])
def test_renders_equal_the_twins_and_the_oracle(shape, gpu, oracle_c):
    cols, rows, w, h, _ = shape
    n = cols * rows
    conv = CONVERSIONS["bilinear"]
    frames, want_rgba, _, _, twin_views = _twin(gpu, shape, conv)
    hp = params(shape)
    assert hp.focused_offsets[:, 0].min() < 0 < hp.focused_offsets[:, 0].max()   # shifts to both sides: both paddings are read
    ctx = _lean(gpu, shape, _inverse(want_rgba))
    poison.render(ctx, "STD")
    assert not (ctx.download_views() == twin_views["STD"]).all()
    surface_layout = sref.pitched(sref.NV12, w, h)
    surfaces = _Surfaces(ctx, surface_layout, sref.DEVICE, sref.scatter(frames, surface_layout, 0xFF))
    ctx.upload_images_yuv_derived(surfaces.desc, n)
    for method in ("TEN_WM", "STD"):
        poison.render(ctx, method)
        assert (ctx.download_views() == twin_views[method]).all(), method
    assert (twin_views["STD"] == oracle_c.blend_std(want_rgba, hp.focused_offsets, hp.offsets, hp.weights)).all()
    ctx.close()


# ---- 4: ordering --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("memory", [sref.HOST, sref.DEVICE], ids=["host", "device"])
def test_renders_are_ordered_around_the_call(memory, gpu):
    """render, call, render without a host wait in between: the render issued before the call shows the old frames, the one behind it the new"""
    shape = SHAPES[0]
    cols, rows, w, h, _ = shape
    n = cols * rows
    conv = CONVERSIONS["bilinear"]
    first, second = _frames(w, h, n, seed=3), _frames(w, h, n, seed=4)
    hp = params(shape)
    rgba = gpu.Context(0)
    rgba.set_grid(cols, rows, w, h)
    rgba.set_params(hp)
    want = []
    for frames in (first, second):
        rgba.upload_grid(in_ref.images(frames, w, h, *conv))
        poison.render(rgba, "STD")
        want.append(rgba.download_views())
    rgba.close()
    assert not (want[0] == want[1]).all()
    lean = _lean(gpu, shape, in_ref.images(second, w, h, *conv))
    lay = sref.pitched(sref.NV12, w, h)
    surfaces = [_Surfaces(lean, lay, memory, sref.scatter(f, lay, 0xFF)) for f in (first, second)]
    for step in (0, 1, 0):
        lean.poison(poison.RENDER, 0xA5)
        lean.upload_images_yuv_derived(surfaces[step].desc, n)
        lean.render("STD")                                               # no host wait in between
        lean.upload_images_yuv_derived(surfaces[1 - step].desc, n)       # … and the next call right behind the render
        lean.sync()
        assert (lean.download_views() == want[step]).all(), step
        poison.render(lean, "STD")
        assert (lean.download_views() == want[1 - step]).all(), step
    lean.close()


# ---- 5: refusals --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS, ids=list(FORMATS))
def test_refusals_leave_the_copy_and_the_staging_buffer(fmt, gpu):
    shape = (3, 1, 18, 5, 1.3)
    cols, rows, w, h, _ = shape
    n = cols * rows
    conv = CONVERSIONS["bilinear"]
    frames = _frames(w, h, n, seed=5)
    lay = sref.pitched(FORMATS[fmt], w, h)
    host = sref.scatter(frames, lay, 0)
    good = sref.descriptor(L, lay, sref.HOST, host.ctypes.data, keep=host)
    want_rgba = in_ref.images(frames, w, h, *conv)
    ctx = _lean(gpu, shape, _inverse(want_rgba))
    layout = ctx.derived_layout()
    was = ctx.download_derived()
    before = ctx.memory_info().workspace_bytes
    lib, raw = ctx._lib, lambda g0, k, m, r, c, d: ctx._lib.lfi_upload_images_yuv_derived(ctx._h, g0, k, m, r, c, C.byref(d) if d is not None else None)
    refused = [(what, (0, n, 0, 0, 0, d), word) for what, d, word in _bad_descriptors(ctx, lay, host)]
    refused += [
        ("n = 0", (0, 0, 0, 0, 0, good), "n >= 1"),
        ("g0 + n beyond the grid", (n - 1, 2, 0, 0, 0, good), "inside"),
        ("g0 below 0", (-1, 2, 0, 0, 0, good), "inside"),
        ("unknown matrix", (0, n, 2, 0, 0, good), "matrix"),
        ("unknown range", (0, n, 0, 2, 0, good), "range"),
        ("unknown chroma", (0, n, 0, 0, 2, good), "chroma"),
    ]
    for what, args, word in refused:
        assert raw(*args) == -1, what   # LFI_EINVAL
        assert word in lib.lfi_last_error(ctx._h).decode(), (what, lib.lfi_last_error(ctx._h).decode())
        assert ctx.memory_info().workspace_bytes == before, what
    assert (ctx.download_derived() == was).all()
    ctx.upload_images_yuv_derived(good, n)   # … and the context goes on
    assert (ctx.download_derived() == derived_ref.planes(want_rgba, layout, layout.phases)).all()
    ctx.close()
    # no grid
    fresh = gpu.Context(0)
    assert fresh._lib.lfi_upload_images_yuv_derived(fresh._h, 0, 1, 0, 0, 0, C.byref(good)) == -1 and "lfi_set_grid" in fresh._lib.lfi_last_error(fresh._h).decode()
    with pytest.raises(L.LfiError):
        fresh.derived_layout()
    fresh.close()
    # a context that still holds its RGBA planes: refused, and its copy (current after a render that reads it) stays what it was
    kept = gpu.Context(0)
    kept.set_grid(cols, rows, w, h)
    kept.upload_grid(_inverse(want_rgba))
    kept.set_params(params(shape))
    with pytest.raises(L.LfiError):
        kept.download_derived()              # no render has built the copy yet
    poison.render(kept, "TEN_WM")
    views = kept.download_views()
    kept_lay, kept_was = kept.derived_layout(), kept.download_derived()
    assert (kept_was == derived_ref.planes(_inverse(want_rgba), kept_lay, kept_lay.phases)).all()
    before = kept.memory_info().workspace_bytes
    assert kept._lib.lfi_upload_images_yuv_derived(kept._h, 0, n, 0, 0, 0, C.byref(good)) == -1
    assert "lfi_release_inputs" in kept._lib.lfi_last_error(kept._h).decode()
    assert kept.memory_info().workspace_bytes == before and (kept.download_derived() == kept_was).all()
    kept.release_inputs()
    kept.upload_images_yuv_derived(good, n)  # … and after the release it is served
    lay2 = kept.derived_layout()
    assert (kept.download_derived() == derived_ref.planes(want_rgba, lay2, lay2.phases)).all()
    poison.render(kept, "TEN_WM")
    assert not (kept.download_views() == views).all()
    kept.close()
