"""GPU (-m gpu): video surfaces — lfi_upload_images_yuv and lfi_download_views_yuv (csrc/hip/yuv_surfaces.hpp): I420 and NV12, tight and
pitched, in host memory and in device memory (read and written in place where everything is a multiple of 16, staged otherwise).

The conversions are defined in integers (include/lfi.h), so every comparison is `==` on all bytes, against tests/yuv_in_ref.py and
tests/yuv_ref.py as they are; tests/yuv_surfaces_ref.py only places the bytes.  Every byte the frames do not own holds a poison: two poisons
must give the same grid, and a download must leave every one of them as it was."""
import ctypes as C

import numpy as np
import pytest

import lfinterpolator_amd as L
import poison
import yuv_in_ref as in_ref
import yuv_ref as out_ref
import yuv_surfaces_ref as sref
from conftest import SEED, SMALL_CASES

pytestmark = pytest.mark.gpu

PATTERN = 0x3C   # what the attached grid holds before a call
# W x H, the smallest at which each path can go wrong: one block; ragged and odd with cw = 9; 65 blocks per row (a second workgroup along
# x, chroma neighbours across its boundary); a second workgroup along y
SIZES = [(8, 2), (18, 5), (520, 6), (24, 10)]
FORMATS = [sref.I420, sref.NV12]
MEMORIES = [sref.HOST, sref.DEVICE]
FORMAT_NAMES = {sref.I420: "i420", sref.NV12: "nv12"}
MEMORY_NAMES = {sref.HOST: "host", sref.DEVICE: "device"}


def _layouts(fmt, w, h):
    """tight (device: staged, no pitch here is a multiple of 16) and a decoder's: pitches rounded up to 256, a gap before the chroma (device:
    in place)"""
    return {"tight": sref.tight(fmt, w, h), "pitched": sref.pitched(fmt, w, h)}


def _frames(w, h, n, seed=0):
    """uniformly random bytes in all planes — codes outside the nominal ranges hit both clamps — and, as the last frame, the extremes"""
    frames = np.random.default_rng(seed + w * 1000 + h).integers(0, 256, (n, in_ref.sizes(w, h)[2]), dtype=np.uint8)
    frames[-1] = in_ref.extremes_frame(w, h)
    return frames


def _attached(gpu, cols, rows, w, h):
    """a context whose grid is a torch tensor holding PATTERN"""
    import torch
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, w, h)
    grid = torch.full((cols * rows, h, w, 4), PATTERN, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.attach_grid(grid.data_ptr(), grid.numel())
    return ctx, grid


def _reset(grid):
    import torch
    grid.fill_(PATTERN)
    torch.cuda.synchronize()   # torch's stream and the context's know nothing of each other


def _read(ctx, grid):
    import torch
    ctx.upload_wait()
    ctx.sync()
    torch.cuda.synchronize()
    return grid.cpu().numpy()


class _Surfaces:
    """n frames' worth of surfaces of layout lay in host or device memory, `shift` bytes into their allocation, holding `content`
    ([n][frame_stride])"""

    def __init__(self, ctx, lay, memory, content, shift=0):
        import torch
        self.lay, self.memory, self.n, self.shift = lay, memory, content.shape[0], shift
        flat = np.concatenate([np.full(shift, 0xEE, np.uint8), content.reshape(-1)])
        if memory == sref.DEVICE:
            self.tensor = torch.from_numpy(flat).to("cuda:0")
            torch.cuda.synchronize()   # torch's stream and the context's know nothing of each other
            base = self.tensor.data_ptr() + shift
            assert self.tensor.data_ptr() % 256 == 0
        else:
            self.array = ctx.pinned_empty((flat.size,))
            self.array[...] = flat
            base = self.array.ctypes.data + shift
        self.desc = sref.descriptor(L, lay, memory, base, keep=self)

    def read(self):
        import torch
        if self.memory == sref.DEVICE:
            torch.cuda.synchronize()
            flat = self.tensor.cpu().numpy()
        else:
            flat = np.array(self.array)
        assert (flat[:self.shift] == 0xEE).all()
        return flat[self.shift:].reshape(self.n, self.lay.frame_stride)


# ---- upload -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("memory", MEMORIES, ids=MEMORY_NAMES.get)
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_NAMES.get)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_grid_equals_the_restatement(size, fmt, memory, gpu):
    """{tight, pitched} x {bilinear, nearest} and one non-default matrix/range pair, the padding poisoned with 0x00 and then with 0xFF: the grid
    is the restatement's, byte for byte, and lfi_upload_images_yuv420's; the surfaces are unchanged afterwards"""
    w, h = size
    n = 2
    frames = _frames(w, h, n)
    ctx, grid = _attached(gpu, n, 1, w, h)
    conversions = [(in_ref.BT709, in_ref.LIMITED, in_ref.BILINEAR), (in_ref.BT709, in_ref.LIMITED, in_ref.NEAREST), (in_ref.BT601, in_ref.FULL, in_ref.BILINEAR)]
    for conv in conversions:
        want = in_ref.images(frames, w, h, *conv)
        _reset(grid)
        ctx.upload_images_yuv420(frames, matrix=conv[0], range=conv[1], chroma=conv[2])
        assert (_read(ctx, grid) == want).all()   # the entry point from before, from the de-interleaved frames
        for name, lay in _layouts(fmt, w, h).items():
            for byte in (0x00, 0xFF):
                content = sref.scatter(frames, lay, byte)
                surfaces = _Surfaces(ctx, lay, memory, content)
                _reset(grid)
                ctx.poison(L.LFI_POISON_SCRATCH, byte ^ 0x5A)
                before = ctx.memory_info().workspace_bytes
                ctx.upload_images_yuv(surfaces.desc, n, matrix=conv[0], range=conv[1], chroma=conv[2])
                got = _read(ctx, grid)
                assert (got == want).all(), (size, FORMAT_NAMES[fmt], MEMORY_NAMES[memory], name, conv, byte, int((got != want).sum()))
                assert (surfaces.read() == content).all(), "the source surfaces were written"
                if memory == sref.DEVICE and name == "pitched":
                    assert ctx.memory_info().workspace_bytes == before   # read in place: no staging buffer
    ctx.close()
    del grid


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_NAMES.get)
def test_eighteen_frames_take_two_chunks_from_the_host_and_one_launch_in_place(fmt, gpu):
    w, h = 18, 5
    n = 18
    padded = 24 * 6 + 2 * 12 * 3   # the staged frame: Y pitch 24, 6 rows; chroma 3 rows of 2 x 12 bytes
    frames = _frames(w, h, n, seed=1)
    want = in_ref.images(frames, w, h, in_ref.BT709, in_ref.LIMITED)
    lay = sref.pitched(fmt, w, h)
    content = sref.scatter(frames, lay, 0x5A)
    # device, in place: no staging buffer at all
    ctx, grid = _attached(gpu, 6, 3, w, h)
    before = ctx.memory_info().workspace_bytes
    dev = _Surfaces(ctx, lay, sref.DEVICE, content)
    ctx.upload_images_yuv(dev.desc, n)
    assert (_read(ctx, grid) == want).all()
    assert ctx.memory_info().workspace_bytes == before
    # host: chunks of 16 + 2 through a buffer of 16 staged frames
    _reset(grid)
    host = _Surfaces(ctx, lay, sref.HOST, content)
    ctx.upload_images_yuv(host.desc, n)
    assert (_read(ctx, grid) == want).all()
    assert ctx.memory_info().workspace_bytes == before + 16 * padded
    assert (host.read() == content).all() and (dev.read() == content).all()
    # a range of images: the others keep the pattern
    _reset(grid)
    ctx.upload_images_yuv(dev.desc, 5, g0=7, matrix="601", range="full", chroma="nearest")
    got = _read(ctx, grid)
    assert (got[7:12] == in_ref.images(frames[:5], w, h, in_ref.BT601, in_ref.FULL, in_ref.NEAREST)).all()
    assert (got[:7] == PATTERN).all() and (got[12:] == PATTERN).all()
    ctx.close()
    del grid


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_NAMES.get)
def test_a_device_surface_off_alignment_is_staged(fmt, gpu):
    """base + 1 with pitch = W: device-to-device 2D copies into the staging planes"""
    w, h = 18, 5
    n = 3
    frames = _frames(w, h, n, seed=2)
    lay = sref.tight(fmt, w, h)
    ctx, grid = _attached(gpu, n, 1, w, h)
    before = ctx.memory_info().workspace_bytes
    content = sref.scatter(frames, lay, 0)
    dev = _Surfaces(ctx, lay, sref.DEVICE, content, shift=1)
    ctx.poison(L.LFI_POISON_SCRATCH, 0xFF)
    ctx.upload_images_yuv(dev.desc, n)
    assert (_read(ctx, grid) == in_ref.images(frames, w, h, in_ref.BT709, in_ref.LIMITED)).all()
    assert ctx.memory_info().workspace_bytes == before + n * (24 * 6 + 2 * 12 * 3)
    assert (dev.read() == content).all()
    ctx.close()
    del grid


@pytest.mark.parametrize("memory", MEMORIES, ids=MEMORY_NAMES.get)
def test_renders_are_ordered_around_an_upload(memory, gpu):
    """own planes, the g3x3_16x16_v8 golden's grid and parameters, NV12 pitched surfaces: a render issued right after an upload, without a host
    wait, equals the render from the restatement's RGBA; a render issued before the upload is untouched by it"""
    name, cols, rows, w, h, views, trajectory, focus, aspect, effect = SMALL_CASES[0]
    hp = gpu.build_params(cols, rows, w, h, trajectory, focus, 0.0, effect, aspect, views)
    n = cols * rows
    conv = (in_ref.BT709, in_ref.LIMITED, in_ref.BILINEAR)
    first, second = _frames(w, h, n, seed=3), _frames(w, h, n, seed=4)
    yuv, rgba = gpu.Context(0), gpu.Context(0)
    for ctx in (yuv, rgba):
        ctx.set_grid(cols, rows, w, h)
        ctx.fill_synthetic(SEED)
        ctx.set_params(hp)
    lay = sref.pitched(sref.NV12, w, h)
    surfaces = [_Surfaces(yuv, lay, memory, sref.scatter(f, lay, 0xFF)) for f in (first, second)]
    want = []
    for frames in (first, second):
        rgba.upload_grid(in_ref.images(frames, w, h, *conv))
        poison.render(rgba, "STD")
        want.append(rgba.download_views())
    assert not (want[0] == want[1]).all()
    for step in (0, 1, 0):
        yuv.poison(poison.RENDER, 0xA5)
        yuv.upload_images_yuv(surfaces[step].desc, n)
        yuv.render("STD")                                       # no host wait in between
        yuv.upload_images_yuv(surfaces[1 - step].desc, n)       # … and the next upload right behind the render
        yuv.sync()
        assert (yuv.download_views() == want[step]).all(), step
        poison.render(yuv, "STD")
        assert (yuv.download_views() == want[1 - step]).all(), step
    yuv.close()
    rgba.close()


# ---- download -----------------------------------------------------------------------------------------------------------------------------------

V = 3


def _rendered(gpu, w, h, layout):
    hp = gpu.build_params(3, 3, w, h, "0,0,1,1", 0.2, 0.0, 3.0, 1.0, V)
    ctx = gpu.Context(0)
    ctx.set_grid(3, 3, w, h)
    ctx.fill_synthetic(SEED)
    ctx.set_params(hp)
    ctx.set_output_layout(layout)
    poison.render(ctx, "STD")
    return ctx


@pytest.mark.parametrize("layout", ["rgba", "planar"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frames_equal_the_restatement_and_padding_keeps_its_poison(size, layout, gpu):
    w, h = size
    ctx = _rendered(gpu, w, h, layout)
    views = ctx.download_views()
    for conv in ((out_ref.BT709, out_ref.LIMITED), (out_ref.BT601, out_ref.FULL)):
        want = out_ref.frames(views, *conv)
        i420 = ctx.download_views_yuv420(matrix=conv[0], range=conv[1])
        assert (i420 == want).all()
        for fmt in FORMATS:
            for memory in MEMORIES:
                cases = [(name, lay, 0) for name, lay in _layouts(fmt, w, h).items()]
                if memory == sref.DEVICE:
                    cases.append(("tight at base + 1", sref.tight(fmt, w, h), 1))
                for name, lay, shift in cases:
                    for byte in poison.POISON:
                        dst = _Surfaces(ctx, lay, memory, np.full((V, lay.frame_stride), byte, np.uint8), shift=shift)
                        ctx.poison(L.LFI_POISON_SCRATCH, byte ^ 0xFF)
                        ctx.download_views_yuv(dst.desc, matrix=conv[0], range=conv[1])
                        got = dst.read()
                        what = (size, layout, conv, FORMAT_NAMES[fmt], MEMORY_NAMES[memory], name, byte)
                        assert (sref.gather(got, lay) == want).all(), what       # NV12 de-interleaved IS lfi_download_views_yuv420's output
                        assert sref.padding_holds(got, lay, byte), what
                    # a sub-range: views [1, 3) into frames 0 and 1, frame 2 untouched
                    dst = _Surfaces(ctx, lay, memory, np.full((V, lay.frame_stride), 0x11, np.uint8), shift=shift)
                    ctx.download_views_yuv(dst.desc, n=2, v0=1, matrix=conv[0], range=conv[1])
                    got = dst.read()
                    assert (sref.gather(got[:2], lay) == want[1:]).all() and sref.padding_holds(got[:2], lay, 0x11) and (got[2] == 0x11).all()
    assert (ctx.download_views() == views).all()   # the call writes no view
    ctx.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------

def _bad_descriptors(ctx, lay, host):
    """(what, descriptor, word of the message): what lfi_yuv_surfaces_check refuses, and pointers that are no device memory"""
    def make(memory=sref.HOST, base=host.ctypes.data, **changes):
        d = dict(fmt=lay.fmt, frame_stride=lay.frame_stride, y_pitch=lay.y_pitch, c_offset=lay.c_offset, c_pitch=lay.c_pitch, cr_offset=lay.cr_offset)
        d.update(changes)
        return L.YuvSurfaces.make(d["fmt"], memory, base, d["frame_stride"], d["y_pitch"], d["c_offset"], d["c_pitch"], d["cr_offset"], keep=host)
    return [
        ("NULL descriptor", None, "NULL"),
        ("NULL base", make(base=None), "NULL"),
        ("unknown format", make(fmt=2), "format"),
        ("unknown memory", make(memory=2), "memory"),
        ("y_pitch below W", make(y_pitch=lay.w - 1), "pitch"),
        ("c_pitch below its minimum", make(c_pitch=(lay.w + 1) // 2 - 1), "pitch"),
        ("chroma inside the Y plane", make(c_offset=lay.h * lay.y_pitch - 1), "overlap"),
        ("Cr inside Cb / cr_offset with NV12", make(cr_offset=lay.c_offset + 1), "cr_offset"),
        ("frame_stride below the extent", make(frame_stride=lay.extent - 1), "frame_stride"),
        ("a host pointer as LFI_MEM_DEVICE", make(memory=sref.DEVICE), "device memory"),
        ("page-locked host memory as LFI_MEM_DEVICE", make(memory=sref.DEVICE, base=ctx.pinned_empty((4 * lay.frame_stride,)).ctypes.data), "device memory"),
    ]


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_NAMES.get)
def test_upload_refusals_leave_the_grid_and_the_staging_buffer(fmt, gpu):
    import torch
    w, h = 18, 5
    n = 3
    frames = _frames(w, h, n, seed=5)
    lay = sref.pitched(fmt, w, h)
    host = sref.scatter(frames, lay, 0)
    ctx, grid = _attached(gpu, n, 1, w, h)
    dev = torch.from_numpy(host.reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    good = sref.descriptor(L, lay, sref.HOST, host.ctypes.data, keep=host)
    before = ctx.memory_info().workspace_bytes
    lib, raw = ctx._lib, lambda g0, k, m, r, c, d: ctx._lib.lfi_upload_images_yuv(ctx._h, g0, k, m, r, c, C.byref(d) if d is not None else None)
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
        assert (_read(ctx, grid) == PATTERN).all(), what
        assert ctx.memory_info().workspace_bytes == before, what
    ctx.upload_images_yuv(good, n)   # … and the context goes on
    assert (_read(ctx, grid) == in_ref.images(frames, w, h, in_ref.BT709, in_ref.LIMITED)).all()
    ctx.close()
    del grid
    # no grid; a row window; released inputs
    fresh = gpu.Context(0)
    assert fresh._lib.lfi_upload_images_yuv(fresh._h, 0, 1, 0, 0, 0, C.byref(good)) == -1 and "lfi_set_grid" in fresh._lib.lfi_last_error(fresh._h).decode()
    fresh.close()
    win = gpu.Context(0)
    win.set_grid(n, 1, w, h)
    win.set_row_window(1, 4, 0, 5)
    assert win._lib.lfi_upload_images_yuv(win._h, 0, n, 0, 0, 0, C.byref(good)) == -1 and "row window" in win._lib.lfi_last_error(win._h).decode()
    win.close()
    hp = gpu.build_params(n, 1, w, h, "0,0,1,1", 0.2, 0.0, 3.0, 1.0, 4)
    rel = gpu.Context(0)
    rel.set_grid(n, 1, w, h)
    rel.fill_synthetic(SEED)
    rel.set_params(hp)
    poison.render(rel, "TEN_WM")
    views = rel.download_views()
    rel.release_inputs()
    assert rel._lib.lfi_upload_images_yuv(rel._h, 0, n, 0, 0, 0, C.byref(good)) == -1 and "released" in rel._lib.lfi_last_error(rel._h).decode()
    poison.render(rel, "TEN_WM")
    assert (rel.download_views() == views).all()
    rel.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_NAMES.get)
def test_download_refusals_leave_the_destination(fmt, gpu):
    import torch
    w, h = 18, 5
    ctx = _rendered(gpu, w, h, "rgba")
    lay = sref.pitched(fmt, w, h)
    host = poison.sentinel((V, lay.frame_stride))
    dev = torch.full((V * lay.frame_stride,), poison.SENTINEL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    good = sref.descriptor(L, lay, sref.HOST, host.ctypes.data, keep=host)
    good_dev = sref.descriptor(L, lay, sref.DEVICE, dev.data_ptr(), keep=dev)
    ctx.download_views_yuv(good)
    want = out_ref.frames(ctx.download_views(), out_ref.BT709, out_ref.LIMITED)
    assert (sref.gather(host, lay) == want).all()
    host[...] = poison.SENTINEL
    before = ctx.memory_info().workspace_bytes
    lib, raw = ctx._lib, lambda v0, k, m, r, d: ctx._lib.lfi_download_views_yuv(ctx._h, v0, k, m, r, C.byref(d) if d is not None else None)
    refused = [(what, (0, V, 0, 0, d), word) for what, d, word in _bad_descriptors(ctx, lay, host)]
    for d in (good, good_dev):
        refused += [
            ("n = 0", (0, 0, 0, 0, d), "n >= 1"),
            ("v0 + n beyond the views", (V - 1, 2, 0, 0, d), "inside"),
            ("v0 below 0", (-1, 2, 0, 0, d), "inside"),
            ("unknown matrix", (0, V, 2, 0, d), "matrix"),
            ("unknown range", (0, V, 0, -1, d), "range"),
        ]
    for what, args, word in refused:
        assert raw(*args) == -1, what   # LFI_EINVAL
        assert word in lib.lfi_last_error(ctx._h).decode(), (what, lib.lfi_last_error(ctx._h).decode())
        assert (host == poison.SENTINEL).all(), what
        assert ctx.memory_info().workspace_bytes == before, what
    torch.cuda.synchronize()
    assert (dev.cpu().numpy() == poison.SENTINEL).all()
    ctx.download_views_yuv(good_dev)   # … and the context goes on
    torch.cuda.synchronize()
    assert (sref.gather(dev.cpu().numpy().reshape(V, lay.frame_stride), lay) == want).all()
    ctx.close()
    # nothing rendered yet; a row window
    fresh = gpu.Context(0)
    fresh.set_grid(3, 3, w, h)
    assert fresh._lib.lfi_download_views_yuv(fresh._h, 0, 1, 0, 0, C.byref(good)) == -1 and "nothing rendered" in fresh._lib.lfi_last_error(fresh._h).decode()
    fresh.close()
    assert (host == poison.SENTINEL).all()
