"""GPU (-m gpu): 10-bit video surfaces — LFI_YUV_I010 and LFI_YUV_P010 through lfi_download_views_yuv, lfi_upload_images_yuv and
lfi_download_quilt_yuv (csrc/hip/yuv10.hpp), under both sitings, and the two calls that refuse them.

Both definitions are integers (include/lfi.h), so every comparison is `==` on every sample, against tests/yuv10_ref.py applied to the views'
own downloads and to the codes that were uploaded.  Every byte the frames do not own holds a poison: two poisons must give the same grid, a
download must leave every one of them as it was, and every written sample's six unused bits must be 0."""
import ctypes as C

import numpy as np
import pytest

import lfinterpolator_amd as L
import poison
import scaled_quilt_ref
import yuv10_ref as ref
import yuv_ref as ref8
from test_gpu_yuv_surfaces import V, _Surfaces, _attached, _read, _rendered, _reset

pytestmark = pytest.mark.gpu

# W x H: the 8-bit surface tests' shapes — one block; ragged and odd with cw = 9 and rows that are not 16-byte aligned; 65 blocks per row (a
# second wave along x, chroma neighbours and the left-sited exchange across its boundary); a second workgroup along y — and the smallest
# frame and a ragged block of one column with an odd H
SIZES = [(8, 2), (18, 5), (520, 6), (24, 10), (1, 1), (9, 3)]
SIZE_IDS = [f"{w}x{h}" for w, h in SIZES]
FORMATS = [ref.I010, ref.P010]
FORMAT_NAMES = {ref.I010: "i010", ref.P010: "p010"}
SITINGS = [(ref.CENTRE, "centre"), (ref.LEFT, "left")]


def _destinations(fmt, w, h):
    """(memory, what, layout, shift): host tight and pitched (staged), device surfaces with pitches of 256 (written in place), and tight
    device surfaces two bytes into their allocation (staged device-to-device)"""
    return [(ref.HOST, "host tight", ref.tight(fmt, w, h), 0), (ref.HOST, "host pitched", ref.pitched(fmt, w, h), 0),
            (ref.DEVICE, "device in place", ref.pitched(fmt, w, h), 0), (ref.DEVICE, "device at base + 2", ref.tight(fmt, w, h), 2)]


# ---- download -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["rgba", "planar"])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_frames_equal_the_restatement_and_padding_keeps_its_poison(size, layout, gpu):
    w, h = size
    ctx = _rendered(gpu, w, h, layout)
    views = ctx.download_views()
    for siting, name in SITINGS:
        ctx.set_yuv_siting("centre", name)
        for conv in ref.FORMATS:
            want = ref.frames(views, *conv, siting)
            for fmt in FORMATS:
                for memory, what, lay, shift in _destinations(fmt, w, h):
                    for byte in poison.POISON:
                        dst = _Surfaces(ctx, lay, memory, np.full((V, lay.frame_stride), byte, np.uint8), shift=shift)
                        ctx.poison(L.LFI_POISON_SCRATCH, byte ^ 0xFF)
                        ctx.download_views_yuv(dst.desc, matrix=conv[0], range=conv[1])
                        got = dst.read()
                        case = (size, layout, name, conv, FORMAT_NAMES[fmt], what, byte)
                        # the words as they lie: the codes in their place AND zeros in the six unused bits
                        assert (ref.gather(got, lay) == ref.words(want, fmt)).all(), case
                        assert ref.padding_holds(got, lay, byte), case
                    # a sub-range: views [1, 3) into frames 0 and 1, frame 2 untouched
                    dst = _Surfaces(ctx, lay, memory, np.full((V, lay.frame_stride), 0x11, np.uint8), shift=shift)
                    ctx.download_views_yuv(dst.desc, n=2, v0=1, matrix=conv[0], range=conv[1])
                    got = dst.read()
                    assert (ref.gather(got[:2], lay) == ref.words(want[1:], fmt)).all() and ref.padding_holds(got[:2], lay, 0x11) and (got[2] == 0x11).all()
    assert (ctx.download_views() == views).all()   # the call writes no view
    ctx.close()


def test_random_attached_views(gpu):
    """views of random bytes in attached memory, 520 x 6 and 130 x 4: every column's neighbour differs from it, so the left-sited exchange
    between lanes, across a 16-lane row (x = 128) and into a second wave (x = 512) shows; both view layouts, both formats, both sitings"""
    from test_gpu_yuv import _attached as attached_views
    for w, h in ((520, 6), (130, 4)):
        content = np.random.default_rng(w).integers(0, 256, (3, h, w, 4), dtype=np.uint8)
        content[..., 3] = 255
        for layout in ("rgba", "planar"):
            ctx, buf = attached_views(gpu, w, h, layout, content)
            for siting, name in SITINGS:
                ctx.set_yuv_siting("centre", name)
                for conv in (ref.FORMATS[1], ref.FORMATS[2]):
                    want = ref.frames(content, *conv, siting)
                    for fmt in FORMATS:
                        lay = ref.tight(fmt, w, h)
                        dst = _Surfaces(ctx, lay, ref.HOST, np.full((3, lay.frame_stride), 0xA5, np.uint8))
                        ctx.download_views_yuv(dst.desc, matrix=conv[0], range=conv[1])
                        assert (ref.gather(dst.read(), lay) == ref.words(want, fmt)).all(), (w, h, layout, name, conv, FORMAT_NAMES[fmt])
            ctx.close()
            del buf


def test_attached_views_reach_the_extremes(gpu):
    """the cube's corners in every 2 x 2 arrangement (tests/yuv_ref.py), uniform corners and greys: 64, 940, 960 and both ends of full range"""
    from test_gpu_yuv import _attached as attached_views
    w, h = 128, 66
    content = ref8.corner_views(w, h, 3)
    ctx, buf = attached_views(gpu, w, h, "rgba", content)
    seen = set()
    for siting, name in SITINGS:
        ctx.set_yuv_siting("centre", name)
        for conv in ref.FORMATS:
            want = ref.frames(content, *conv, siting)
            lay = ref.tight(ref.P010, w, h)
            dst = _Surfaces(ctx, lay, ref.HOST, np.full((3, lay.frame_stride), 0x5A, np.uint8))
            ctx.download_views_yuv(dst.desc, matrix=conv[0], range=conv[1])
            assert (ref.gather(dst.read(), lay) == ref.words(want, ref.P010)).all(), (name, conv)
            if siting == ref.CENTRE:   # uniform 2 x 2 blocks of the corners: the chroma's ends (the left-sited filter mixes neighbouring blocks)
                seen.add((conv[1], int(want[:, :w * h].min()), int(want[:, :w * h].max()), int(want[:, w * h:].min()), int(want[:, w * h:].max())))
    assert {(ref.LIMITED, 64, 940, 64, 960), (ref.FULL, 0, 1023, 1, 1023)} == seen
    ctx.close()
    del buf


def test_the_device_frames_grow_to_the_larger_depth(gpu):
    """the staged frames of a host download: 24 x 6 + 2 x 12 x 3 bytes per 8-bit frame of 18 x 5, twice that per 10-bit frame; the buffer grows
    once and an 8-bit call afterwards leaves it alone"""
    w, h = 18, 5
    staged = 24 * 6 + 2 * 12 * 3
    ctx = _rendered(gpu, w, h, "rgba")
    base = ctx.memory_info().workspace_bytes
    first = ctx.download_views_yuv420()
    assert ctx.memory_info().workspace_bytes == base + V * staged
    lay = ref.tight(ref.I010, w, h)
    dst = _Surfaces(ctx, lay, ref.HOST, np.zeros((V, lay.frame_stride), np.uint8))
    ctx.download_views_yuv(dst.desc)
    assert ctx.memory_info().workspace_bytes == base + 2 * V * staged
    ctx.poison(L.LFI_POISON_SCRATCH, 0xA5)   # covers the grown frames
    assert (ctx.download_views_yuv420() == first).all()
    assert ctx.memory_info().workspace_bytes == base + 2 * V * staged
    # in place: no buffer at all
    fresh = _rendered(gpu, w, h, "rgba")
    lay = ref.pitched(ref.P010, w, h)
    dst = _Surfaces(fresh, lay, ref.DEVICE, np.zeros((V, lay.frame_stride), np.uint8))
    fresh.download_views_yuv(dst.desc)
    assert fresh.memory_info().workspace_bytes == base
    fresh.close()
    ctx.close()


# ---- upload -------------------------------------------------------------------------------------------------------------------------------------

def _codes(w, h, n, seed=0):
    """uniformly random 10-bit codes in all planes — codes outside the nominal ranges hit both clamps — and, as the last frame, the extremes"""
    codes = np.random.default_rng(seed + w * 1000 + h).integers(0, 1024, (n, ref.sizes(w, h)[2]), dtype=np.uint16)
    codes[-1] = ref.extremes_frame(w, h)
    return codes


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_NAMES.get)
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_grid_equals_the_restatement(size, fmt, gpu):
    """the four coefficient sets x both sitings x both filters, from host frames (tight: staged) and from device surfaces in place (pitches of
    256), the padding poisoned with 0x00 and then with 0xFF: the grid is the restatement's, byte for byte, alpha included"""
    w, h = size
    n = 2
    codes = _codes(w, h, n)
    ctx, grid = _attached(gpu, n, 1, w, h)
    sources = [(ref.HOST, "host tight", ref.tight(fmt, w, h)), (ref.DEVICE, "device in place", ref.pitched(fmt, w, h))]
    for siting, name in SITINGS:
        ctx.set_yuv_siting(name, "centre")
        for conv in ref.FORMATS:
            for filt in (ref.BILINEAR, ref.NEAREST):
                want = ref.images(codes, w, h, *conv, filt, siting)
                assert (want[..., 3] == 255).all()
                for memory, what, lay in sources:
                    for byte in (0x00, 0xFF):
                        content = ref.scatter(codes, lay, byte)
                        surfaces = _Surfaces(ctx, lay, memory, content)
                        _reset(grid)
                        ctx.poison(L.LFI_POISON_SCRATCH, byte ^ 0x5A)
                        before = ctx.memory_info().workspace_bytes
                        ctx.upload_images_yuv(surfaces.desc, n, matrix=conv[0], range=conv[1], chroma=filt)
                        got = _read(ctx, grid)
                        assert (got == want).all(), (size, FORMAT_NAMES[fmt], name, conv, filt, what, byte, int((got != want).sum()))
                        assert (surfaces.read() == content).all(), "the source surfaces were written"
                        if memory == ref.DEVICE:
                            assert ctx.memory_info().workspace_bytes == before   # read in place: no staging buffer
    ctx.close()
    del grid


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_NAMES.get)
def test_the_unused_bits_are_ignored(fmt, gpu):
    """a P010 frame with random bits in its low six, an I010 frame with random bits above bit 9: the same grid"""
    w, h = 18, 5
    n = 3
    codes = _codes(w, h, n, seed=3)
    junk = np.random.default_rng(33).integers(0, 65536, codes.shape, dtype=np.uint16)
    ctx, grid = _attached(gpu, n, 1, w, h)
    for siting, name in SITINGS:
        ctx.set_yuv_siting(name, "centre")
        want = ref.images(codes, w, h, ref.BT709, ref.LIMITED, ref.BILINEAR, siting)
        for memory, lay in ((ref.HOST, ref.pitched(fmt, w, h)), (ref.DEVICE, ref.pitched(fmt, w, h)), (ref.DEVICE, ref.tight(fmt, w, h))):
            content = ref.scatter(codes, lay, 0xFF, junk)
            assert (content != ref.scatter(codes, lay, 0xFF)).any()
            surfaces = _Surfaces(ctx, lay, memory, content)
            _reset(grid)
            ctx.upload_images_yuv(surfaces.desc, n)
            assert (_read(ctx, grid) == want).all(), (FORMAT_NAMES[fmt], name, memory)
    ctx.close()
    del grid


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_NAMES.get)
def test_eighteen_frames_take_two_chunks_from_the_host(fmt, gpu):
    """chunks of 16 + 2 through a buffer of 16 staged 10-bit frames; a range of images leaves the others alone"""
    w, h = 18, 5
    n = 18
    padded = 2 * (24 * 6 + 2 * 12 * 3)
    codes = _codes(w, h, n, seed=1)
    want = ref.images(codes, w, h, ref.BT709, ref.LIMITED)
    lay = ref.pitched(fmt, w, h)
    content = ref.scatter(codes, lay, 0x5A)
    ctx, grid = _attached(gpu, 6, 3, w, h)
    before = ctx.memory_info().workspace_bytes
    host = _Surfaces(ctx, lay, ref.HOST, content)
    ctx.upload_images_yuv(host.desc, n)
    assert (_read(ctx, grid) == want).all()
    assert ctx.memory_info().workspace_bytes == before + 16 * padded
    _reset(grid)
    ctx.upload_images_yuv(host.desc, 5, g0=7, matrix="601", range="full", chroma="nearest")
    got = _read(ctx, grid)
    assert (got[7:12] == ref.images(codes[:5], w, h, ref.BT601, ref.FULL, ref.NEAREST)).all()
    assert (got[:7] == 0x3C).all() and (got[12:] == 0x3C).all()
    ctx.close()
    del grid


# ---- quilt --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["rgba", "planar"])
@pytest.mark.parametrize("tile", [(18, 10), (17, 9)], ids=["even-18x10", "odd-17x9"])
def test_quilt_frames_equal_the_restatement_of_the_scaled_quilt(tile, layout, gpu):
    """a 3 x 2 quilt of views of 50 x 22: by definition the 10-bit frame of lfi_download_quilt_scaled's image taken as one view — two launches for
    even tiles too"""
    from test_gpu_quilt_yuv import _rendered as rendered_quilt
    tx, ty = 3, 2
    tw, th = tile
    ctx = rendered_quilt(gpu, layout)
    views = ctx.download_views()
    scaled = scaled_quilt_ref.quilt(views, tx, ty, tw, th)
    assert (scaled == ctx.download_quilt_scaled(tx, ty, tw, th)).all()
    qw, qh = tx * tw, ty * th
    for siting, name in SITINGS:
        ctx.set_yuv_siting("centre", name)
        for conv in (ref.FORMATS[0], ref.FORMATS[3]):
            want = ref.codes(scaled, *conv, siting)[None]
            for fmt in FORMATS:
                for memory, what, lay, shift in _destinations(fmt, qw, qh):
                    for byte in (0x00, 0xFF):
                        dst = _Surfaces(ctx, lay, memory, np.full((1, lay.frame_stride), byte, np.uint8), shift=shift)
                        ctx.poison(L.LFI_POISON_SCRATCH, byte ^ 0x5A)
                        ctx.download_quilt_yuv(tx, ty, 0, tw, th, conv[0], conv[1], dst.desc)
                        got = dst.read()
                        case = (tile, layout, name, conv, FORMAT_NAMES[fmt], what, byte)
                        assert (ref.gather(got, lay) == ref.words(want, fmt)).all(), case
                        assert ref.padding_holds(got, lay, byte), case
    assert (ctx.download_views() == views).all()
    ctx.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------

def _bad_descriptors(ctx, lay, host):
    """(what, descriptor, word of the message): what test_gpu_yuv_surfaces._bad_descriptors lists for the 8-bit formats, in samples of two
    bytes, and the alignment cases of the 10-bit formats"""
    assert host.ctypes.data % 2 == 0
    def make(memory=ref.HOST, base=host.ctypes.data, **changes):
        d = dict(fmt=lay.fmt, frame_stride=lay.frame_stride, y_pitch=lay.y_pitch, c_offset=lay.c_offset, c_pitch=lay.c_pitch, cr_offset=lay.cr_offset)
        d.update(changes)
        return L.YuvSurfaces.make(d["fmt"], memory, base, d["frame_stride"], d["y_pitch"], d["c_offset"], d["c_pitch"], d["cr_offset"], keep=host)
    cw = (lay.w + 1) // 2
    c_min = 4 * cw if lay.fmt == ref.P010 else 2 * cw
    return [
        ("NULL descriptor", None, "NULL"),
        ("NULL base", make(base=None), "NULL"),
        ("unknown format", make(fmt=0x100 | 2), "format"),
        ("plain 2", make(fmt=2), "format"),
        ("unknown memory", make(memory=2), "memory"),
        ("y_pitch a sample below 2W", make(y_pitch=2 * lay.w - 2), "pitch"),
        ("y_pitch a byte below 2W", make(y_pitch=2 * lay.w - 1), "pitch"),
        ("the 8-bit y_pitch", make(y_pitch=lay.w), "pitch"),
        ("c_pitch a sample below its minimum", make(c_pitch=c_min - 2), "pitch"),
        ("c_pitch a byte below its minimum", make(c_pitch=c_min - 1), "pitch"),
        ("chroma inside the Y plane", make(c_offset=lay.h * lay.y_pitch - 2), "overlap"),
        ("Cr inside Cb / cr_offset with P010", make(cr_offset=lay.c_offset + 2), "cr_offset"),
        ("frame_stride below the extent", make(frame_stride=lay.extent - 2), "frame_stride"),
        ("an odd y_pitch", make(y_pitch=lay.y_pitch + 1, c_offset=lay.c_offset + 2 * lay.h, cr_offset=lay.cr_offset and lay.cr_offset + 2 * lay.h), "alignment"),
        ("an odd c_pitch", make(c_pitch=c_min + 1), "alignment"),
        ("an odd c_offset", make(c_offset=lay.c_offset + 1), "alignment"),
        ("an odd frame_stride", make(frame_stride=lay.frame_stride + 1), "alignment"),
        ("an odd base", make(base=host.ctypes.data + 1), "alignment"),
        ("a host pointer as LFI_MEM_DEVICE", make(memory=ref.DEVICE), "device memory"),
        ("page-locked host memory as LFI_MEM_DEVICE", make(memory=ref.DEVICE, base=ctx.pinned_empty((4 * lay.frame_stride,)).ctypes.data), "device memory"),
    ]


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_NAMES.get)
def test_upload_refusals_leave_the_grid_and_the_staging_buffer(fmt, gpu):
    w, h = 18, 5
    n = 3
    codes = _codes(w, h, n, seed=5)
    lay = ref.pitched(fmt, w, h)
    host = ref.scatter(codes, lay, 0)
    ctx, grid = _attached(gpu, n, 1, w, h)
    good = ref.descriptor(L, lay, ref.HOST, host.ctypes.data, keep=host)
    before = ctx.memory_info().workspace_bytes
    lib, raw = ctx._lib, lambda g0, k, m, r, c, d: ctx._lib.lfi_upload_images_yuv(ctx._h, g0, k, m, r, c, C.byref(d) if d is not None else None)
    refused = [(what, (0, n, 0, 0, 0, d), word) for what, d, word in _bad_descriptors(ctx, lay, host)]
    refused += [("n = 0", (0, 0, 0, 0, 0, good), "n >= 1"), ("g0 + n beyond the grid", (n - 1, 2, 0, 0, 0, good), "inside"),
                ("unknown matrix", (0, n, 2, 0, 0, good), "matrix"), ("unknown chroma", (0, n, 0, 0, 2, good), "chroma")]
    for what, args, word in refused:
        assert raw(*args) == -1, what   # LFI_EINVAL
        assert word in lib.lfi_last_error(ctx._h).decode(), (what, lib.lfi_last_error(ctx._h).decode())
        assert (_read(ctx, grid) == 0x3C).all(), what
        assert ctx.memory_info().workspace_bytes == before, what
    ctx.upload_images_yuv(good, n)   # … and the context goes on
    assert (_read(ctx, grid) == ref.images(codes, w, h, ref.BT709, ref.LIMITED)).all()
    ctx.close()
    del grid


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_NAMES.get)
def test_download_refusals_leave_the_destination_and_an_8_bit_call_is_a_fresh_contexts(fmt, gpu):
    import torch
    w, h = 18, 5
    ctx = _rendered(gpu, w, h, "rgba")
    views = ctx.download_views()
    lay = ref.pitched(fmt, w, h)
    host = poison.sentinel((V, lay.frame_stride))
    dev = torch.full((V * lay.frame_stride,), poison.SENTINEL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    good = ref.descriptor(L, lay, ref.HOST, host.ctypes.data, keep=host)
    good_dev = ref.descriptor(L, lay, ref.DEVICE, dev.data_ptr(), keep=dev)
    ctx.download_views_yuv(good)
    want = ref.frames(views, ref.BT709, ref.LIMITED)
    assert (ref.gather(host, lay) == ref.words(want, fmt)).all()
    host[...] = poison.SENTINEL
    before = ctx.memory_info().workspace_bytes
    lib, raw = ctx._lib, lambda v0, k, m, r, d: ctx._lib.lfi_download_views_yuv(ctx._h, v0, k, m, r, C.byref(d) if d is not None else None)
    refused = [(what, (0, V, 0, 0, d), word) for what, d, word in _bad_descriptors(ctx, lay, host)]
    for d in (good, good_dev):
        refused += [("n = 0", (0, 0, 0, 0, d), "n >= 1"), ("v0 + n beyond the views", (V - 1, 2, 0, 0, d), "inside"),
                    ("unknown matrix", (0, V, 2, 0, d), "matrix"), ("unknown range", (0, V, 0, -1, d), "range")]
    for what, args, word in refused:
        assert raw(*args) == -1, what   # LFI_EINVAL
        assert word in lib.lfi_last_error(ctx._h).decode(), (what, lib.lfi_last_error(ctx._h).decode())
        assert (host == poison.SENTINEL).all(), what
        assert ctx.memory_info().workspace_bytes == before, what
    # lfi_download_rgbd_yuv refuses the 10-bit formats, for a destination it would take as 8-bit
    assert lib.lfi_download_rgbd_yuv(ctx._h, 0, 1, 0, 0, 8, 4, 0, 0, C.byref(good)) == -1
    assert "10-bit" in lib.lfi_last_error(ctx._h).decode(), lib.lfi_last_error(ctx._h).decode()
    assert (host == poison.SENTINEL).all() and ctx.memory_info().workspace_bytes == before
    torch.cuda.synchronize()
    assert (dev.cpu().numpy() == poison.SENTINEL).all()
    ctx.download_views_yuv(good_dev)   # … and the context goes on
    torch.cuda.synchronize()
    assert (ref.gather(dev.cpu().numpy().reshape(V, lay.frame_stride), lay) == ref.words(want, fmt)).all()
    # an 8-bit call on the same context gives the bytes of a context that never saw a 10-bit format
    fresh = _rendered(gpu, w, h, "rgba")
    assert (fresh.download_views() == views).all()
    for conv in ref8.FORMATS:
        assert (ctx.download_views_yuv420(matrix=conv[0], range=conv[1]) == fresh.download_views_yuv420(matrix=conv[0], range=conv[1])).all(), conv
    assert (ctx.download_views_yuv420() == ref8.frames(views, ref8.BT709, ref8.LIMITED)).all()
    fresh.close()
    ctx.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_NAMES.get)
def test_the_derived_upload_refuses_ten_bit_frames(fmt, gpu):
    """a context that holds only the planar copy: 10-bit frames are refused, the copy and the workspace stay, and the 8-bit call still works"""
    from test_gpu_yuv_derived import _lean
    import yuv_in_ref as in8
    shape = (5, 4, 18, 5, 0.9)
    cols, rows, w, h, _ = shape
    n = cols * rows
    images = np.random.default_rng(21).integers(0, 256, (n, h, w, 4), dtype=np.uint8)
    images[..., 3] = 255
    ctx = _lean(gpu, shape, images)
    planes = ctx.download_derived()
    before = ctx.memory_info().workspace_bytes
    codes = _codes(w, h, n, seed=8)
    lay = ref.tight(fmt, w, h)
    host = ref.scatter(codes, lay, 0)
    desc = ref.descriptor(L, lay, ref.HOST, host.ctypes.data, keep=host)
    assert ctx._lib.lfi_upload_images_yuv_derived(ctx._h, 0, n, 0, 0, 0, C.byref(desc)) == -1
    assert "10-bit" in ctx._lib.lfi_last_error(ctx._h).decode(), ctx._lib.lfi_last_error(ctx._h).decode()
    ctx.upload_wait()
    ctx.sync()
    assert (ctx.download_derived() == planes).all() and ctx.memory_info().workspace_bytes == before
    second = np.random.default_rng(22).integers(0, 256, (n, in8.sizes(w, h)[2]), dtype=np.uint8)
    ctx.upload_images_yuv_derived(ctx.yuv_surfaces_packed("i420", "host", second.ctypes.data, keep=second), n)
    ctx.upload_wait()
    ctx.sync()
    assert not (ctx.download_derived() == planes).all()
    ctx.close()
