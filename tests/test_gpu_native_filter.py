"""GPU (-m gpu): FILTERED native lenticular images — lfi_download_native under LFI_LENT_BGR, LFI_LENT_BILINEAR and LFI_LENT_BLEND
(csrc/hip/native_filter.hpp) and the CLI's --native-filter, --native-blend, --lens-bgr and --lens-file.

Everything is defined in integers (include/lfi.h), so every comparison is byte for byte: the native image against the numpy restatement
(tests/native_filter_ref.py, held against the definition by tests/test_host_native_filter.py) applied to the views' own downloads.  As in
tests/test_gpu_native.py the context's scratch buffers are poisoned before every checked call, every call is checked under both poison
bytes, and the host image is wider than the output and pre-filled with poison.SENTINEL: bytes outside the image must stay untouched."""
import os

import numpy as np
import pytest
from PIL import Image

import lfinterpolator_amd as L
import native_filter_ref as fref
import native_ref as ref
import poison
from conftest import GOLDEN_DIR, SEED
from native_filter_ref import BGR, BILINEAR, BLEND
from native_ref import INVERT
from view_rows import run_cli

pytestmark = pytest.mark.gpu

COLS = ROWS = 3
W, H, V = ref.W, ref.H, ref.V
PAD = 7                                       # pixels the host image's rows are wider than the output


def _ctx(gpu, hp, layout):
    ctx = gpu.Context(0)
    ctx.set_grid(COLS, ROWS, W, H)
    ctx.fill_synthetic(SEED)
    ctx.set_params(hp)
    ctx.set_output_layout(layout)
    return ctx


def _params(gpu, views=V):
    return gpu.build_params(COLS, ROWS, W, H, "0,0,1,1", 0.2, 0.0, 3.0, 1.0, views)


def _abi(lens):
    return L.Lenticular(lens.x_step, lens.y_step, lens.phase0, lens.views, lens.flags)


def _native(ctx, lens, v0, out, tile):
    """the native image under poison, in a host image PAD pixels wider than the output; asserts that the padding is untouched"""
    ctx.poison(L.LFI_POISON_SCRATCH, poison._byte(None))
    img = poison.sentinel((out[1], out[0] + PAD, 4))
    ctx.download_native(_abi(lens), out[0], out[1], tile[0], tile[1], v0=v0, out=img)
    assert (img[:, out[0]:] == poison.SENTINEL).all(), "bytes outside the native image were written"
    return img[:, :out[0]]


def _lenses():
    """(name, steps, n, v0): the two general step sets with every view range, the two boundary sets with the 8 views they are made for"""
    for n, v0 in fref.VIEW_RANGES:
        for name in ref.GENERAL:
            yield name, ref.STEPS[name], n, v0
    for name in ("boundary", "boundary rows"):
        yield name, ref.STEPS[name], 8, 1


@pytest.mark.parametrize("tile", ref.TILES)
@pytest.mark.parametrize("layout", ["rgba", "planar"])
def test_filtered_native_image_equals_the_restatement(layout, tile, gpu):
    ctx = _ctx(gpu, _params(gpu), layout)
    poison.render(ctx, "STD")
    scaled = ref.tiles(ctx.download_views(), *tile)   # T_v of every view, once
    for out in fref.OUTPUTS:
        for name, steps, n, v0 in _lenses():
            for flags in fref.GPU_FLAG_SETS:
                lens = ref.Lens(*steps, n, flags)
                want = fref.native(scaled, lens, v0, *out, *tile)
                for _ in range(2):   # both poison bytes
                    got = _native(ctx, lens, v0, out, tile)
                    assert (got == want).all(), (layout, tile, out, n, v0, name, flags, int((got != want).sum()))
    ctx.close()


@pytest.mark.parametrize("layout", ["rgba", "planar"])
def test_filtered_native_image_of_attached_views(layout, gpu):
    import torch
    ctx = _ctx(gpu, _params(gpu, 6), layout)
    vl = ctx.view_layout()
    buf = torch.zeros(6 * vl.view_stride_bytes, dtype=torch.uint8, device="cuda:0")
    ctx.attach_views(buf.data_ptr(), buf.numel())
    poison.render(ctx, "STD")
    views = ctx.download_views()
    lens = ref.Lens(*ref.STEPS["negative slant"], 5, INVERT | BGR | BILINEAR | BLEND)
    for tile in ((W, H), (17, 9)):
        for _ in range(2):
            assert (_native(ctx, lens, 1, (64, 36), tile) == fref.native(views, lens, 1, 64, 36, *tile)).all(), (layout, tile)
    ctx.close()


@pytest.mark.parametrize("layout", ["rgba", "planar"])
def test_bilinear_at_the_tiles_own_size_is_the_plain_call(layout, gpu):
    """tile = out: every bilinear weight is 0 — the flag changes no byte (and the call takes the cheaper route)"""
    ctx = _ctx(gpu, _params(gpu), layout)
    poison.render(ctx, "STD")
    for size in ((W, H), (17, 9), (1, 1)):
        for flags in (0, INVERT, BLEND | BGR):
            lens = ref.Lens(*ref.STEPS["slant"], 10, flags)
            plain = _native(ctx, lens, 0, size, size).copy()
            for _ in range(2):
                assert (_native(ctx, ref.Lens(*ref.STEPS["slant"], 10, flags | BILINEAR), 0, size, size) == plain).all(), (layout, size, flags)
    ctx.close()


def test_unknown_flag_bits_stay_refused(gpu):
    ctx = _ctx(gpu, _params(gpu), "rgba")
    poison.render(ctx, "STD")
    views = ctx.download_views()
    lens = ref.Lens(*ref.STEPS["slant"], 10, BILINEAR | BLEND)
    want = fref.native(views, lens, 0, 64, 36, 17, 9)
    image = poison.sentinel((36, 64 + PAD, 4))
    for flags in (64, 2 | 8, 1 << 5, 2, 1 | 1 << 31, 4 | 8 | 16 | 32):
        with pytest.raises(gpu.LfiError, match="flag bits"):
            ctx.download_native(_abi(ref.Lens(*ref.STEPS["slant"], 10, flags)), 64, 36, 17, 9, out=image)
        assert (image == poison.SENTINEL).all(), flags
        assert (_native(ctx, lens, 0, (64, 36), (17, 9)) == want).all()   # the context goes on
    ctx.close()


def test_cli_filtered_native_image(gpu, tmp_path):
    """--native 31x17 --lens-file … --native-filter bilinear --native-blend writes native.png = the restatement of the NN.png files of the same
    run; --lens-bgr likewise"""
    dst = tmp_path / "out"
    golden = os.path.join(GOLDEN_DIR, "lens_calibration.json")
    args = ["--synthetic", "4,4,48,20", "-o", str(dst), "-t", "0,0.5,1,0.5", "-m", "TEN_WM", "-f", "0.1", "-n", "6", "-b", "1"]

    def views_of_the_run():
        return np.stack([np.array(Image.open(dst / f"{v:02d}.png")) for v in range(6)])

    res = run_cli(gpu, *args, "--native", "31x17", "--lens-file", golden, "--native-filter", "bilinear", "--native-blend")
    assert res.returncode == 0, res.stderr
    assert "3840x2160" in res.stdout and "31x17" in res.stdout      # the note: the file describes another panel
    native = np.array(Image.open(dst / "native.png"))
    cal = ref.calibrate(52.5741, -7.1956, -0.3817, 283.0, True, 31, 17, 6)
    lens = ref.Lens(cal.x_step, cal.y_step, cal.phase0, 6, INVERT | BILINEAR | BLEND)
    assert len(np.unique(ref.select(cal, 31, 17))) == 6               # the calibration is one that uses every view
    assert native.shape == (17, 31, 4) and (native == fref.native(views_of_the_run(), lens, 0, 31, 17, 48, 20)).all()
    assert (native != ref.native(views_of_the_run(), cal, 0, 31, 17, 48, 20)).any()
    res = run_cli(gpu, *args, "--native", "64x36", "--lens", "11.25,-5.5,0.125,100", "--lens-bgr", "--native-tile", "24x10", "--native-views", "5")
    assert res.returncode == 0, res.stderr
    native = np.array(Image.open(dst / "native.png"))
    cal = ref.calibrate(11.25, -5.5, 0.125, 100.0, False, 64, 36, 5)
    lens = ref.Lens(cal.x_step, cal.y_step, cal.phase0, 5, BGR)
    assert native.shape == (36, 64, 4) and (native == fref.native(views_of_the_run(), lens, 0, 64, 36, 24, 10)).all()
    assert (native != ref.native(views_of_the_run(), cal, 0, 64, 36, 24, 10)).any()
