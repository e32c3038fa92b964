"""GPU (-m gpu): native lenticular images — lfi_download_native (csrc/hip/native_image.hpp, with csrc/hip/quilt_scaled.hpp as its first stage) and
the CLI's --native.

The interlace is defined in integers (include/lfi.h), so every comparison is byte for byte: the native image against the numpy restatement
(tests/native_ref.py, held against the definition by tests/test_host_native.py) applied to the views' own downloads.  The context's scratch
buffers — the device-resident scaled tiles and the native image's device copy among them — are poisoned before every checked call, every call
is checked under both poison bytes, and the host image is wider than the output and pre-filled with poison.SENTINEL: bytes outside the image
must stay untouched."""
import numpy as np
import pytest
from PIL import Image

import lfinterpolator_amd as L
import native_ref as ref
import poison
from conftest import SEED
from view_rows import run_cli

pytestmark = pytest.mark.gpu

COLS = ROWS = 3
W, H, V = ref.W, ref.H, ref.V
PAD = 7                                       # pixels the host image's rows are wider than the output
RANGES = ref.VIEW_RANGES + [(8, 1)]           # … and the 8 views the boundary step sets are made for


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


@pytest.mark.parametrize("tile", ref.TILES)
@pytest.mark.parametrize("layout", ["rgba", "planar"])
def test_native_image_equals_the_restatement(layout, tile, gpu):
    ctx = _ctx(gpu, _params(gpu), layout)
    poison.render(ctx, "STD")
    scaled = ref.tiles(ctx.download_views(), *tile)   # T_v of every view, once
    for out in ref.OUTPUTS:
        for n, v0 in RANGES:
            for name, steps in ref.STEPS.items():
                for invert in (False, True):
                    lens = ref.Lens(*steps, n, ref.INVERT if invert else 0)
                    want = ref.native(scaled, lens, v0, *out, *tile)
                    for _ in range(2):   # both poison bytes
                        got = _native(ctx, lens, v0, out, tile)
                        assert (got == want).all(), (layout, tile, out, n, v0, name, invert, int((got != want).sum()))
    ctx.close()


@pytest.mark.parametrize("layout", ["rgba", "planar"])
def test_one_view_at_the_views_size_is_the_view(layout, gpu):
    ctx = _ctx(gpu, _params(gpu), layout)
    poison.render(ctx, "STD")
    views = ctx.download_views()
    for v in (0, 4, 9):
        for _ in range(2):
            assert (_native(ctx, ref.Lens(*ref.STEPS["slant"], 1), v, (W, H), (W, H)) == views[v]).all(), (layout, v)
    ctx.close()


@pytest.mark.parametrize("layout", ["rgba", "planar"])
def test_native_image_of_attached_views(layout, gpu):
    import torch
    ctx = _ctx(gpu, _params(gpu, 6), layout)
    vl = ctx.view_layout()
    buf = torch.zeros(6 * vl.view_stride_bytes, dtype=torch.uint8, device="cuda:0")
    ctx.attach_views(buf.data_ptr(), buf.numel())
    poison.render(ctx, "STD")
    views = ctx.download_views()
    lens = ref.Lens(*ref.STEPS["negative slant"], 5, ref.INVERT)
    for tile in ((W, H), (17, 9)):
        for _ in range(2):
            assert (_native(ctx, lens, 1, (64, 36), tile) == ref.native(views, lens, 1, 64, 36, *tile)).all(), (layout, tile)
    ctx.close()


def test_refusals_leave_a_usable_context(gpu):
    hp = _params(gpu)
    ctx = _ctx(gpu, hp, "rgba")
    poison.render(ctx, "STD")
    views = ctx.download_views()
    lens = ref.Lens(*ref.STEPS["slant"], 10)
    want = ref.native(views, lens, 0, 64, 36, 17, 9)

    def valid():
        assert (_native(ctx, lens, 0, (64, 36), (17, 9)) == want).all()

    valid()
    narrow = poison.sentinel((36, 63, 4))
    image = poison.sentinel((36, 64 + PAD, 4))

    def call(lens=lens, v0=0, out=(64, 36), tile=(17, 9), img=image):
        return lambda: ctx.download_native(None if lens is None else _abi(lens), out[0], out[1], tile[0], tile[1], v0=v0, out=img)

    refused = [
        ("tile_w = W + 1", call(tile=(W + 1, 9)), "scaled quilt tiles"),
        ("tile_h = H + 1", call(tile=(17, H + 1)), "scaled quilt tiles"),
        ("tile_w = 0", call(tile=(0, 9)), "scaled quilt tiles"),
        ("tile_h = 0", call(tile=(17, 0)), "scaled quilt tiles"),
        ("n = 0", call(lens=lens.with_views(0)), "native image needs"),
        ("n = -1", call(lens=lens.with_views(-1)), "native image needs"),
        ("v0 + n beyond the views", call(lens=lens.with_views(4), v0=7), "native image needs"),
        ("v0 below 0", call(lens=lens.with_views(4), v0=-1), "native image needs"),
        ("pitch too small", call(img=narrow), "pitch"),
        ("no lens", call(lens=None), "lens description"),
        ("unknown flag bits", call(lens=ref.Lens(*ref.STEPS["slant"], 10, 2)), "flag bits"),
        ("unknown flag bits beside a known one", call(lens=ref.Lens(*ref.STEPS["slant"], 10, 1 | 1 << 31)), "flag bits"),
        ("out_w = 65536", call(out=(65536, 36), img=poison.sentinel((36, 64, 4))), "native images are"),
    ]
    for what, fn, message in refused:
        with pytest.raises(gpu.LfiError, match=message):
            fn()
        assert (image == poison.SENTINEL).all() and (narrow == poison.SENTINEL).all(), what
        valid()
    ctx.close()
    # a row window: the subpixels read rows the band does not hold
    band = (4, 12)
    win = gpu.Context(0)
    win.set_grid(COLS, ROWS, W, H)
    in_rows = gpu.input_rows(band, hp.focused_offsets, H)
    win.set_row_window(band[0], band[1], in_rows[0], in_rows[1])
    win.fill_synthetic(SEED)
    win.set_params(hp)
    poison.render(win, "STD")
    for tile in ((17, 9), (W, H)):
        with pytest.raises(gpu.LfiError, match="row window"):
            win.download_native(_abi(lens), 64, 36, tile[0], tile[1], out=image)
    assert (image == poison.SENTINEL).all()
    assert (win.download_view(0)[band[0]:band[1]] == views[0][band[0]:band[1]]).all()   # … and the context goes on
    win.close()
    # nothing rendered yet
    fresh = gpu.Context(0)
    with pytest.raises(gpu.LfiError, match="nothing rendered"):
        fresh.download_native(_abi(lens), 4, 4, 1, 1)
    fresh.close()


@pytest.mark.parametrize("layout", ["rgba", "planar"])
def test_the_call_has_no_side_effects_and_its_buffer_is_counted(layout, gpu):
    ctx = _ctx(gpu, _params(gpu), layout)
    poison.render(ctx, "STD")
    views = ctx.download_views()
    scaled = ctx.download_quilt_scaled(5, 2, 17, 9)
    before = ctx.memory_info().workspace_bytes
    lens = ref.Lens(*ref.STEPS["slant"], 10)
    _native(ctx, lens, 0, (131, 67), (17, 9))
    _native(ctx, lens, 0, (7, 5), (W, H))
    assert ctx.memory_info().workspace_bytes == before + 131 * 67 * 4   # the device image grows and is kept
    assert (ctx.download_views() == views).all()
    ctx.poison(L.LFI_POISON_SCRATCH, poison._byte(None))
    assert (ctx.download_quilt_scaled(5, 2, 17, 9) == scaled).all()
    ctx.close()


def test_cli_native_image(gpu, tmp_path):
    """--native 64x36 --lens … writes native.png = the restatement of the NN.png files of the same run under the Python calibration restatement;
    --native-tile and --native-views; the refusals"""
    dst = tmp_path / "out"
    args = ["--synthetic", "4,4,48,20", "-o", str(dst), "-t", "0,0.5,1,0.5", "-m", "TEN_WM", "-f", "0.1", "-n", "6", "-b", "1"]
    calibration = (11.25, -5.5, 0.125, 100.0)

    def views_of_the_run():
        return np.stack([np.array(Image.open(dst / f"{v:02d}.png")) for v in range(6)])

    res = run_cli(gpu, *args, "--native", "64x36", "--lens", "11.25,-5.5,0.125,100")
    assert res.returncode == 0, res.stderr
    native = np.array(Image.open(dst / "native.png"))
    lens = ref.calibrate(*calibration, False, 64, 36, 6)
    assert len(np.unique(ref.select(lens, 64, 36))) == 6          # the calibration is one that uses every view
    assert native.shape == (36, 64, 4) and (native == ref.native(views_of_the_run(), lens, 0, 64, 36, 48, 20)).all()
    res = run_cli(gpu, *args, "--native", "31x17", "--lens", "11.25,-5.5,0.125,100,1", "--native-tile", "24x10", "--native-views", "5")
    assert res.returncode == 0, res.stderr
    native = np.array(Image.open(dst / "native.png"))
    lens = ref.calibrate(*calibration, True, 31, 17, 5)
    assert native.shape == (17, 31, 4) and (native == ref.native(views_of_the_run(), lens, 0, 31, 17, 24, 10)).all()
    # refusals
    res = run_cli(gpu, *args, "--native", "64x36", "--lens", "11.25,-5.5,0.125,100", "-g", "2")
    assert res.returncode != 0 and "--native" in res.stderr and "one GPU" in res.stderr
    res = run_cli(gpu, *args, "--lens", "11.25,-5.5,0.125,100")
    assert res.returncode != 0 and "--lens" in res.stderr and "--native" in res.stderr
    for extra in (["--native", "64x36", "--lens", "11.25,-5.5,0.125"], ["--native", "64x36", "--lens", "11.25,0,0.125,100"],
                  ["--native", "64", "--lens", "11.25,-5.5,0.125,100"], ["--native", "64x36", "--lens", "11.25,-5.5,0.125,100", "--native-tile", "49x10"],
                  ["--native", "64x36", "--lens", "11.25,-5.5,0.125,100", "--native-views", "7"]):
        res = run_cli(gpu, *args, *extra)
        assert res.returncode != 0 and res.stderr.strip(), extra
