"""GPU (-m gpu): scaled quilts — lfi_download_quilt_scaled / lfi_download_quilt_tiles_scaled (csrc/hip/quilt_scaled.hpp) and the CLI's --quilt-tile.

The resize is defined in integers (include/lfi.h), so every comparison is byte for byte: the scaled quilt against the numpy restatement
(tests/scaled_quilt_ref.py, held against the definition by tests/test_host_scaled_quilt.py) applied to the views' own downloads.  The context's
scratch buffers — the quilt's device image among them — are poisoned before every call a check reads, with alternating bytes, and the host image
is wider than the quilt and pre-filled with poison.SENTINEL: bytes outside the quilt must stay untouched."""
import numpy as np
import pytest
from PIL import Image

import lfinterpolator_amd as L
import poison
import scaled_quilt_ref as ref
from conftest import SEED
from view_rows import run_cli

pytestmark = pytest.mark.gpu

COLS = ROWS = 3
W, H, V = 50, 22, 10            # a width that is not a multiple of four; 50 = 2·25, 22 = 2·11
TILES = [(17, 9), (25, 11), (50, 11), (50, 22), (1, 1)]
PAD = 7                         # pixels the host image's rows are wider than the quilt


def _ctx(gpu, hp, layout, cols=COLS, rows=ROWS, w=W, h=H):
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, w, h)
    ctx.fill_synthetic(SEED)
    ctx.set_params(hp)
    ctx.set_output_layout(layout)
    return ctx


def _params(gpu, views=V):
    return gpu.build_params(COLS, ROWS, W, H, "0,0,1,1", 0.2, 0.0, 3.0, 1.0, views)


def _scaled(ctx, tiles_x, tiles_y, tw, th, v0=0):
    """the scaled quilt under poison, in a host image PAD pixels wider than the quilt; asserts that the padding is untouched"""
    ctx.poison(L.LFI_POISON_SCRATCH, poison._byte(None))
    out = poison.sentinel((tiles_y * th, tiles_x * tw + PAD, 4))
    ctx.download_quilt_scaled(tiles_x, tiles_y, tw, th, v0=v0, out=out)
    assert (out[:, tiles_x * tw:] == poison.SENTINEL).all(), "bytes outside the quilt were written"
    return out[:, :tiles_x * tw]


@pytest.mark.parametrize("layout", ["rgba", "planar"])
def test_scaled_quilt_equals_the_restatement(layout, gpu):
    ctx = _ctx(gpu, _params(gpu), layout)
    poison.render(ctx, "STD")
    views = ctx.download_views()
    for tw, th in TILES:
        for tx, ty, v0 in ((3, 3, 0), (4, 2, 1), (1, 1, 7)):
            for _ in range(2):   # both poison bytes
                got = _scaled(ctx, tx, ty, tw, th, v0=v0)
                want = ref.quilt(views[v0:], tx, ty, tw, th)
                assert (got == want).all(), (layout, tw, th, tx, ty, v0, int((got != want).sum()))
    # the views' own size: the unscaled quilt's bytes
    assert (_scaled(ctx, 4, 2, W, H, v0=1) == ctx.download_quilt(4, 2, v0=1)).all()
    ctx.close()


@pytest.mark.parametrize("layout", ["rgba", "planar"])
def test_scaled_quilt_of_attached_views(layout, gpu):
    import torch
    ctx = _ctx(gpu, _params(gpu, 6), layout)
    vl = ctx.view_layout()
    buf = torch.zeros(6 * vl.view_stride_bytes, dtype=torch.uint8, device="cuda:0")
    ctx.attach_views(buf.data_ptr(), buf.numel())
    poison.render(ctx, "STD")
    views = ctx.download_views()
    for tw, th in ((17, 9), (25, 11)):
        assert (_scaled(ctx, 3, 2, tw, th) == ref.quilt(views, 3, 2, tw, th)).all(), (layout, tw, th)
    ctx.close()


@pytest.mark.parametrize("layout", ["rgba", "planar"])
def test_three_contexts_fill_one_scaled_quilt(layout, gpu):
    """contexts that hold views [0, 3), [3, 8), [8, 10) of the trajectory fill tiles 0-2, 3-7, 8-9 of a 5 x 2 quilt: ranges that start and end in
    the middle of a row of tiles (up to three rectangles per call)"""
    hp = _params(gpu)
    tw, th = 17, 9
    ctx = _ctx(gpu, hp, layout)
    poison.render(ctx, "STD")
    want = _scaled(ctx, 5, 2, tw, th)
    assert (want == ref.quilt(ctx.download_views(), 5, 2, tw, th)).all()
    ctx.close()
    got = poison.sentinel((2 * th, 5 * tw + PAD, 4))
    for v0, v1 in ((0, 3), (3, 8), (8, 10)):
        part = _ctx(gpu, hp.rows(v0, v1), layout)
        poison.render(part, "STD")
        part.poison(L.LFI_POISON_SCRATCH, poison._byte(None))
        part.download_quilt_tiles_scaled(got, 5, 2, v0, v1 - v0, tw, th)
        part.close()
    assert (got[:, :5 * tw] == want).all() and (got[:, 5 * tw:] == poison.SENTINEL).all()


def test_refusals_leave_a_usable_context(gpu):
    hp = _params(gpu)
    ctx = _ctx(gpu, hp, "rgba")
    poison.render(ctx, "STD")
    views = ctx.download_views()
    want = ref.quilt(views, 3, 2, 17, 9)

    def valid():
        assert (_scaled(ctx, 3, 2, 17, 9) == want).all()

    valid()
    narrow = poison.sentinel((2 * 9, 3 * 17 - 1, 4))
    refused = [
        ("tile_w = W + 1", lambda: ctx.download_quilt_scaled(3, 2, W + 1, 9), "scaled quilt tiles"),
        ("tile_h = 0", lambda: ctx.download_quilt_scaled(3, 2, 17, 0), "scaled quilt tiles"),
        ("tile_w = 0", lambda: ctx.download_quilt_scaled(3, 2, 0, 9), "scaled quilt tiles"),
        ("tile_h = H + 1", lambda: ctx.download_quilt_scaled(3, 2, 17, H + 1), "scaled quilt tiles"),
        ("too many tiles", lambda: ctx.download_quilt_scaled(4, 3, 17, 9), "quilt needs"),
        ("tiles past the quilt", lambda: ctx.download_quilt_tiles_scaled(poison.sentinel((18, 51, 4)), 3, 2, 5, 2, 17, 9), "quilt needs"),
        ("no tiles", lambda: ctx.download_quilt_scaled(0, 2, 17, 9), "quilt needs"),
        ("pitch too small", lambda: ctx.download_quilt_scaled(3, 2, 17, 9, out=narrow), "pitch"),
    ]
    for what, call, message in refused:
        with pytest.raises(gpu.LfiError, match=message):
            call()
        valid()
    assert (narrow == poison.SENTINEL).all()
    ctx.close()
    # a row window: a tile's rows average source rows the band does not hold
    band = (4, 12)
    win = gpu.Context(0)
    win.set_grid(COLS, ROWS, W, H)
    in_rows = gpu.input_rows(band, hp.focused_offsets, H)
    win.set_row_window(band[0], band[1], in_rows[0], in_rows[1])
    win.fill_synthetic(SEED)
    win.set_params(hp)
    poison.render(win, "STD")
    with pytest.raises(gpu.LfiError, match="row window"):
        win.download_quilt_scaled(3, 2, 17, 9)
    got = np.zeros((2 * H, 3 * W, 4), np.uint8)   # … and the context goes on: the unscaled quilt of the band
    win.download_quilt_tiles(got, 3, 2, 0, 6)
    assert (got[band[0]:band[1], :W] == views[0][band[0]:band[1]]).all()
    win.close()
    # nothing rendered yet
    fresh = gpu.Context(0)
    with pytest.raises(gpu.LfiError, match="nothing rendered"):
        fresh.download_quilt_scaled(1, 1, 1, 1)
    fresh.close()


@pytest.mark.parametrize("layout", ["rgba", "planar"])
def test_the_call_has_no_side_effects(layout, gpu):
    ctx = _ctx(gpu, _params(gpu), layout)
    poison.render(ctx, "STD")
    views = ctx.download_views()
    unscaled = ctx.download_quilt(5, 2)
    _scaled(ctx, 5, 2, 17, 9)
    _scaled(ctx, 1, 1, 1, 1, v0=9)
    assert (ctx.download_views() == views).all()
    ctx.poison(L.LFI_POISON_SCRATCH, poison._byte(None))
    assert (ctx.download_quilt(5, 2) == unscaled).all()
    ctx.close()


def test_full_size_quilt_of_config_3(gpu):
    """BASELINE config 3's shape (15 x 15 @ 1080p, 45 views, TEN_WM, planar layout) as the 5 x 9 quilt of a 4096 x 4096 Looking-Glass image: tiles
    of 819 x 455.  Six tiles — the first, the last and four spread over the quilt — against the restatement of their views, every byte."""
    cols = rows = 15
    w, h, views, tw, th = 1920, 1080, 45, 819, 455
    hp = gpu.build_params(cols, rows, w, h, "0,0.5,1,0.5", 0.06, 0.0, 3.0, 2.276, views)
    ctx = _ctx(gpu, hp, "planar", cols, rows, w, h)
    poison.render(ctx, "TEN_WM")
    ctx.poison(L.LFI_POISON_SCRATCH, poison._byte(None))
    got = ctx.download_quilt_scaled(5, 9, tw, th)
    assert got.shape == (9 * th, 5 * tw, 4)
    for v in (0, 7, 18, 26, 38, 44):
        ty, tx = divmod(v, 5)
        want = ref.resize(ctx.download_view(v), tw, th)
        tile = got[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]
        assert (tile == want).all(), (v, int((tile != want).sum()))
    ctx.close()


def test_cli_scaled_quilt(gpu, tmp_path):
    """-q 3,2 --quilt-tile 24x10 writes quilt.png of 3 x 2 tiles of 24 x 10 pixels = the restatement of the NN.png files; -q alone is unchanged"""
    dst = tmp_path / "out"
    args = ["--synthetic", "4,4,48,20", "-o", str(dst), "-t", "0,0.5,1,0.5", "-m", "TEN_WM", "-f", "0.1", "-n", "6", "-q", "3,2", "-b", "1"]
    res = run_cli(gpu, *args, "--quilt-tile", "24x10")
    assert res.returncode == 0, res.stderr
    quilt = np.array(Image.open(dst / "quilt.png"))
    assert quilt.shape == (2 * 10, 3 * 24, 4) == (20, 72, 4)
    for v in range(6):
        view = np.array(Image.open(dst / f"{v:02d}.png"))
        ty, tx = divmod(v, 3)
        assert (quilt[ty * 10:(ty + 1) * 10, tx * 24:(tx + 1) * 24] == ref.resize(view, 24, 10)).all(), v
    # ratios that are not integers
    res = run_cli(gpu, *args, "--quilt-tile", "17x9")
    assert res.returncode == 0, res.stderr
    quilt = np.array(Image.open(dst / "quilt.png"))
    assert quilt.shape == (18, 51, 4)
    for v in range(6):
        ty, tx = divmod(v, 3)
        assert (quilt[ty * 9:(ty + 1) * 9, tx * 17:(tx + 1) * 17] == ref.resize(np.array(Image.open(dst / f"{v:02d}.png")), 17, 9)).all(), v
    # refusals: no quilt, a size outside the limits, a malformed size
    res = run_cli(gpu, *args[:-4], "-b", "1", "--quilt-tile", "24x10")
    assert res.returncode != 0 and "--quilt-tile" in res.stderr and "-q" in res.stderr
    for size in ("49x10", "24x21", "0x10", "24", "axb"):
        res = run_cli(gpu, *args, "--quilt-tile", size)
        assert res.returncode != 0 and ("tile" in res.stderr), (size, res.stderr)
