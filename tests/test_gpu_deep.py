"""GPU (-m gpu): deep views — LFI_FLAG_DEEP_VIEWS through lfi_render / lfi_prepare (csrc/hip/deep_blend.hpp) and the LFI_YUV_DEEP formats of
lfi_download_views_yuv (csrc/hip/deep_yuv.hpp; GBRP10: copies).

STD codes and bytes are demanded `==` the oracle's (its chain's value, rounded as the header says).  TEN_WM codes must lie inside the interval of
the exact sum under the accumulation bound (tests/ten_interval.py, with two more bits: tests/deep_ref.interval10), and `code >> 2` must BE the
byte of the same launch.  The YUV frames are integers: `==` on every word, unused bits included, against tests/deep_ref.py applied to the deep
views' own download.  Every checked render is preceded by a poison of the views AND the deep planes (allocated by lfi_prepare first).

NOT tested, because the API cannot reach it: that a ranged launch leaves the DEEP planes of the other views as they were (a LFI_YUV_DEEP download
outside the last launch's range is refused, and nothing else reads the planes).  In its place the 8-bit views outside the range must still hold
the poison; the kernel stores a lane's bytes and codes under one predicate and one row index."""
import functools

import numpy as np
import pytest

import lfinterpolator_amd as L
import deep_ref as ref
import poison
import ten_interval
import yuv10_ref
from oracle import lfi_oracle_c as oc
from test_gpu_yuv_surfaces import _Surfaces

pytestmark = pytest.mark.gpu

DEEP_RENDER = poison.RENDER | L.LFI_POISON_DEEP
_byte = [0]


def _context(gpu, case, flags=L.LFI_FLAG_DEEP_VIEWS, layout="planar"):
    _, cols, rows, w, h, _, _, _, _, _ = case
    hp, _ = ref.inputs(L, oc, case)
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, w, h)
    ctx.fill_synthetic(ref.SEED)
    ctx.set_output_layout(layout)
    ctx.set_params(hp, flags=flags)
    return ctx, hp


def _render(ctx, method, v0=0, v1=None):
    """allocate the deep planes, poison them with the views, render, synchronise; returns the poison byte"""
    ctx.prepare(method, v0=v0, v1=v1)
    b = poison.POISON[_byte[0] & 1]
    _byte[0] += 1
    ctx.poison(DEEP_RENDER, b)
    ctx.render(method, v0=v0, v1=v1)
    ctx.sync()
    return b


@functools.lru_cache(maxsize=None)
def _std(name):
    case = ref.CASES[ref.CASE_IDS.index(name)]
    hp, lf = ref.inputs(L, oc, case)
    out, pre = oc.blend_std(lf, hp.focused_offsets, hp.offsets, hp.weights, return_prequant=True)
    return out, ref.q10_std(pre)


@functools.lru_cache(maxsize=None)
def _ten(name):
    case = ref.CASES[ref.CASE_IDS.index(name)]
    hp, lf = ref.inputs(L, oc, case)
    S, eps = ten_interval.exact_sums(oc, lf, hp)
    return ref.interval10(S, eps)


# ---- the blend ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ref.CASES, ids=ref.CASE_IDS)
def test_std_codes_and_bytes_are_the_oracles(case, gpu):
    ctx, _ = _context(gpu, case)
    want_bytes, want_codes = _std(case[0])
    for _ in range(2):   # both poison bytes
        _render(ctx, "STD")
        assert ctx.last_kernel_name() == "deep_blend<STD>"
        deep = ctx.download_deep_views()
        assert deep.dtype == np.uint16 and deep.shape == want_codes.shape
        assert (deep == want_codes).all(), (case[0], int((deep != want_codes).sum()))
        assert (ctx.download_views() == want_bytes).all(), case[0]
    ctx.close()


@pytest.mark.parametrize("case", ref.CASES, ids=ref.CASE_IDS)
def test_ten_codes_lie_in_their_intervals_and_shift_to_the_bytes(case, gpu):
    ctx, _ = _context(gpu, case)
    lo, hi = _ten(case[0])
    for _ in range(2):
        _render(ctx, "TEN_WM")
        assert ctx.last_kernel_name() == "deep_blend<TEN_WM>"
        deep, views = ctx.download_deep_views(), ctx.download_views()
        outside = int(((deep < lo) | (deep > hi)).sum())
        print(case[0], "codes outside their interval:", outside, "of", deep.size, "; at the upper value where two are admitted:",
              int(((deep == hi) & (hi != lo)).sum()), "of", int((hi != lo).sum()))
        assert outside == 0, (case[0], outside)
        assert (deep >> 2 == views[..., :3]).all() and (views[..., 3] == 255).all(), case[0]
        assert deep.max() <= 1023
    ctx.close()


def test_ten_dyadic_weights_give_the_exact_code(gpu):
    """one row of weights 1/64 over 64 images: every product and every partial sum is exact in fp32, whatever the order: == q10 of the exact sum"""
    case = ref.CASES[1]
    hp, lf = ref.inputs(L, oc, case)
    w = hp.weights.copy()
    w[0, :] = np.float16(1.0 / 64).view(np.uint16)
    hp2 = L.host.HostParams(hp.focused_offsets, hp.offsets, w, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)
    ctx, _ = _context(gpu, case)
    ctx.set_params(hp2, flags=L.LFI_FLAG_DEEP_VIEWS)
    _render(ctx, "TEN_WM", 0, 1)
    S = oc.blend_f64(lf, hp2.focused_offsets, hp2.offsets, hp2.weights, v0=0, v1=1)
    assert (ctx.download_deep_views(0, 1)[0] == ref.q10_ten(S[0])).all()
    ctx.close()


@pytest.mark.parametrize("method", ["STD", "TEN_WM"])
def test_a_view_range_writes_its_views_only(method, gpu):
    case = ref.CASES[1]
    ctx, _ = _context(gpu, case)
    v0, v1 = 5, 23
    b = _render(ctx, method, v0, v1)
    assert not poison.written_outside(ctx, v0, v1, b)
    deep = ctx.download_deep_views(v0, v1 - v0)
    if method == "STD":
        assert (deep == _std(case[0])[1][v0:v1]).all() and (ctx.download_views(v0, v1) == _std(case[0])[0][v0:v1]).all()
    else:
        lo, hi = _ten(case[0])
        assert ((deep >= lo[v0:v1]) & (deep <= hi[v0:v1])).all() and (deep >> 2 == ctx.download_views(v0, v1)[..., :3]).all()
    for bad in ((0, 64), (4, 2), (22, 2), (23, 1)):
        with pytest.raises(L.LfiError, match="LFI_YUV_DEEP"):
            ctx.download_deep_views(*bad)
    ctx.close()


def test_codes_are_the_same_after_release_inputs(gpu):
    case = ref.CASES[3]   # two chunks
    ctx, _ = _context(gpu, case)
    _render(ctx, "TEN_WM")
    first = ctx.download_deep_views()
    ctx.release_inputs()
    for method in ("TEN_WM", "STD"):
        _render(ctx, method)
        deep = ctx.download_deep_views()
        assert (deep == (first if method == "TEN_WM" else _std(case[0])[1])).all(), method
    ctx.close()


def test_planes_are_counted_with_the_views_and_prepared(gpu):
    case = ref.CASES[0]
    _, _, _, w, h, views, _, _, _, _ = case
    ctx, _ = _context(gpu, case)
    before = ctx.memory_info().views_bytes
    ctx.prepare("TEN_WM")
    pitch16 = (2 * w + 127) // 128 * 128
    assert ctx.memory_info().views_bytes == before + views * 3 * h * pitch16
    ctx.render("TEN_WM")
    ctx.sync()
    assert ctx.memory_info().views_bytes == before + views * 3 * h * pitch16
    ctx.set_output_layout("rgba")   # releases them with the views
    assert ctx.memory_info().views_bytes == views * h * w * 4
    ctx.close()


def test_benchmark_allocates_the_planes_before_its_first_timed_launch(gpu):
    case = ref.CASES[0]
    _, _, _, w, h, views, _, _, _, _ = case
    ctx, _ = _context(gpu, case)
    before = ctx.memory_info().views_bytes
    ctx.benchmark("STD", warmup=0, runs=2)
    assert ctx.last_kernel_name() == "deep_blend<STD>" and ctx.memory_info().views_bytes == before + views * 3 * h * ((2 * w + 127) // 128 * 128)
    assert (ctx.download_deep_views() == _std(case[0])[1]).all()
    with pytest.raises(L.LfiError, match="LFI_FLAG_DEEP_VIEWS"):
        ctx.benchmark("STD", all_focus=True, warmup=0, runs=1)
    ctx.close()


def test_another_number_of_views_drops_the_deep_views_under_attached_views_too(gpu):
    """an attached view buffer that still fits is kept by lfi_set_params; the deep views of the old parameters go all the same"""
    import torch
    case = ref.CASES[0]
    ctx, hp = _context(gpu, case)
    layout = ctx.view_layout()
    buf = torch.zeros(layout.view_stride_bytes * hp.weights.shape[0], dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.attach_views(buf.data_ptr(), buf.numel())
    _render(ctx, "TEN_WM")
    ctx.download_deep_views()
    ctx.set_params(hp.rows(0, 2), flags=L.LFI_FLAG_DEEP_VIEWS)
    with pytest.raises(L.LfiError, match="LFI_YUV_DEEP"):
        ctx.download_deep_views()
    _render(ctx, "TEN_WM")
    assert ctx.download_deep_views().shape[0] == 2
    ctx.close()
    del buf


# ---- frames from the deep views -------------------------------------------------------------------------------------------------------------------

V = 3
SITINGS = [(ref.CENTRE, "centre"), (ref.LEFT, "left")]
FORMATS = [(yuv10_ref.I010, "i010"), (yuv10_ref.P010, "p010")]


def _deep_rendered(gpu, w, h, method="TEN_WM"):
    hp = gpu.build_params(3, 3, w, h, "0,0,1,1", 0.2, 0.0, 3.0, 1.0, V)
    ctx = gpu.Context(0)
    ctx.set_grid(3, 3, w, h)
    ctx.fill_synthetic(ref.SEED)
    ctx.set_output_layout("planar")
    ctx.set_params(hp, flags=L.LFI_FLAG_DEEP_VIEWS)
    _render(ctx, method)
    return ctx


def _deep_surfaces(ctx, lay, memory, content, shift=0):
    dst = _Surfaces(ctx, lay, memory, content, shift=shift)
    dst.desc.format |= ref.DEEP
    return dst


def _destinations(fmt, w, h):
    """host tight and pitched (staged), device surfaces with pitches of 256 (written in place), and tight device surfaces two bytes into their
    allocation (a pitch that forces staging, device to device)"""
    return [(yuv10_ref.HOST, "host tight", yuv10_ref.tight(fmt, w, h), 0), (yuv10_ref.HOST, "host pitched", yuv10_ref.pitched(fmt, w, h), 0),
            (yuv10_ref.DEVICE, "device in place", yuv10_ref.pitched(fmt, w, h), 0), (yuv10_ref.DEVICE, "device at base + 2", yuv10_ref.tight(fmt, w, h), 2)]


@pytest.mark.parametrize("size", [(18, 5), (130, 5), (520, 6), (24, 10)], ids=["18x5", "130x5", "520x6", "24x10"])
def test_frames_equal_the_restatement_and_padding_keeps_its_poison(size, gpu):
    """18 x 5: ragged and odd, cw = 9; 130 x 5: 17 lanes of a wave, the left-sited exchange between them, a ragged block of two columns; 520 x 6:
    65 blocks per row, a second wave along x whose lane 0 loads pixel column 511 itself for the left-sited filter; 24 x 10: ch = 5, a second
    workgroup along y (the sizes of tests/test_gpu_yuv10.py for the sibling kernels)"""
    w, h = size
    ctx = _deep_rendered(gpu, w, h)
    deep, views = ctx.download_deep_views(), ctx.download_views()
    assert len(np.unique(deep)) > 64   # not a flat picture
    for siting, name in SITINGS:
        ctx.set_yuv_siting("centre", name)
        for conv in ref.FORMATS:
            want = ref.frames(deep, *conv, siting)
            for fmt, fname in FORMATS:
                for memory, what, lay, shift in _destinations(fmt, w, h):
                    for byte in poison.POISON:
                        dst = _deep_surfaces(ctx, lay, memory, np.full((V, lay.frame_stride), byte, np.uint8), shift=shift)
                        ctx.poison(L.LFI_POISON_SCRATCH, byte ^ 0xFF)
                        ctx.download_views_yuv(dst.desc, matrix=conv[0], range=conv[1])
                        got = dst.read()
                        case = (size, name, conv, fname, what, byte)
                        assert (yuv10_ref.gather(got, lay) == yuv10_ref.words(want, fmt)).all(), case   # the codes in place AND zeros in the unused bits
                        assert yuv10_ref.padding_holds(got, lay, byte), case
                # a sub-range: views [1, 3) into frames 0 and 1, frame 2 untouched
                lay = yuv10_ref.tight(fmt, w, h)
                dst = _deep_surfaces(ctx, lay, yuv10_ref.HOST, np.full((V, lay.frame_stride), 0x11, np.uint8))
                ctx.download_views_yuv(dst.desc, n=2, v0=1, matrix=conv[0], range=conv[1])
                got = dst.read()
                assert (yuv10_ref.gather(got[:2], lay) == yuv10_ref.words(want[1:], fmt)).all() and (got[2] == 0x11).all()
    # without LFI_YUV_DEEP the frames are what they were: made of the 8-bit views
    lay = yuv10_ref.tight(yuv10_ref.I010, w, h)
    plain = _Surfaces(ctx, lay, yuv10_ref.HOST, np.zeros((V, lay.frame_stride), np.uint8))
    ctx.set_yuv_siting("centre", "centre")
    ctx.download_views_yuv(plain.desc)
    assert (yuv10_ref.gather(plain.read(), lay) == yuv10_ref.frames(views, yuv10_ref.BT709, yuv10_ref.LIMITED)).all()
    assert (ctx.download_views() == views).all() and (ctx.download_deep_views() == deep).all()   # the calls write no view and no plane
    ctx.close()


def test_gbrp10_device_in_place_equals_the_host_route(gpu):
    w, h = 18, 5
    ctx = _deep_rendered(gpu, w, h, "STD")
    deep = ctx.download_deep_views()   # host, tight
    tight = dict(y_pitch=2 * w, c_offset=2 * w * h, c_pitch=2 * w, cr_offset=4 * w * h, frame_stride=6 * w * h)
    pitched = dict(y_pitch=256, c_offset=256 * h + 256, c_pitch=512, cr_offset=256 * h + 256 + 512 * h + 256, frame_stride=256 * h + 512 + 1024 * h + 256)
    for geo in (tight, pitched):
        lay = yuv10_ref.Layout(ref.GBRP10, w, h, geo["y_pitch"], geo["c_offset"], geo["c_pitch"], geo["cr_offset"], geo["frame_stride"])
        for memory in (yuv10_ref.HOST, yuv10_ref.DEVICE):
            for byte in poison.POISON:
                dst = _Surfaces(ctx, lay, memory, np.full((V, lay.frame_stride), byte, np.uint8))
                ctx.download_views_yuv(dst.desc, matrix="601", range="full")   # valid, ignored
                assert (dst.read() == ref.gbrp10_bytes(deep, poison=byte, **geo)).all(), (geo is tight, memory, byte)
        dst = _Surfaces(ctx, lay, yuv10_ref.DEVICE, np.full((V, lay.frame_stride), 0x11, np.uint8))
        ctx.download_views_yuv(dst.desc, n=1, v0=2)
        got = dst.read()
        assert (got[:1] == ref.gbrp10_bytes(deep[2:], poison=0x11, **geo)).all() and (got[1:] == 0x11).all()
    with pytest.raises(L.LfiError, match="matrix"):
        ctx.download_views_yuv(L.YuvSurfaces.gbrp10_from_array(np.zeros((V, 3, h, w), np.uint16)), matrix=7)
    ctx.close()


# ---- refusals and validity ------------------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_flag_and_leave_everything_as_it_was(gpu):
    case = ref.CASES[0]
    _, cols, rows, w, h, views, _, _, _, _ = case
    ctx, hp = _context(gpu, case)
    _render(ctx, "TEN_WM")
    deep, bytes_ = ctx.download_deep_views(), ctx.download_views()

    def unchanged():
        return (ctx.download_deep_views() == deep).all() and (ctx.download_views() == bytes_).all()

    def refused(call, word="LFI_FLAG_DEEP_VIEWS"):
        with pytest.raises(L.LfiError, match=word):
            call()
        assert unchanged()

    refused(lambda: ctx.render("TEN_WM", all_focus=True))
    refused(lambda: ctx.prepare("STD", all_focus=True))
    refused(lambda: ctx.render_stream("TEN_WM", np.tile(hp.weights, (2, 1))))
    refused(lambda: ctx.render_stream_yuv420("TEN_WM", np.tile(hp.weights, (2, 1))))
    refused(lambda: ctx.download_prequant("STD", 0))
    # per-view rows of either kind
    ctx.set_view_offsets(np.tile(hp.focused_offsets[None], (views, 1, 1)))
    refused(lambda: ctx.render("STD"))
    ctx.set_view_offsets(None)
    ctx.set_view_float_offsets(np.tile(hp.offsets[None], (views, 1, 1)))
    refused(lambda: ctx.render("STD"))
    ctx.set_view_float_offsets(None)
    ctx.render("STD")   # and served again
    ctx.render("TEN_WM")
    ctx.sync()
    assert unchanged()
    # LFI_FLAG_TEN_ROUND_PER_BATCH, weights outside [0, 2): the parameters change, the views and planes stay
    ctx.set_params(hp, flags=L.LFI_FLAG_DEEP_VIEWS | L.LFI_FLAG_TEN_ROUND_PER_BATCH)
    refused(lambda: ctx.render("TEN_WM"))
    wide = hp.weights.copy()
    wide[0, 0] = np.float16(2.5).view(np.uint16)
    ctx.set_params(L.host.HostParams(hp.focused_offsets, hp.offsets, wide, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius), flags=L.LFI_FLAG_DEEP_VIEWS)
    refused(lambda: ctx.render("STD"))
    ctx.set_params(hp, flags=L.LFI_FLAG_DEEP_VIEWS)
    # the surfaces calls that refuse a LFI_YUV_DEEP format by name
    for fmt in (ref.I010_DEEP, ref.P010_DEEP, ref.GBRP10):
        buf = np.zeros((1, 6 * 2 * w * 2 * h), np.uint8)
        one = L.yuv_surfaces_packed(fmt if fmt == ref.GBRP10 else fmt & ~ref.DEEP, "host", buf.ctypes.data, w, h, keep=buf)
        one.format = fmt
        refused(lambda: ctx.upload_images_yuv(one, 1), "LFI_YUV_DEEP")
        refused(lambda: ctx.download_rgbd_yuv(0, 1, 0, 0, w - w % 2, h - h % 2, "709", "limited", one), "LFI_YUV_DEEP")
        refused(lambda: ctx.download_quilt_yuv(1, 1, 0, w, h, "709", "limited", one), "LFI_YUV_DEEP")
    ctx.close()
    # a mosaic needs even image sizes: a grid of its own, 2 x 2 images of 16 x 4
    ctx = gpu.Context(0)
    ctx.set_grid(2, 2, 16, 4)
    for fmt in (ref.I010_DEEP, ref.P010_DEEP, ref.GBRP10):
        buf = np.zeros((1, 6 * 32 * 8), np.uint8)
        frame = L.yuv_surfaces_packed(fmt if fmt == ref.GBRP10 else fmt & ~ref.DEEP, "host", buf.ctypes.data, 32, 8, keep=buf)
        frame.format = fmt
        with pytest.raises(L.LfiError, match="LFI_YUV_DEEP"):
            ctx.upload_mosaic_yuv(L.Mosaic.make(2, 2, "grid"), frame)
    ctx.close()
    # the RGBA layout and a row window: contexts of their own
    ctx, _ = _context(gpu, case, layout="rgba")
    with pytest.raises(L.LfiError, match="LFI_FLAG_DEEP_VIEWS"):
        ctx.render("TEN_WM")
    with pytest.raises(L.LfiError, match="LFI_FLAG_DEEP_VIEWS"):
        ctx.prepare("TEN_WM")
    ctx.close()
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, w, h)
    ctx.set_row_window(1, 3, 0, h)
    ctx.fill_synthetic(ref.SEED)
    ctx.set_output_layout("planar")
    ctx.set_params(hp, flags=L.LFI_FLAG_DEEP_VIEWS)
    with pytest.raises(L.LfiError, match="LFI_FLAG_DEEP_VIEWS"):
        ctx.render("TEN_WM")
    ctx.close()
    # after lfi_release_inputs: offsets beyond the copy's reach
    ctx, hp = _context(gpu, case)
    ctx.render("TEN_WM")
    ctx.release_inputs()
    far = L.host.HostParams(hp.focused_offsets * 0 + np.array([w * 3, 0], np.int32), hp.offsets, hp.weights, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)
    ctx.set_params(far, flags=L.LFI_FLAG_DEEP_VIEWS)
    with pytest.raises(L.LfiError, match="LFI_FLAG_DEEP_VIEWS"):
        ctx.render("TEN_WM")
    ctx.close()


def test_a_render_without_the_flag_drops_the_deep_views_and_a_deep_render_restores_them(gpu):
    case = ref.CASES[0]
    ctx, hp = _context(gpu, case)
    with pytest.raises(L.LfiError, match="LFI_YUV_DEEP"):   # nothing deep rendered yet
        ctx.prepare("STD")
        ctx.download_deep_views()
    _render(ctx, "STD")
    deep = ctx.download_deep_views()
    ctx.set_params(hp)   # the flag off: the planes stay valid until a launch writes views without them
    assert (ctx.download_deep_views() == deep).all()
    poison.render(ctx, "STD")
    assert ctx.last_kernel_name() != "deep_blend<STD>"
    assert (ctx.download_views() == _std(case[0])[0]).all()   # the same bytes either way
    with pytest.raises(L.LfiError, match="LFI_YUV_DEEP"):
        ctx.download_deep_views()
    ctx.set_params(hp, flags=L.LFI_FLAG_DEEP_VIEWS)
    _render(ctx, "STD")
    assert (ctx.download_deep_views() == deep).all()
    ctx.set_output_layout("rgba")
    ctx.set_output_layout("planar")
    with pytest.raises(L.LfiError, match="LFI_YUV_DEEP"):
        ctx.download_deep_views()
    ctx.close()


# ---- the command line -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["TEN_WM", "STD"])
def test_cli_deep_writes_unchanged_pngs_and_frames_made_of_the_deep_views(method, gpu, tmp_path):
    """--deep --gbrp10 --p010 --y4m --yuv-depth 10 on a synthetic 3 x 3 grid of 18 x 6: the PNG files are those of a run without --deep; the raw
    planes hold 10-bit codes (TEN_WM: whose upper eight bits are the PNG's bytes); the P010 and C420p10 frames are the restatement applied to
    those codes; the program says which options read the raw files"""
    from PIL import Image
    from view_rows import run_cli
    w, h, n = 18, 6, 4
    args = ["--synthetic", f"3,3,{w},{h}", "-t", "0,0,1,1", "-m", method, "-n", str(n), "-b", "1", "-f", "0.2"]
    plain, deep = tmp_path / "plain", tmp_path / "deep"
    res = run_cli(gpu, *args, "-o", str(plain))
    assert res.returncode == 0, res.stderr
    raw, p010, y4m = tmp_path / "v.raw", tmp_path / "v.p010", tmp_path / "v.y4m"
    res = run_cli(gpu, *args, "-o", str(deep), "--deep", "--gbrp10", str(raw), "--p010", str(p010), "--y4m", str(y4m), "--yuv-depth", "10",
                  "--yuv-matrix", "601", "--yuv-range", "full")
    assert res.returncode == 0, (res.stdout, res.stderr)
    assert "deep views" in res.stdout and f"-f rawvideo -pix_fmt gbrp10le -s {w}x{h}" in res.stdout and "-pix_fmt p010le" in res.stdout
    want = np.stack([np.array(Image.open(plain / f"{v:02d}.png")) for v in range(n)])
    got = np.stack([np.array(Image.open(deep / f"{v:02d}.png")) for v in range(n)])
    assert (got == want).all()
    planes = np.fromfile(raw, "<u2").reshape(n, 3, h, w)
    codes = L.YuvSurfaces.gbrp10_to_rgb(planes)
    assert codes.max() <= 1023 and len(np.unique(codes)) > 64
    if method == "TEN_WM":
        assert (codes >> 2 == want[..., :3]).all()
    else:
        assert (np.abs(codes.astype(int) - 4 * want[..., :3].astype(int)) <= 2).all()   # rn(4 s) against 4 rn(s)
    frames = ref.frames(codes, ref.BT601, ref.FULL, ref.CENTRE)
    lay = yuv10_ref.tight(yuv10_ref.P010, w, h)
    got_p010 = np.fromfile(p010, np.uint8).reshape(n, lay.frame_stride)
    assert (yuv10_ref.gather(got_p010, lay) == yuv10_ref.words(frames, yuv10_ref.P010)).all()
    body = y4m.read_bytes()
    assert b"C420p10" in body[:80]
    lay = yuv10_ref.tight(yuv10_ref.I010, w, h)
    frame_bytes = lay.frame_stride
    payload = body[body.index(b"\n") + 1:]
    assert len(payload) == n * (len(b"FRAME\n") + frame_bytes)
    got_i010 = np.stack([np.frombuffer(payload[k * (6 + frame_bytes) + 6:(k + 1) * (6 + frame_bytes)], np.uint8) for k in range(n)])
    assert (yuv10_ref.gather(got_i010, lay) == yuv10_ref.words(frames, yuv10_ref.I010)).all()
