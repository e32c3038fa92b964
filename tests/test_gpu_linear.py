"""GPU (-m gpu): linear-light blending — LFI_FLAG_LINEAR_LIGHT through lfi_render / lfi_prepare / lfi_benchmark (csrc/hip/blend_linear.hpp) and the
program's --light linear.

STD bytes are demanded `==` the numpy restatement of the header's definition (tests/linear_ref.py) on every case.  TEN_WM bytes must lie inside the
interval of the exact sum; with one-hot and half/half weight rows that is `==`, and the one-hot views are the input images' own bytes.
tests/test_host_linear.py shows on the CPU that these renders tell a linear-light render from an encoded one (more than 90 % of the bytes differ)
and that no interval holds more than two values.  Every checked render is preceded by a poison of the views."""
import functools

import numpy as np
import pytest

import lfinterpolator_amd as L
import linear_ref as ref
import poison
import ten_interval
from oracle import lfi_oracle_c as oc

pytestmark = pytest.mark.gpu

FLAG = L.LFI_FLAG_LINEAR_LIGHT
NAME = {"STD": "blend_linear<STD>", "TEN_WM": "blend_linear<TEN_WM>"}


def _context(gpu, case, hp=None, flags=FLAG, layout="planar"):
    _, cols, rows, w, h, _, _ = case
    hp = hp or ref.inputs(L, oc, case)[0]
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, w, h)
    ctx.fill_synthetic(ref.SEED)
    ctx.set_output_layout(layout)
    ctx.set_params(hp, flags=flags)
    return ctx, hp


@functools.lru_cache(maxsize=None)
def _encoded(name):
    """the oracle's flag-free STD render of a case"""
    hp, lf = ref.inputs(L, oc, ref.CASES[ref.CASE_IDS.index(name)])
    return oc.blend_std(lf, hp.focused_offsets, hp.offsets, hp.weights)


@functools.lru_cache(maxsize=None)
def _interval(name):
    case = ref.CASES[ref.CASE_IDS.index(name)]
    hp, lf = ref.inputs(L, oc, case)
    return ref.ten_interval_of(ref.restated(L, oc, case), hp, lf.shape[0])


def _std_ok(got, res, name, v0=0, v1=None):
    want = res.bytes[v0:v1]
    assert (got[..., 3] == 255).all(), name
    assert (got[..., :3] == want).all(), (name, v0, v1, int((got[..., :3] != want).sum()))


def _ten_ok(got, name, v0=0, v1=None, interval=None):
    lo, hi = interval or _interval(name)
    lo, hi = lo[v0:v1], hi[v0:v1]
    out = ten_interval.outside(got, lo, hi)   # alpha 255 too
    c = got[..., :3]
    print(name, (v0, v1), "bytes outside their interval:", out, "of", c.size, "; at the upper value where two are admitted:", int(((c == hi) & (hi != lo)).sum()),
          "of", int((hi != lo).sum()))
    assert out == 0, (name, out)


def _ok(method, got, case, v0=0, v1=None):
    if method == "STD":
        _std_ok(got, ref.restated(L, oc, case), case[0], v0, v1)
    else:
        _ten_ok(got, case[0], v0, v1)


# ---- the blend ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ref.CASES, ids=ref.CASE_IDS)
def test_std_bytes_are_the_restatements(case, gpu):
    ctx, hp = _context(gpu, case)
    res = ref.restated(L, oc, case)
    views = hp.weights.shape[0]
    for _ in range(2):   # both poison bytes
        poison.render(ctx, "STD")
        assert ctx.last_kernel_name() == NAME["STD"]
        _std_ok(ctx.download_views(), res, case[0])
    for v1 in (3, 64):   # 3 views: a quarter of one wave's 16; 64: one pass exactly
        if v1 <= views:
            b = poison.render(ctx, "STD", v1=v1)
            _std_ok(ctx.download_views(0, v1), res, case[0], 0, v1)
            assert not poison.written_outside(ctx, 0, v1, b, views=(v1, views - 1))
    ctx.close()


@pytest.mark.parametrize("case", ref.CASES, ids=ref.CASE_IDS)
def test_ten_bytes_lie_in_their_intervals(case, gpu):
    ctx, hp = _context(gpu, case)
    views = hp.weights.shape[0]
    for _ in range(2):
        poison.render(ctx, "TEN_WM")
        assert ctx.last_kernel_name() == NAME["TEN_WM"]
        _ten_ok(ctx.download_views(), case[0])
    for v1 in (3, 64):
        if v1 <= views:
            b = poison.render(ctx, "TEN_WM", v1=v1)
            _ten_ok(ctx.download_views(0, v1), case[0], 0, v1)
            assert not poison.written_outside(ctx, 0, v1, b, views=(v1, views - 1))
    ctx.close()


def test_one_hot_and_half_rows_are_exact_under_both_methods(gpu):
    """rows 0 and 1 hold a single 1.0, row 2 two weights of 0.5: every product and partial sum is exact in fp32 whatever the order, so TEN_WM == the
    restatement with no interval; the one-hot views are the input image at the clamped offsets, and every byte value 0 ... 255 occurs in them: the
    whole of D and E is exercised on the device"""
    hp, lf = ref.exact_rows(L, oc)
    res = ref.restate(lf, hp)
    px = ref.samples(lf, hp.focused_offsets)
    rows = [v for v, _ in ref.ONE_HOT] + [v for v, _, _ in ref.HALVES]
    ctx, _ = _context(gpu, ref.ONE_CHUNK_70, hp=hp)
    interval = ref.ten_interval_of(res, hp, lf.shape[0])
    for method in ("TEN_WM", "STD"):
        poison.render(ctx, method)
        assert ctx.last_kernel_name() == NAME[method]
        got = ctx.download_views()
        assert (got[..., 3] == 255).all()
        assert (got[rows][..., :3] == res.bytes[rows]).all(), (method, int((got[rows][..., :3] != res.bytes[rows]).sum()))
        for v, g in ref.ONE_HOT:
            assert (got[v][..., :3] == px[g]).all(), (method, v)
        assert len(np.unique(got[[v for v, _ in ref.ONE_HOT]][..., :3])) == 256
        if method == "STD":
            _std_ok(got, res, "exact_rows")
        else:
            _ten_ok(got, "exact_rows", interval=interval)
    ctx.close()


@pytest.mark.parametrize("method", ["STD", "TEN_WM"])
def test_a_view_range_writes_its_views_only(method, gpu):
    case = ref.ONE_CHUNK_70
    ctx, _ = _context(gpu, case)
    v0, v1 = 5, 23
    for _ in range(2):
        b = poison.render(ctx, method, v0=v0, v1=v1)
        assert not poison.written_outside(ctx, v0, v1, b)
        _ok(method, ctx.download_views(v0, v1), case, v0, v1)
    ctx.close()


@pytest.mark.parametrize("method", ["STD", "TEN_WM"])
def test_a_view_range_that_ends_with_the_padded_weight_matrix(method, gpu):
    """64 views (the matrix is padded to 64 rows), views [37, 64): the second wave's 16 views start at 53 and would end at 69 — the weights of
    views 53 ... 63 are read without reading across the matrix's end, and land in their places"""
    case = ref.ONE_CHUNK_70
    hp = ref.inputs(L, oc, case)[0].rows(0, 64)
    ctx, _ = _context(gpu, case, hp=hp)
    v0, v1 = 37, 64
    b = poison.render(ctx, method, v0=v0, v1=v1)
    assert not poison.written_outside(ctx, v0, v1, b)
    _ok(method, ctx.download_views(v0, v1), case, v0, v1)
    ctx.close()


# ---- state and interface ----------------------------------------------------------------------------------------------------------------------------

def test_the_same_bytes_after_release_inputs(gpu):
    case = ref.TWO_CHUNKS_70
    ctx, _ = _context(gpu, case)
    poison.render(ctx, "TEN_WM")
    first = ctx.download_views()
    _ten_ok(first, case[0])
    ctx.release_inputs()
    for method in ("TEN_WM", "STD"):
        poison.render(ctx, method)
        assert ctx.last_kernel_name() == NAME[method]
        got = ctx.download_views()
        if method == "TEN_WM":
            assert (got == first).all()
        else:
            _std_ok(got, ref.restated(L, oc, case), case[0])
    ctx.close()


def test_a_prepared_render_is_only_a_launch_and_benchmark_reports_the_kernel(gpu):
    case = ref.RAGGED
    ctx, _ = _context(gpu, case)
    ctx.prepare("STD")
    m = ctx.memory_info()
    built = (m.grid_bytes, m.derived_bytes, m.views_bytes, m.maps_bytes, m.workspace_bytes)
    assert m.derived_bytes > 0
    poison.render(ctx, "STD")
    m = ctx.memory_info()
    assert (m.grid_bytes, m.derived_bytes, m.views_bytes, m.maps_bytes, m.workspace_bytes) == built
    _std_ok(ctx.download_views(), ref.restated(L, oc, case), case[0])
    ctx.close()
    ctx, _ = _context(gpu, case)
    for method in ("STD", "TEN_WM"):
        ctx.poison(poison.RENDER, poison.POISON[0])
        ctx.benchmark(method, warmup=0, runs=2)
        assert ctx.last_kernel_name() == NAME[method]
        _ok(method, ctx.download_views(), case)
    with pytest.raises(L.LfiError, match="LFI_FLAG_LINEAR_LIGHT is set: "):
        ctx.benchmark("STD", all_focus=True, warmup=0, runs=1)
    ctx.close()


@pytest.mark.parametrize("method", ["STD", "TEN_WM"])
def test_the_flag_is_handed_over_between_renders(method, gpu):
    case = ref.RAGGED
    ctx, hp = _context(gpu, case)

    def flagged():
        poison.render(ctx, method)
        assert ctx.last_kernel_name() == NAME[method]
        got = ctx.download_views()
        _ok(method, got, case)
        return got

    first = flagged()
    ctx.set_params(hp)   # the flag off: the encoded render, by another kernel
    poison.render(ctx, method)
    assert "blend_linear" not in ctx.last_kernel_name()
    plain = ctx.download_views()
    if method == "STD":
        assert (plain == _encoded(case[0])).all()
    else:
        lf = ref.inputs(L, oc, case)[1]
        assert ten_interval.outside(plain, *ten_interval.bounds(oc, lf, hp)) == 0
    assert (plain[..., :3] != first[..., :3]).mean() > 0.90
    ctx.set_params(hp, flags=FLAG)
    assert (flagged() == first).all()
    ctx.close()


def test_a_linear_render_drops_the_deep_views(gpu):
    case = ref.RAGGED
    ctx, hp = _context(gpu, case, flags=L.LFI_FLAG_DEEP_VIEWS)
    ctx.prepare("STD")
    ctx.render("STD")
    ctx.sync()
    assert ctx.download_deep_views().shape[0] == hp.weights.shape[0]
    ctx.set_params(hp, flags=FLAG)
    poison.render(ctx, "STD")
    _std_ok(ctx.download_views(), ref.restated(L, oc, case), case[0])
    with pytest.raises(L.LfiError, match="LFI_YUV_DEEP"):
        ctx.download_deep_views()
    ctx.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_flag_and_leave_the_views_as_they_were(gpu):
    case = ref.RAGGED
    _, cols, rows, w, h, views, _ = case
    ctx, hp = _context(gpu, case)
    poison.render(ctx, "TEN_WM")
    bytes_ = ctx.download_views()
    _ten_ok(bytes_, case[0])

    def held():
        m = ctx.memory_info()
        return m.grid_bytes, m.derived_bytes, m.views_bytes, m.maps_bytes, m.workspace_bytes

    def refused(call, match="LFI_FLAG_LINEAR_LIGHT is set: "):
        before = held()
        with pytest.raises(L.LfiError, match=match):
            call()
        assert held() == before                          # nothing allocated
        assert (ctx.download_views() == bytes_).all()    # nothing written

    def served():
        """a flag-free render works after the refusal; then the linear-light bytes again"""
        ctx.set_params(hp)
        poison.render(ctx, "STD")
        assert (ctx.download_views() == _encoded(case[0])).all()
        ctx.set_params(hp, flags=FLAG)
        poison.render(ctx, "TEN_WM")
        assert (ctx.download_views() == bytes_).all()

    refused(lambda: ctx.render("TEN_WM", all_focus=True))
    refused(lambda: ctx.prepare("STD", all_focus=True))
    refused(lambda: ctx.render_stream("TEN_WM", np.tile(hp.weights, (2, 1))))
    refused(lambda: ctx.render_stream_yuv420("TEN_WM", np.tile(hp.weights, (2, 1))))
    refused(lambda: ctx.download_prequant("STD", 0))
    served()
    # per-view rows of either kind
    ctx.set_view_offsets(np.tile(hp.focused_offsets[None], (views, 1, 1)))
    refused(lambda: ctx.render("STD"))
    ctx.set_view_offsets(None)
    ctx.set_view_float_offsets(np.tile(hp.offsets[None], (views, 1, 1)))
    refused(lambda: ctx.render("STD"))
    ctx.set_view_float_offsets(None)
    served()
    # LFI_FLAG_TEN_ROUND_PER_BATCH, LFI_FLAG_DEEP_VIEWS or LFI_FLAG_IN_FRAME beside it, weights outside [0, 2): the parameters change, the views stay
    ctx.set_params(hp, flags=FLAG | L.LFI_FLAG_TEN_ROUND_PER_BATCH)
    refused(lambda: ctx.render("TEN_WM"))
    for other in (L.LFI_FLAG_DEEP_VIEWS, L.LFI_FLAG_IN_FRAME, L.LFI_FLAG_DEEP_VIEWS | L.LFI_FLAG_IN_FRAME):
        ctx.set_params(hp, flags=FLAG | other)
        refused(lambda: ctx.render("STD"))
        refused(lambda: ctx.prepare("STD"))
        refused(lambda: ctx.benchmark("TEN_WM", warmup=0, runs=1))
    # without the new flag the pair keeps the message it had
    ctx.set_params(hp, flags=L.LFI_FLAG_DEEP_VIEWS | L.LFI_FLAG_IN_FRAME)
    refused(lambda: ctx.render("STD"), match="LFI_FLAG_IN_FRAME is set: LFI_FLAG_DEEP_VIEWS is not supported together with it")
    wide = hp.weights.copy()
    wide[0, 0] = np.float16(2.5).view(np.uint16)
    ctx.set_params(ref.with_weights(L, hp, wide), flags=FLAG)
    refused(lambda: ctx.render("STD"))
    served()
    ctx.close()
    # the RGBA layout and a row window: contexts of their own
    ctx, _ = _context(gpu, case, layout="rgba")
    for call in (lambda: ctx.render("TEN_WM"), lambda: ctx.prepare("TEN_WM")):
        with pytest.raises(L.LfiError, match="LFI_FLAG_LINEAR_LIGHT is set: "):
            call()
    ctx.set_params(hp)
    poison.render(ctx, "STD")
    assert (ctx.download_views() == _encoded(case[0])).all()
    ctx.close()
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, w, h)
    ctx.set_row_window(1, 9, 0, h)   # rows 1 ... 8 of the views, every input row held
    ctx.fill_synthetic(ref.SEED)
    ctx.set_output_layout("planar")
    ctx.set_params(hp, flags=FLAG)
    with pytest.raises(L.LfiError, match="LFI_FLAG_LINEAR_LIGHT is set: "):
        ctx.render("TEN_WM")
    ctx.close()
    # after lfi_release_inputs: offsets beyond the copy's reach
    ctx, hp = _context(gpu, case)
    ctx.render("TEN_WM")
    ctx.release_inputs()
    far = L.host.HostParams(hp.focused_offsets * 0 + np.array([w * 3, 0], np.int32), hp.offsets, hp.weights, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)
    ctx.set_params(far, flags=FLAG)
    with pytest.raises(L.LfiError, match="LFI_FLAG_LINEAR_LIGHT is set: "):
        ctx.render("TEN_WM")
    ctx.close()


# ---- the command line -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["TEN_WM", "STD"])
def test_cli_light_linear_writes_the_apis_views(method, gpu, tmp_path):
    """--light linear on a synthetic 3 x 3 grid of 18 x 6: the PNG files hold the API's bytes for the same parameters, differ from a run with
    --light encoded, and the --y4m frames are the restatement of the video conversion (tests/yuv_ref.py) applied to those PNGs' pixels"""
    from PIL import Image
    import yuv_ref
    from test_host_yuv import parse_y4m
    from view_rows import run_cli
    w, h, n = 18, 6, 4
    args = ["--synthetic", f"3,3,{w},{h}", "-t", "0,0,1,1", "-m", method, "-n", str(n), "-b", "1", "-f", "0.2"]
    encoded, linear, y4m = tmp_path / "encoded", tmp_path / "linear", tmp_path / "v.y4m"
    res = run_cli(gpu, *args, "-o", str(encoded), "--light", "encoded")
    assert res.returncode == 0 and "linear-light blending" not in res.stdout, res.stderr
    res = run_cli(gpu, *args, "-o", str(linear), "--light", "linear", "--y4m", str(y4m))
    assert res.returncode == 0, (res.stdout, res.stderr)
    assert res.stdout.count("linear-light blending") == 1
    want = np.stack([np.array(Image.open(encoded / f"{v:02d}.png")) for v in range(n)])
    got = np.stack([np.array(Image.open(linear / f"{v:02d}.png")) for v in range(n)])
    assert (got != want).mean() > 0.05
    hp = gpu.build_params(3, 3, w, h, "0,0,1,1", 0.2, 0.0, 3.0, 1.0, n)
    ctx = gpu.Context(0)
    ctx.set_grid(3, 3, w, h)
    ctx.fill_synthetic(ref.SEED)
    ctx.set_output_layout("planar")
    ctx.set_params(hp, flags=FLAG)
    poison.render(ctx, method)
    api = ctx.download_views()
    ctx.close()
    assert (got == api).all()
    if method == "STD":
        assert (api[..., :3] == ref.restate(oc.synthetic_lf(9, w, h, ref.SEED), hp).bytes).all()
    tags, frames = parse_y4m(y4m.read_bytes())
    assert len(frames) == n
    for v, frame in enumerate(frames):
        assert (frame == yuv_ref.frame(got[v], yuv_ref.BT709, yuv_ref.LIMITED)).all(), v
