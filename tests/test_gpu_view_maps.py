"""GPU (-m gpu): per-view focus maps (lfi_view_focus_maps) — every view of a view-centred all-focus render reads a map estimated at its own
camera, as the reference's focusMapCompare.sh second run does per camera.

View v's map 0 is the oracle's focus_estimate with the view's float offsets O[v] and its ids (build_view_focus_ids row v), map 1 its
focus_filter; view v of an all-focus render is the oracle's all-focus render of weight row v at O[v] over view v's own map: STD byte for byte,
TEN_WM within the TEN_WM contract (≤ 1 LSB from M16, < 1e-3 of the bytes off the exactly-summed model, every byte inside the interval of the
exact sum: tests/ten_interval.py).  Every map and view a check reads was poisoned first; the render kernel's shapes and edges are the table
of tests/view_rows.py (tests/test_gpu_view_rows_coverage.py)."""
import dataclasses
import os

import numpy as np
import pytest

import lfinterpolator_amd as L
import poison
from conftest import SEED
from test_gpu_view_centres import CASES, _random_maps
from view_rows import check_views, run_cli, ten_want

pytestmark = pytest.mark.gpu

KERNEL = {"STD": "blend_vfocus_af<STD,view_maps>", "TEN_WM": "blend_vfocus_af<TEN_WM,view_maps>"}
VIEW_MAPS = L.LFI_POISON_VIEW_MAPS | L.LFI_POISON_FOCUS_WORKSPACE
LFI_EINVAL = -1
_calls = [0]


def _byte():
    _calls[0] += 1
    return poison.POISON[_calls[0] & 1]


def _setup(gpu, oracle_c, case, layout="rgba", flags=0, views=None):
    name, cols, rows, W, H, traj, focus, rng_, V, aspect, effect = case
    V = V if views is None else views
    hp = gpu.build_params(cols, rows, W, H, traj, focus, rng_, effect, aspect, V)
    O, _ = gpu.build_view_centred_offsets(cols, rows, W, H, traj, aspect, np.full(V, focus, np.float32))
    ids = gpu.build_view_focus_ids(cols, rows, traj, V)
    lf = oracle_c.synthetic_lf(cols * rows, W, H, SEED)
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, W, H)
    ctx.fill_synthetic(SEED)
    ctx.set_params(hp, flags)
    ctx.set_output_layout(layout)
    ctx.set_view_float_offsets(O)
    return ctx, hp, O, ids, lf


def _estimate(ctx, ids, what=VIEW_MAPS):
    ctx.poison(what, _byte())
    ctx.view_focus_maps(ids)
    ctx.sync()


def _oracle_maps(oc, lf, O, ids, hp, v):
    m0 = oc.focus_estimate(lf, O[v], ids[v], hp.focus, hp.range, hp.block_radius, threads=8)
    return m0, oc.focus_filter(m0, hp.block_radius, threads=8)


def _check_maps(ctx, oc, lf, O, ids, hp, views=None):
    for v in (range(len(O)) if views is None else views):
        m0, m1 = _oracle_maps(oc, lf, O, ids, hp, v)
        assert (ctx.download_view_map(v, 0) == m0).all(), ("map 0", v)
        assert (ctx.download_view_map(v, 1) == m1).all(), ("map 1", v)


def _want_views(oc, lf, O, hp, method, maps_of, unified=False):
    """maps_of(v) -> (map0, map1) of view v; per view the oracle's STD view, or the TEN_WM (M16, exact, S, ε) tuple of check_views."""
    out = []
    for v in range(len(O)):
        m = maps_of(v)[1 if (method == "STD" or unified) else 0]
        kw = dict(all_focus=True, map_plane=m, focus=hp.focus, rng=hp.range)
        w = hp.weights[v:v + 1]
        if method == "STD":
            out.append(oc.blend_std(lf, hp.focused_offsets, O[v], w, **kw)[0])
        else:
            out.append(ten_want(oc, lf, hp.focused_offsets, O[v], w, **kw))
    return out


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_view_maps_match_the_oracle_per_camera(gpu, oracle_c, case):
    ctx, hp, O, ids, lf = _setup(gpu, oracle_c, case)
    _estimate(ctx, ids)
    _check_maps(ctx, oracle_c, lf, O, ids, hp)
    ctx.close()


# radius edges: W below 100 px (radius 1), an odd radius raised to even (W 150 → 2, H 250 → 2), and a tall image
@pytest.mark.parametrize("W,H", [(33, 17), (150, 250), (201, 9)])
def test_view_maps_at_radius_edges(gpu, oracle_c, W, H):
    case = ("radius", 4, 4, W, H, "0,0,1,1", 0.1, 0.6, 5, 1.0, 3.0)
    ctx, hp, O, ids, lf = _setup(gpu, oracle_c, case)
    _estimate(ctx, ids)
    _check_maps(ctx, oracle_c, lf, O, ids, hp)
    ctx.close()


RENDER_CASES = [c for c in CASES if c[0] in ("long_8x8", "diag_3x3_oddW", "diag_15x15", "wide_5x2_v70")]


@pytest.mark.parametrize("unified", [False, True], ids=["default_map", "unified_map"])
@pytest.mark.parametrize("map_kind", ["own", "random"])
@pytest.mark.parametrize("layout", ["rgba", "planar"])
@pytest.mark.parametrize("method", ["STD", "TEN_WM"])
@pytest.mark.parametrize("case", RENDER_CASES, ids=[c[0] for c in RENDER_CASES])
def test_render_reads_each_views_own_map(gpu, oracle_c, case, method, layout, map_kind, unified):
    ctx, hp, O, ids, lf = _setup(gpu, oracle_c, case, layout, gpu.LFI_FLAG_UNIFIED_FOCUS_MAP if unified else 0)
    _estimate(ctx, ids)
    if map_kind == "own":
        maps = {v: (ctx.download_view_map(v, 0), ctx.download_view_map(v, 1)) for v in range(len(O))}
        if case[0] != "long_8x8":   # (test_view_maps_match_the_oracle_per_camera checks every case's maps)
            _check_maps(ctx, oracle_c, lf, O, ids, hp, views=[0, len(O) - 1])
    else:
        maps = {v: tuple(_random_maps(ctx.height, ctx.width, 100 + v)) for v in range(len(O))}
        for v, pair in maps.items():
            for k in (0, 1):
                ctx.upload_view_map(v, k, pair[k])
    poison.render(ctx, method, all_focus=True)
    assert ctx.last_kernel_name() == KERNEL[method]
    check_views(ctx.download_views(), _want_views(oracle_c, lf, O, hp, method, lambda v: maps[v], unified), method)
    ctx.close()


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("long_8x8", "diag_15x15", "diag_3x3_oddW")], ids=lambda c: c[0])
def test_single_camera_equivalence(gpu, oracle_c, case):
    """focusMapCompare.sh's second run: one context per camera (offsets O[v], ids row v, weight row v, lfi_focus_map, one all-focus view)
    gives view v's maps and STD view byte for byte, and a TEN_WM view within the contract."""
    ctx, hp, O, ids, lf = _setup(gpu, oracle_c, case)
    _estimate(ctx, ids)
    poison.render(ctx, "STD", all_focus=True)
    std = ctx.download_views()
    poison.render(ctx, "TEN_WM", all_focus=True)
    ten = ctx.download_views()
    V = len(O)
    for v in sorted({0, V // 2, V - 1}):
        one = dataclasses.replace(hp, offsets=np.ascontiguousarray(O[v]), focus_map_ids=np.ascontiguousarray(ids[v]),
                                  weights=np.ascontiguousarray(hp.weights[v:v + 1]))
        c1 = gpu.Context(0)
        c1.set_grid(case[1], case[2], case[3], case[4])
        c1.fill_synthetic(SEED)
        c1.set_params(one)
        poison.focus_map(c1)
        for k in (0, 1):
            assert (c1.download_map(k) == ctx.download_view_map(v, k)).all(), (v, k)
        poison.render(c1, "STD", all_focus=True)
        assert (c1.download_view(0) == std[v]).all(), v
        poison.render(c1, "TEN_WM", all_focus=True)
        maps = (ctx.download_view_map(v, 0), ctx.download_view_map(v, 1))
        want = _want_views(oracle_c, lf, O[v:v + 1], dataclasses.replace(hp, weights=hp.weights[v:v + 1]), "TEN_WM", lambda _: maps)
        check_views(c1.download_views(), want, "TEN_WM")
        check_views(ten[v:v + 1], want, "TEN_WM")
        c1.close()
    ctx.close()


def test_order_of_ids_changes_no_byte(gpu, oracle_c):
    case = [c for c in CASES if c[0] == "diag_15x15"][0]
    ctx, hp, O, ids, lf = _setup(gpu, oracle_c, case)
    _estimate(ctx, ids)
    first = [(ctx.download_view_map(v, 0), ctx.download_view_map(v, 1)) for v in range(len(O))]
    rng = np.random.default_rng(5)
    perm = np.stack([rng.permutation(row) for row in ids])
    assert (perm != ids).any()
    _estimate(ctx, perm)
    for v in range(len(O)):
        assert (ctx.download_view_map(v, 0) == first[v][0]).all() and (ctx.download_view_map(v, 1) == first[v][1]).all(), v
    _check_maps(ctx, oracle_c, lf, O, perm, hp, views=[0, len(O) - 1])
    ctx.close()


def test_padded_planes_are_reused_correctly(gpu, oracle_c):
    """Two estimates with other rows and ids, one image replaced in between: the second pads only what it needs and is still exact."""
    cols, rows, W, H, V = 8, 8, 64, 48, 16
    case = ("reuse", cols, rows, W, H, "0,0,1,1", 0.0, 0.5, V, 1.0, 3.0)
    ctx, hp, O, ids, lf = _setup(gpu, oracle_c, case)
    _estimate(ctx, ids)
    _check_maps(ctx, oracle_c, lf, O, ids, hp, views=[0, V // 2, V - 1])
    # the reverse trajectory (shifts of the same size: the planes' geometry is kept), a sampled image replaced
    traj_b = "1,1,0,0"
    hp_b = gpu.build_params(cols, rows, W, H, traj_b, 0.0, 0.5, 3.0, 1.0, V)
    O_b, _ = gpu.build_view_centred_offsets(cols, rows, W, H, traj_b, 1.0, np.zeros(V, np.float32))
    ids_b = gpu.build_view_focus_ids(cols, rows, traj_b, V)
    g = int(ids_b[0][0])
    new = np.random.default_rng(9).integers(0, 256, (H, W, 4), dtype=np.uint8)
    ctx.upload_image(g, new)
    lf_b = lf.copy()
    lf_b[g] = new
    ctx.set_params(hp_b)
    ctx.set_view_float_offsets(O_b)
    _estimate(ctx, ids_b, what=L.LFI_POISON_VIEW_MAPS)   # (the workspace keeps its padded planes)
    _check_maps(ctx, oracle_c, lf_b, O_b, ids_b, hp_b)
    ctx.close()


def test_centre_map_is_unchanged(gpu, oracle_c):
    case = [c for c in CASES if c[0] == "long_8x8"][0]
    ctx, hp, O, ids, lf = _setup(gpu, oracle_c, case, views=16)
    poison.focus_map(ctx)
    before = [ctx.download_map(0), ctx.download_map(1)]
    _estimate(ctx, ids)
    poison.focus_map(ctx)
    after = [ctx.download_map(0), ctx.download_map(1)]
    assert all((b == a).all() for b, a in zip(before, after))
    # set_params clears the per-view maps: a view-centred render reads the centre's map again
    ctx.set_params(hp)
    ctx.set_view_float_offsets(O)
    poison.render(ctx, "STD", all_focus=True)
    assert ctx.last_kernel_name() == "blend_vfocus_af<STD>"
    check_views(ctx.download_views(), _want_views(oracle_c, lf, O, hp, "STD", lambda v: after), "STD")
    # a view-maps estimate, then new rows (the same rows): cleared again
    _estimate(ctx, ids)
    ctx.set_view_float_offsets(O)
    poison.render(ctx, "STD", all_focus=True)
    assert ctx.last_kernel_name() == "blend_vfocus_af<STD>"
    ctx.close()


def test_stream_order_without_host_waits(gpu, oracle_c):
    cols, rows, W, H, V = 8, 8, 64, 48, 12
    case = ("order", cols, rows, W, H, "0,0,1,1", 0.05, 0.5, V, 1.0, 3.0)
    ctx, hp, O_a, ids_a, lf = _setup(gpu, oracle_c, case)
    O_b, _ = gpu.build_view_centred_offsets(cols, rows, W, H, "0,1,1,0", 1.0, np.full(V, 0.05, np.float32))
    ids_b = gpu.build_view_focus_ids(cols, rows, "0,1,1,0", V)
    ctx.poison(VIEW_MAPS | poison.RENDER, _byte())
    ctx.view_focus_maps(ids_a)
    ctx.render("STD", all_focus=True)
    ctx.set_view_float_offsets(O_b)
    ctx.view_focus_maps(ids_b)
    got_a = ctx.download_views()
    maps_a = lambda v: _oracle_maps(oracle_c, lf, O_a, ids_a, hp, v)
    check_views(got_a, _want_views(oracle_c, lf, O_a, hp, "STD", maps_a), "STD")
    ctx.render("STD", all_focus=True)
    got_b = ctx.download_views()
    maps_b = lambda v: _oracle_maps(oracle_c, lf, O_b, ids_b, hp, v)
    check_views(got_b, _want_views(oracle_c, lf, O_b, hp, "STD", maps_b), "STD")
    _check_maps(ctx, oracle_c, lf, O_b, ids_b, hp)
    ctx.close()


def test_refusals(gpu, oracle_c):
    import ctypes as C
    case = ("refuse", 4, 4, 32, 16, "0,0,1,1", 0.1, 0.5, 4, 1.0, 3.0)
    ctx, hp, O, ids, lf = _setup(gpu, oracle_c, case)
    lib, h = ctx._lib, ctx._h

    def call(ids_vk, views=None, n=None):
        a = np.ascontiguousarray(ids_vk, dtype=np.int32)
        return lib.lfi_view_focus_maps(h, a.ctypes.data_as(C.c_void_p), a.shape[0] if views is None else views, a.shape[1] if n is None else n)

    assert call(ids, views=3) == LFI_EINVAL
    assert call(ids, n=0) == LFI_EINVAL
    assert call(np.zeros((4, 33), np.int32)) == LFI_EINVAL
    bad = ids.copy()
    bad[2, 1] = 16
    assert call(bad) == LFI_EINVAL
    bad[2, 1] = -1
    assert call(bad) == LFI_EINVAL
    assert lib.lfi_view_focus_maps(h, None, 4, ids.shape[1]) == LFI_EINVAL
    # no float rows
    ctx.set_view_float_offsets(None)
    assert call(ids) == LFI_EINVAL
    ctx.set_view_float_offsets(O)
    assert call(ids) == 0
    # the render-side refusals of the float rows stay
    with pytest.raises(gpu.LfiError):
        ctx.render_stream("STD", hp.weights, all_focus=True)
    with pytest.raises(gpu.LfiError):
        ctx.download_prequant("STD", 0, all_focus=True)
    ctx.set_params(hp, gpu.LFI_FLAG_TEN_ROUND_PER_BATCH)
    ctx.set_view_float_offsets(O)
    assert call(ids) == 0
    assert lib.lfi_render(h, gpu.LFI_METHOD_TEN_WM, 1, 0, 4) == LFI_EINVAL
    # range 0
    ctx.set_params(dataclasses.replace(hp, range=0.0))
    ctx.set_view_float_offsets(O)
    assert call(ids) == LFI_EINVAL
    # a row window
    ctx.set_row_window(0, 8, 0, 16)
    ctx.fill_synthetic(SEED)
    ctx.set_params(hp)
    ctx.set_view_float_offsets(O)
    assert call(ids) == LFI_EINVAL
    ctx.close()
    # released inputs
    ctx, hp, O, ids, lf = _setup(gpu, oracle_c, case)
    ctx.release_inputs()
    assert ctx._lib.lfi_view_focus_maps(ctx._h, ids.ctypes.data_as(C.c_void_p), 4, ids.shape[1]) == LFI_EINVAL
    ctx.close()


def test_full_size_8x8_1080p_64_views(gpu, oracle_c):
    cols, rows, W, H, V, traj = 8, 8, 1920, 1080, 64, "0,0,1,1"
    case = ("full", cols, rows, W, H, traj, 0.0, 0.5, V, 1.0, 3.0)
    ctx, hp, O, ids, lf = _setup(gpu, oracle_c, case)
    _estimate(ctx, ids)
    assert ctx.memory_info().maps_bytes >= 2 * W * H * 4 * (V + 1)
    poison.render(ctx, "STD", all_focus=True)
    assert ctx.last_kernel_name() == KERNEL["STD"]
    threads = min(os.cpu_count() or 1, 16)
    for v in (0, 31, 63):
        m0 = ctx.download_view_map(v, 0)
        m1 = ctx.download_view_map(v, 1)
        view = ctx.download_view(v)
        for y0, y1 in ((0, 2), (H // 2 - 1, H // 2 + 2), (H - 2, H)):
            want0 = oracle_c.focus_estimate(lf, O[v], ids[v], hp.focus, hp.range, hp.block_radius, threads=threads, rows=(y0, y1))
            assert (m0[y0:y1] == want0[y0:y1]).all(), ("map 0", v, y0)
            want1 = oracle_c.focus_filter(m0, hp.block_radius, threads=threads, rows=(y0, y1))   # the filter of the (verified) map 0
            assert (m1[y0:y1] == want1[y0:y1]).all(), ("map 1", v, y0)
            want = oracle_c.blend_std(lf, hp.focused_offsets, O[v], hp.weights[v:v + 1], all_focus=True, map_plane=m1, focus=hp.focus,
                                      rng=hp.range, threads=threads, rows=(y0, y1))[0]
            assert (view[y0:y1] == want[y0:y1]).all(), ("STD view", v, y0)
    ctx.close()


@pytest.mark.parametrize("method", ["STD", "TEN_WM"])
def test_cli_view_maps(gpu, oracle_c, tmp_path, method):
    from PIL import Image
    cols, rows, W, H, V, traj, f, r = 4, 4, 48, 20, 6, "0,0,1,1", 0.1, 0.3
    dst = tmp_path / "out"
    res = run_cli(gpu, "--synthetic", f"{cols},{rows},{W},{H}", "-t", traj, "-f", str(f), "-r", str(r), "-c", "--view-maps", "-n", str(V),
                  "-m", method, "-b", "2", "-o", str(dst))
    assert res.returncode == 0, res.stderr
    assert sorted(os.listdir(dst)) == sorted([f"{i:02d}.png" for i in range(V)] + [f"map{k}_{v:02d}.png" for v in range(V) for k in (0, 1)])
    hp = gpu.build_params(cols, rows, W, H, traj, f, r, 3.0, 1.0, V)
    O, _ = gpu.build_view_centred_offsets(cols, rows, W, H, traj, 1.0, np.full(V, f, np.float32))
    ids = gpu.build_view_focus_ids(cols, rows, traj, V)
    lf = oracle_c.synthetic_lf(cols * rows, W, H, SEED)
    maps = {v: _oracle_maps(oracle_c, lf, O, ids, hp, v) for v in range(V)}
    for v in range(V):
        for k in (0, 1):
            assert (np.array(Image.open(dst / f"map{k}_{v:02d}.png")) == maps[v][k]).all(), (v, k)
    got = np.stack([np.array(Image.open(dst / f"{v:02d}.png")) for v in range(V)])
    check_views(got, _want_views(oracle_c, lf, O, hp, method, lambda v: maps[v]), method)
