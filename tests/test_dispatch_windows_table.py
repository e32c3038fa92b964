"""CPU: the window plans of tests/dispatch_windows.py held to their conditions, before tests/test_gpu_dispatch_windows.py leans on them.

Conditions on the inputs and on the reference alone, none a measurement of a kernel: every band's four window values and the image height
exclude every whole-image assumption (an interior band with in_y0, in_rows, out_y0, out_rows and H_w five different numbers; a top and a
bottom band whose clamps happen inside the held rows); the oracle's picture changes from every row to the next, so that a kernel indexing
the held rows off by one cannot pass; the interval of the exact sum stays narrow enough to be a check at every plan's height; and the
windowed rows reach every kernel and every template form the unwindowed table reaches, the five generic kernels excepted (refused under
a window, which the GPU module asserts)."""
import re

import pytest

import dispatch_windows as dw
import ten_interval as ti
import test_gpu_dispatch_coverage as dc
from test_ten_interval import TWO_VALUED_CAP

CU = 256                  # the MI355X's; the GPU test sizes the persistent bands by the device's own count
ROWS_DIFFER_SHARE = 0.5   # of a view row's bytes, from the row above it


@pytest.fixture(scope="module")
def plans(native, oracle_c):
    made = {}

    def get(row):
        if row.name not in made:
            made[row.name] = dw.window_plan(native, oracle_c, row, CU)
        return made[row.name]
    return get


@pytest.mark.parametrize("row", dw.WINDOWED, ids=lambda r: r.name)
def test_window_plan_excludes_every_whole_image_assumption(row, plans, native):
    H, bands, hp, lf, m = plans(row)
    assert lf.shape == (row.n, H, row.W, 4) and (m is None) == (not row.all_focus)
    above, below = dw.uses_negative_and_positive_oy(row, hp)
    interior = top = bottom = 0
    for o0, o1, i0, i1 in bands:
        assert 0 <= i0 <= o0 < o1 <= i1 <= H
        assert i1 - i0 < H, (row.name, "a band holds every input row", (o0, o1, i0, i1))
        # the library's own test at lfi_set_params: the rows the band samples at the integer focused offsets are held
        assert native.input_rows((o0, o1), hp.focused_offsets, H)[0] >= i0 and native.input_rows((o0, o1), hp.focused_offsets, H)[1] <= i1
        if 0 < i0 < o0 and o1 < i1 < H:
            interior += 1
            assert len({i0, i1 - i0, o0, o1 - o0, H}) == 5, (row.name, (o0, o1, i0, i1), H)
        elif o0 == i0 == 0:
            top += 1
            assert above, (row.name, "no image is sampled above its pixel: the clamp at row 0 is never taken")
        elif o1 == i1 == H:
            bottom += 1
            assert below, (row.name, "no image is sampled below its pixel: the clamp at the last row is never taken")
        else:
            pytest.fail(f"{row.name}: band {(o0, o1, i0, i1)} of {H} rows is neither interior, top nor bottom")
    if row.persistent:
        assert (interior, top, bottom) == (1, 0, 0)
        o0, o1 = bands[0][:2]
        tiles = (row.W + row.persistent - 1) // row.persistent * (o1 - o0)
        assert tiles > 2 * CU, (row.name, tiles)
    else:
        assert (interior, top, bottom) == (1, 1, 1)
        outs = [b[:2] for b in bands]
        assert outs[0][0] == 0 and outs[-1][1] == H and all(a[1] == b[0] for a, b in zip(outs, outs[1:])), outs
        assert len({o1 - o0 for o0, o1 in outs}) == 3, outs
        # the smallest such height: moved up or down by the three rows that keeping the heights unequal may add, the middle band is no
        # longer interior
        m0, m1 = outs[1]
        hp_first = dc.xcd_first_params(native, row, H) if row.order == "xcd" else None
        assert dw.held_rows(native, row, hp, (m0 - 3, m1 - 3), H, hp_first)[0] == 0
        assert dw.held_rows(native, row, hp, (m0 + 3, m1 + 3), H, hp_first)[1] == H


@pytest.mark.parametrize("row", dw.WINDOWED, ids=lambda r: r.name)
def test_windowed_render_can_fail(row, plans, oracle_c):
    """More than half of the bytes of every row of the oracle's STD views differ from the row above: held rows indexed one off, or a
    band written one row off, cannot give the right picture.  (The first two views of the row's range.)"""
    H, bands, hp, lf, m = plans(row)
    v1 = min(row.v0 + 2, row.v1)
    want = oracle_c.blend_std(lf, hp.focused_offsets, hp.offsets, hp.weights, v0=row.v0, v1=v1, threads=dc.THREADS, all_focus=row.all_focus,
                              map_plane=m, focus=hp.focus, rng=hp.range)[row.v0:v1]
    share = (want[:, 1:, :, :3] != want[:, :-1, :, :3]).mean(axis=(0, 2, 3))
    print(f"WINDOW_TEETH {row.name} H_w={H} rows differing from the row above: min {share.min():.3f} mean {share.mean():.3f}")
    assert share.shape == (H - 1,) and share.min() > ROWS_DIFFER_SHARE, (row.name, int(share.argmin()) + 1, float(share.min()))


TEN_ROWS = [r for r in dw.WINDOWED if r.method == "TEN_WM" and not r.flags & dc.ROUND and not r.persistent]


@pytest.mark.parametrize("row", TEN_ROWS, ids=lambda r: r.name)
def test_interval_stays_a_check_at_the_window_height(row, plans, oracle_c):
    """tests/test_ten_interval.py's condition at the plan's own height (its persistent rows are held to it at a representative height
    there): at most TWO_VALUED_CAP of the bytes have two admissible values, none has three."""
    H, bands, hp, lf, m = plans(row)
    S, eps, lo, hi = (a[row.v0:row.v1] for a in dc.ten_row_interval(oracle_c, row, hp, lf, m))
    width = hi.astype(int) - lo.astype(int)
    print(f"TEN_INTERVAL_CPU {row.name} H_w={H} two_valued={(width == 1).mean():.4%} widest={width.max()}")
    assert width.min() >= 0 and width.max() <= 1, (row.name, width.min(), width.max())
    assert (width == 1).mean() <= TWO_VALUED_CAP, (row.name, (width == 1).mean())
    q = ti.quantise(S)
    assert ((lo <= q) & (q <= hi)).all()


def test_windowed_rows_reach_what_the_table_reaches():
    """Every kernel of MATRIX but the generic five is rendered under a window, in every (layout, chunks) form
    test_matrix_reaches_every_chunk_count_and_output_form lists, with a persistent row where that test demands one."""
    assert dw.GENERIC == {r.expect for r in dw.REFUSED} and len(dw.REFUSED) + len(dw.WINDOWED) == len(dc.MATRIX)
    assert {r.expect for r in dw.WINDOWED} == {r.expect for r in dc.MATRIX} - dw.GENERIC - dc.MEASUREMENT_ONLY
    # the refusal's own text and its list of kernels, as lfi_dispatch.hpp has them
    text = open(dc.HIP_DIR + "/lfi_dispatch.hpp").read()
    assert text.count(dw.REFUSAL) == 1
    body = text[text.index("bool generic_kernel(BlendKernel k)"):]
    body = body[:body.index("}")]
    assert sorted("blend_" + k for k in set(re.findall(r"K::(\w+)", body))) == sorted(dw.GENERIC)

    def forms(kernel, layout=None):
        return {r.chunks for r in dw.WINDOWED if r.expect == kernel and (layout is None or r.layout == layout)}

    def table_forms(kernel, layout=None):
        return {r.chunks for r in dc.MATRIX if r.expect == kernel and (layout is None or r.layout == layout)}
    for kernel in sorted({r.expect for r in dw.WINDOWED}):
        for layout in ("rgba", "planar"):
            assert forms(kernel, layout) == table_forms(kernel, layout), (kernel, layout)
    assert forms("blend_p3<TEN_WM>") == {1, 2, 3, 4}
    assert forms("blend_p3<TEN_WM,rgba>") == {2, 3, 4}
    assert forms("blend_stdx<STD>", "planar") == {1, 2, 3, 4}
    assert forms("blend_stdx<STD>", "rgba") == {2, 3, 4}
    assert forms("blend_stdxa<STD,allfocus>", "planar") == {1, 2, 3, 4}
    assert forms("blend_stdxa<STD,allfocus>", "rgba") == {1, 2, 3, 4}
    assert forms("blend_afs<STD,allfocus>") == {3, 4}
    p3_one = [r for r in dw.WINDOWED if r.expect == "blend_p3<TEN_WM>" and r.chunks == 1]
    assert any(r.v1 - r.v0 <= 64 for r in p3_one) and any(64 < r.v1 - r.v0 <= 256 for r in p3_one) and any(r.v1 - r.v0 > 256 for r in p3_one)
    for kernel in ("blend_p3<TEN_WM>", "blend_p3<TEN_WM,rgba>", "blend_stdx<STD>", "blend_stdxa<STD,allfocus>", "blend_afs<STD,allfocus>",
                   "blend_persist<TEN_WM,allfocus>", "blend_persist<STD>", "blend_planar<TEN_WM>", "blend_planar<STDF>"):
        assert any(r.persistent for r in dw.WINDOWED if r.expect == kernel), kernel
    assert {r.order for r in dw.WINDOWED if r.expect == "blend_p3<TEN_WM>" and r.persistent} == {"plain", "xcd"}
    assert {r.layout for r in dw.WINDOWED if r.far} == {"rgba", "planar"}
    assert dc.WRITES_PLANES <= {r.expect for r in dw.WINDOWED if r.layout == "planar" and not r.scratch}
    assert dc.READS_COPY <= {r.expect for r in dw.WINDOWED}
    # what the suite had never rendered under a window: weights outside [0, 2) with STD, a view range off blend_p3, dyadic rows
    assert any(r.weights == "wide" for r in dw.WINDOWED) and any(r.weights == "dyadic" for r in dw.WINDOWED)
    assert any((r.v0, r.v1) != (0, r.V) and not r.expect.startswith("blend_p3") for r in dw.WINDOWED)
