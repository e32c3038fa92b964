"""Every row of the dispatch-coverage table (tests/test_gpu_dispatch_coverage.py MATRIX) rendered under a row window, against the oracle.

Row windows (lfi_set_row_window) are how a frame is sharded over GPUs; every persistent blend kernel carries in_y0, in_rows, out_y0 and
out_rows by hand through its row arithmetic (sampled rows clamp(y + oy, 0, H − 1) − in_y0, plane strides in_rows × pitch and out_rows ×
pitch, n_tiles = tiles_x × out_rows).  Here each row of the table that a window admits renders the bands of its plan
(tests/dispatch_windows.py; the plans' conditions are held on the CPU by tests/test_dispatch_windows_table.py) in fresh windowed contexts,
under both poison bytes, with the table's own contract and no other tolerance: the kernel's name unchanged by the window, the band's rows
against the oracle's whole-frame render at the plan's height (STD ==, TEN_WM within one LSB of M16 and inside the interval of the exact
sum, dyadic rows ε = 0), the rows outside the band zero, the views outside the range still poisoned.  Rows marked persistent render one
interior band of more than 2 × CUs tiles: the tile loops and both tile orders with out_rows ≠ H and out_y0 ≠ 0.

The five generic kernels address whole planes and are refused under a window; the refusal, and that it leaves the context as it was, is
asserted for each of their rows.
"""
import dataclasses

import numpy as np
import pytest

import dispatch_windows as dw
import poison
import test_gpu_dispatch_coverage as dc


@pytest.mark.gpu
@pytest.mark.parametrize("row", dw.WINDOWED, ids=lambda r: r.name)
def test_dispatch_row_under_a_row_window(row, gpu, oracle_c):
    cu = dc._cu_count()
    H, bands, hp, lf, m = dw.window_plan(gpu, oracle_c, row, cu)
    if row.persistent:
        (o0, o1, _, _), = bands
        tiles = (row.W + row.persistent - 1) // row.persistent * (o1 - o0)
        assert tiles > 2 * cu, (tiles, cu)
    want, tol, S, eps, lo, hi = dc.row_expected(oracle_c, row, hp, lf, m)
    outside = None if row.V <= 80 else [0, row.v0 - 1, row.v1, row.V - 1]
    union = {b: np.zeros_like(want) for b in poison.POISON}
    for o0, o1, i0, i1 in bands:
        tag = f"[{o0}:{o1}|{i0}:{i1}/{H}]"
        ctx = dc.row_context(gpu, row, hp, lf, m, H, window=(o0, o1, i0, i1))

        def band(a):   # the band's rows of a [views][H][W][…] array of row_expected
            return None if a is None else a[:, o0:o1]

        def check(byte):
            got = poison.render_range(ctx, row.method, row.v0, row.v1, all_focus=row.all_focus, byte=byte, outside=outside,
                                      inspect=(lambda: dc.check_paths(ctx, row)) if byte == poison.POISON[0] else None)
            assert ctx.last_kernel_name() == row.expect, (row.name, tag, ctx.last_kernel_name())
            assert got.shape == want.shape
            dc.check_rendered(row, tag, byte, got[:, o0:o1], band(want), tol, band(S), eps, band(lo), band(hi))
            assert not got[:, :o0].any() and not got[:, o1:].any(), (row.name, tag, "rows outside the band were downloaded")
            union[byte] |= got
        poison.twice(check)
        ctx.close()
    if len(bands) > 1:
        # the three bands tile [0, H): together they are the whole frame
        for byte, got in union.items():
            dc.check_rendered(row, f"[0:{H}]", byte, got, want, tol, S, eps, lo, hi)


@pytest.mark.gpu
@pytest.mark.parametrize("row", dw.REFUSED, ids=lambda r: r.name)
def test_generic_kernels_are_refused_under_a_row_window(row, gpu, oracle_c):
    """The rows that reach a generic kernel — by variant, by LFI_FLAG_TEN_ROUND_PER_BATCH or by weights outside [0, 2) under TEN_WM — in an
    interior band: the render is refused, writes nothing and allocates nothing; the same context renders the band once the variant is the
    default, the flags are 0 and the weights are build_params' own."""
    served = dataclasses.replace(row, method="STD", variant="auto", flags=0, weights="default", expect="(a windowed kernel)")
    H, bands, hp_ok, lf, m = dw.window_plan(gpu, oracle_c, served, dc._cu_count())
    hp = dc.row_inputs(gpu, oracle_c, row, H)[0]     # the same images: they depend on the shape alone
    o0, o1, i0, i1 = bands[1]
    assert 0 < i0 < o0 and o1 < i1 < H
    ctx = dc.row_context(gpu, row, hp, lf, m, H, window=(o0, o1, i0, i1))

    def state():
        mi = ctx.memory_info()
        return {name: getattr(mi, name) for name, _ in mi._fields_}
    for byte in poison.POISON:
        ctx.poison(poison.RENDER, byte)
        ctx.sync()
        before = state()
        with pytest.raises(gpu.LfiError, match=dw.REFUSAL):
            ctx.render(row.method, all_focus=row.all_focus, v0=row.v0, v1=row.v1)
        ctx.sync()
        assert state() == before, (row.name, "the refused render changed lfi_memory_info", before, state())
        assert poison.written_outside(ctx, 0, 0, byte) == [], (row.name, "the refused render wrote views")
    ctx.set_variant(row.method, "auto")
    ctx.set_params(hp_ok, 0)
    want = oracle_c.blend_std(lf, hp_ok.focused_offsets, hp_ok.offsets, hp_ok.weights, v0=row.v0, v1=row.v1, threads=dc.THREADS,
                              all_focus=row.all_focus, map_plane=m, focus=hp_ok.focus, rng=hp_ok.range)[row.v0:row.v1]

    def check(byte):
        got = poison.render_range(ctx, "STD", row.v0, row.v1, all_focus=row.all_focus, byte=byte)
        assert ctx.last_kernel_name() not in dw.GENERIC, ctx.last_kernel_name()
        assert (got[:, o0:o1] == want[:, o0:o1]).all(), (row.name, hex(byte), poison.mismatch(got[:, o0:o1], want[:, o0:o1]))
        assert not got[:, :o0].any() and not got[:, o1:].any()
    poison.twice(check)
    ctx.close()
