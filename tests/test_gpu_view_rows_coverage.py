"""Per-view-rows coverage: every kernel launch_view_rows (csrc/hip/lfi_dispatch.hpp) can launch — blend_vfocus and blend_vfocus_af in all
16 template forms — at the shapes, view ranges, sources and weights of the table in tests/view_rows.py, compared against the oracle under
poison (tests/poison.py).

Every row renders for both methods and twice, under both poison bytes: views outside the range must still hold the poison, the kernel name
must be the row's, STD is byte for byte the oracle's, TEN_WM within one LSB of M16 (not for `wide` weights, where M16's per-batch rounding
is not the contract of an fp32-accumulating kernel) and inside the interval of the exact sum (tests/ten_interval.py); rows with `dyadic`
weights have no accumulation error, so their interval is one value: the exact model byte for byte, fp16 ties included.  The CPU side of the
table (its names, its edges, the interval's own width) is tests/test_view_rows_table.py."""
import numpy as np
import pytest

import poison
import ten_interval
import view_rows as vr

pytestmark = pytest.mark.gpu


def make_context(gpu, row, inp):
    """A fresh context with the row's per-view rows (and maps) set, after the row's `before` step."""
    ctx = gpu.Context(0)
    ctx.set_grid(row.cols, row.rows, row.W, row.H)
    if row.window:
        ctx.set_row_window(row.window[0], row.window[1], *inp.in_rows)
    ctx.upload_grid(inp.lf)
    ctx.set_output_layout(row.layout)
    if row.before == "plain":
        # the planar copy built for the small offsets of a plain render; the per-view offsets set next reach further: it has to grow
        ctx.set_params(inp.hp_before)
        ctx.render("TEN_WM")
        ctx.sync()
        assert ctx.derived_layout().reach < int(np.abs(inp.offsets[..., 0]).max())
    ctx.set_params(inp.hp, row.flags)
    if row.before == "release":
        ctx.prepare("TEN_WM")
        ctx.release_inputs()
    if row.source == "rgba":
        ctx.grid_device_ptr()   # handed out and not marked modified: the RGBA planes are read directly
    if row.kind == "int":
        ctx.set_view_offsets(inp.offsets)
        return ctx
    ctx.set_view_float_offsets(inp.offsets)
    if row.kind == "float":
        for k in (0, 1):
            ctx.upload_map(k, inp.maps[k])
    else:
        ctx.view_focus_maps(inp.ids)
        for v, pair in inp.maps.items():
            for k in (0, 1):
                ctx.upload_view_map(v, k, pair[k])
    return ctx


def check_render(ctx, row, method, want, byte, label=None):
    """One poisoned render of the row's view range against `want` (view_rows.expected).  Returns the number of bytes outside the interval
    (TEN_WM) or off the oracle (STD) after printing the figures; the caller asserts."""
    y0, y1 = row.window if row.window else (0, row.H)
    outside_views = None if row.V <= 80 else [0, row.v0 - 1, row.v1, row.V - 1]
    got = poison.render_range(ctx, method, row.v0, row.v1, all_focus=row.kind != "int", byte=byte, outside=outside_views)[:, y0:y1]
    name = ctx.last_kernel_name()
    assert name == row.expect(method), (row.name, name)
    if method == "STD":
        bad = poison.mismatch(got, want.std)
        assert bad == 0, (row.name, hex(byte), bad)
        return
    if row.weights != "wide":
        bad = poison.mismatch(got, want.m16, vr.TEN_TOL_LSB)
        assert bad == 0, (row.name, hex(byte), bad)
    out = ten_interval.outside(got, want.lo, want.hi)
    differ = int((got[..., :3] != ten_interval.quantise(want.S)).sum())
    print(f"TEN_INTERVAL {label or row.name} {name} {hex(byte)} bytes={want.lo.size} differ_from_exact={differ} outside={out}")
    assert out == 0, (row.name, hex(byte), out, "needed multiples of eps, largest:", float(ten_interval.report(got, want.S, want.eps).max()))


@pytest.mark.parametrize("method", vr.METHODS)
@pytest.mark.parametrize("row", vr.VIEW_MATRIX, ids=lambda r: r.name)
def test_view_row(row, method, gpu, oracle_c):
    inp = vr.row_inputs(gpu, oracle_c, row)
    want = vr.expected(gpu, oracle_c, row, method)
    ctx = make_context(gpu, row, inp)
    poison.twice(lambda byte: check_render(ctx, row, method, want, byte))
    if row.kind == "int" and row.source == "planar":
        # the copy the launch read is padded for every per-view shift
        assert ctx.derived_layout().reach >= int(np.abs(inp.oracle_offsets[..., 0]).max()), row.name
    ctx.close()
