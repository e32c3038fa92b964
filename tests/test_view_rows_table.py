"""CPU: the per-view-rows coverage table (tests/view_rows.py VIEW_MATRIX) held to the code it covers, before the GPU test leans on it.

launch_view_rows reports its kernel through a names[4][2] table indexed at run time, so no string literal stands in its note_kernel call
and test_gpu_dispatch_coverage's name check cannot see it.  Here: every name of that table and every (name, view layout) pair — the 16
template instantiations — has a row, and every note_kernel call under csrc/hip/ is either a literal one or this indexed table; the rows
reach the edges that follow from the kernels' tile constants, which are read from the headers (a changed constant fails here instead of
silently un-edging the rows); the interval of the exact sum stays narrow enough to be a check on every TEN_WM row's own inputs (a condition
on the reference alone); and the interval reports a gather defect in the last partial quad of one view that both older clauses of
view_rows.check_views let through."""
import os
import re

import numpy as np
import pytest

import poison
import ten_interval as ti
import view_rows as vr
from conftest import ROOT

HIP_DIR = os.path.join(ROOT, "lfinterpolator_amd", "csrc", "hip")
TWO_VALUED_CAP = 0.02


def _read(name):
    with open(os.path.join(HIP_DIR, name)) as f:
        return f.read()


def _names_table():
    """The names[4][2] initialiser of launch_view_rows, in order."""
    text = _read("lfi_dispatch.hpp")
    body = text[text.index("int launch_view_rows(lfi_ctx *c, ViewRowsKind k, int method, int all_focus, const KernelArgs &a_in)\n{"):]
    m = re.search(r"names\[4\]\[2\]\s*=\s*\{(.*?)\};", body, flags=re.S)
    assert m, "launch_view_rows no longer holds a names[4][2] table"
    return re.findall(r'"([^"]+)"', m.group(1))


def test_every_view_rows_kernel_and_layout_has_a_row():
    names = _names_table()
    assert len(names) == 8 and len(set(names)) == 8, names
    assert len({r.name for r in vr.VIEW_MATRIX}) == len(vr.VIEW_MATRIX)
    covered = {(r.expect(m), r.layout) for r in vr.VIEW_MATRIX for m in vr.METHODS}
    missing = sorted({(n, lay) for n in names for lay in ("rgba", "planar")} - covered)
    assert not missing, f"kernel and view layout without a row in tests/view_rows.py VIEW_MATRIX: {missing}"
    unknown = sorted({k for k, _ in covered} - set(names))
    assert not unknown, f"rows name kernels launch_view_rows cannot report: {unknown}"
    assert len(covered) == 16


def test_every_note_kernel_call_is_a_literal_or_the_view_rows_table():
    """A note_kernel call without a string literal escapes test_gpu_dispatch_coverage's name check; the one known form is launch_view_rows'
    indexed table, covered above.  A third form fails here until someone covers it."""
    calls = indexed = 0
    for f in sorted(os.listdir(HIP_DIR)):
        if not f.endswith((".hpp", ".hip")):
            continue
        text = _read(f)
        found = re.findall(r"note_kernel\(\s*c\s*,(.*?)\);", text, flags=re.S)
        # every use but the definition itself has this form
        assert len(found) == len(re.findall(r"\bnote_kernel\(", text)) - len(re.findall(r"void note_kernel\(", text)), f
        for arg in found:
            calls += 1
            if re.search(r'"[^"]+"', arg):
                continue
            assert f == "lfi_dispatch.hpp" and re.fullmatch(r"\s*names\[[^;]*\]\[ten\]", arg), (f, arg)
            indexed += 1
    assert calls >= 14 and indexed == 1, (calls, indexed)


def _constants():
    """VF_TILE_W, VF_PX, VF_ROWS, VF_VIEWS and VM_VIEWS as the headers define them (integers and products of earlier constants)."""
    out = {}
    for header in ("blend_vfocus.hpp", "blend_vfocus_af.hpp"):
        for name, expr in re.findall(r"constexpr int (V[FM]_\w+) = ([^;]+);", _read(header)):
            value = 1
            for factor in expr.split("*"):
                factor = factor.strip()
                value *= out[factor] if factor in out else int(factor)
            out[name] = value
    assert set(out) == {"VF_TILE_W", "VF_PX", "VF_ROWS", "VF_VIEWS", "VM_VIEWS"}, out
    return out


@pytest.mark.parametrize("kind", vr.KINDS)
def test_rows_reach_the_tile_edges(kind):
    c = _constants()
    tile, px, rows_per_wg = c["VF_TILE_W"], c["VF_PX"], c["VF_ROWS"]
    views = c["VM_VIEWS"] if kind == "view_maps" else c["VF_VIEWS"]
    rows = [r for r in vr.VIEW_MATRIX if r.kind == kind]
    widths = {r.W for r in rows}
    assert {r.W % tile for r in rows} >= {0, 1, tile - 1}, (kind, sorted({r.W % tile for r in rows}))
    # … at the first tile boundary itself, and the smallest width of three tiles: a tile constant that changes moves these widths, and a
    # remainder that still happens to fit must not pass for the edge
    assert widths >= {tile - 1, tile, tile + 1, 2 * tile + 1}, (kind, tile, sorted(widths))
    assert any(r.W % px for r in rows), kind                                   # a partial quad at the end of a row
    assert {r.W % px for r in rows} >= {1, px - 1}, (kind, px)                 # … of one pixel, and of all but one
    assert any((r.W + tile - 1) // tile >= 3 for r in rows), kind
    assert any(r.out_rows % rows_per_wg for r in rows), kind                   # a workgroup whose last waves have no row
    assert {r.out_rows % rows_per_wg for r in rows} >= {1, rows_per_wg - 1}, (kind, rows_per_wg)
    assert any(r.v0 % views and r.v1 == r.V and r.V % 64 == 0 for r in rows), kind   # the last chunk reads the padding views
    assert any((r.v1 - r.v0) % views for r in rows), kind
    assert {r.v1 - r.v0 for r in rows} >= {views, views + 1}, (kind, views)    # exactly one chunk, and one view more
    assert {r.chunks for r in rows} >= {1, 2, 3, 4}, kind
    assert {r.layout for r in rows} == {"rgba", "planar"}, kind
    assert any(r.weights == "dyadic" for r in rows), kind


@pytest.mark.parametrize("row", vr.VIEW_MATRIX, ids=lambda r: r.name)
def test_interval_stays_a_check_on_every_view_row(row, native, oracle_c):
    """A condition on the reference alone, not a measurement of a kernel: on the row's own inputs at most 2 % of the bytes have two admissible
    values, none has three, and the exact model lies inside; a dyadic row's interval is one value (view_rows.expected asserts its
    preconditions: multiples of 2^-12, sums ≤ 2, enough fp16 ties)."""
    want = vr.expected(native, oracle_c, row, "TEN_WM")
    width = want.hi.astype(int) - want.lo.astype(int)
    share = (width == 1).mean()
    print(f"TEN_INTERVAL_CPU {row.name} k_pad={(row.n + 15) // 16 * 16} two_valued={share:.4%} widest={width.max()} ties={want.ties}")
    assert width.min() >= 0 and width.max() <= 1, (row.name, width.min(), width.max())
    assert share <= TWO_VALUED_CAP, (row.name, share)
    q = ti.quantise(want.S)
    assert ((want.lo <= q) & (q <= want.hi)).all()
    k_pad = (row.n + 15) // 16 * 16
    if row.weights == "dyadic":
        assert (want.eps == 0).all() and (want.lo == want.hi).all() and want.ties >= vr.DYADIC_TIES
    elif row.weights == "default":
        assert (want.eps == k_pad * 2.0 ** -15).all()
    else:
        assert (want.eps > k_pad * 2.0 ** -15).all()
    if row.weights != "wide":
        assert poison.mismatch(np.concatenate([q, np.full(q.shape[:-1] + (1,), 255, np.uint8)], -1), want.m16, 1) == 0


@pytest.mark.parametrize("grid", [(15, 15), (12, 12)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_interval_reports_a_neighbouring_views_offset_in_the_last_quad(grid, native, oracle_c):
    """The defect of a gather kernel with a partial store path and a chunk tail: in one view, one image takes its offset from the next view's
    row, but only in the last partial quad of the pixel rows (columns 256…258 of 259).  For some (view, image) every byte stays within one
    LSB of M16 and fewer than 1e-3 of all bytes differ from the exact model — both older clauses of check_views pass — while bytes leave the
    interval of the exact sum.  (The mutant's sums follow from the exact ones by linearity: one image's term replaced, exact in double.)"""
    L, oc = native, oracle_c
    cols, rows = grid
    W, H, V, n = 259, 5, 9, cols * rows
    x0 = W // 4 * 4
    hp = L.build_params(cols, rows, W, H, vr.TRAJ, 0.0, 0.0, vr.EFFECT, vr.ASPECT, V)
    D = L.build_view_offsets(cols, rows, W, H, vr.TRAJ, vr.ASPECT, L.focus_ramp(0.0, 0.6, V))
    lf = oc.synthetic_lf(n, W, H, 0x5EED + n + W)
    want = [vr.ten_want(oc, lf, D[v], hp.offsets, hp.weights[v:v + 1]) for v in range(V)]
    m16, exact, S = (np.stack([w[k] for w in want]) for k in range(3))
    eps = np.array([w[3] for w in want])
    lo, hi = ti.interval(S, eps)
    assert ti.outside(exact, lo, hi) == 0

    def term(v, g, row_of):
        """w[v][g] · image g sampled at D[row_of][g]: one image's part of view v's exact sums."""
        return oc.blend_f64(lf[g:g + 1], D[row_of, g:g + 1], hp.offsets[g:g + 1], hp.weights[v:v + 1, g:g + 1])[0]

    found, old_fails = [], 0
    for v in range(V):
        other = v + 1 if v + 1 < V else v - 1
        for g in range(n):
            if (D[v, g] == D[other, g]).all():
                continue
            s = S[v].copy()
            s[:, x0:] += (term(v, g, other) - term(v, g, v))[:, x0:]
            mut = exact.copy()
            mut[v, ..., :3] = ti.quantise(s)
            if not (mut != exact).any():
                continue
            old_passes = np.abs(mut.astype(int) - m16.astype(int)).max() <= vr.TEN_TOL_LSB and (mut != exact).mean() < 1e-3
            out = ti.outside(mut, lo, hi)
            if old_passes and out:
                found.append((v, g, out))
            old_fails += not old_passes
    assert found
    # the linearity the search rests on, checked on the first mutant found: the oracle's own sums with image g's offset replaced
    v, g, _ = found[0]
    Dm = D[v].copy()
    Dm[g] = D[v + 1 if v + 1 < V else v - 1, g]
    direct = oc.blend_f64(lf, Dm, hp.offsets, hp.weights[v:v + 1])[0]
    assert (direct[:, x0:] == (S[v] + term(v, g, v + 1 if v + 1 < V else v - 1) - term(v, g, v))[:, x0:]).all()
    images = len({g for _, g, _ in found})
    print(f"TEN_INTERVAL_CPU {cols}x{rows} {W}x{H} V={V}: {len(found)} (view, image) mutants of the last quad pass the older clauses and leave "
          f"the interval ({images} of {n} images = {images / n:.1%}; most bytes outside: {max((o for _, _, o in found), default=0)}); "
          f"{old_fails} are caught by the older clauses")
