"""Row windows for the dispatch-coverage table: for every row of tests/test_gpu_dispatch_coverage.py MATRIX that a row window admits, an image
height H_w and the bands (out_y0, out_y1, in_y0, in_y1) it renders under lfi_set_row_window.

A kernel under a window carries in_y0, in_rows, out_y0 and out_rows by hand through its row arithmetic.  A band tests that arithmetic only
where the four values and the image height are five different numbers, so the heights here follow from each row's own vertical reach (the
offsets scale with the image WIDTH: ±17 rows at 8×8 and W = 300, ±57 at W = 1000, more for all-focus rows), never from a constant.

    rows with persistent == 0: three bands of unequal height that tile [0, H_w) — a top band (the clamp at row 0 inside the held rows), an
                               interior band, a bottom band (the clamp at row H_w − 1); H_w the smallest height at which the middle one is
                               interior
    rows with persistent  > 0: one interior band of more than 2 × CUs tiles, so that the persistent kernels walk their tile loops with
                               out_rows ≠ H and out_y0 ≠ 0

tests/test_dispatch_windows_table.py holds every plan to its conditions on the CPU; tests/test_gpu_dispatch_windows.py renders them.  A plain
module like poison.py.
"""
import test_gpu_dispatch_coverage as dc

# launch_blend refuses these under a window (lfi_dispatch.hpp generic_kernel): one pixel grid over the whole image, no window arithmetic
GENERIC = {"blend_ten_m16", "blend_ten_direct", "blend_std_mfma", "blend_std_valu", "blend_std_vfma"}
REFUSAL = "with a row window only renders with the default"

WINDOWED = [r for r in dc.MATRIX if r.expect not in GENERIC]
REFUSED = [r for r in dc.MATRIX if r.expect in GENERIC]

MIDDLE_ROWS = 11     # the interior band of a three-band plan
SPARE_TILE_ROWS = 8  # persistent rows: band rows beyond 2 × CUs / tiles_x, as test_dispatch_row's image has


def held_rows(L, row, hp, band, H, hp_first=None):
    """Input rows [in_y0, in_y1) a context must hold to render output rows `band` of the row at image height H.  order == "xcd": the
    context's first lfi_set_params carries the larger offsets of the focus sweep's first step (hp_first), which the window must cover too."""
    if row.all_focus:
        return L.input_rows_all_focus(band, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, H)
    y0, y1 = L.input_rows(band, hp.focused_offsets, H)
    if hp_first is not None:
        f0, f1 = L.input_rows(band, hp_first.focused_offsets, H)
        y0, y1 = min(y0, f0), max(y1, f1)
    return y0, y1


def band_rows(row, cu):
    """Rows of a persistent row's band: more than 2 × cu tiles of row.persistent pixels."""
    tiles_x = (row.W + row.persistent - 1) // row.persistent
    return 2 * cu // tiles_x + SPARE_TILE_ROWS


def _params(L, row, H):
    """The row's host parameters alone at height H (row_inputs without the images)."""
    hp = L.build_params(row.cols, row.rows, row.W, H, "0.071,0.071,0.93,0.93", *((0.1, 0.3) if row.all_focus else (0.23, 0.0)), 3.0, 1.783, row.V)
    return hp, dc.xcd_first_params(L, row, H) if row.order == "xcd" else None


def _layout(L, row, mid, hp, hp_first):
    """(top, bottom): the fewest rows above and below a middle band of `mid` rows that make it interior — 0 < in_y0 and in_y1 < H — with
    top, mid and bottom three different numbers.  The reach is measured in the middle of an image tall enough that no clamp shortens it."""
    tall = 8 * row.W + 4 * mid
    at = tall // 2
    y0, y1 = held_rows(L, row, hp, (at, at + mid), tall, hp_first)
    up, down = at - y0, y1 - (at + mid)
    assert 0 < up < at and 0 < down < tall - at - mid, (row.name, up, down, tall)
    top, bottom = up + 1, down + 1
    while top == mid:
        top += 1
    while bottom in (mid, top):
        bottom += 1
    return top, bottom


def window_plan(L, oc, row, cu):
    """(H_w, bands, hp, lf, m): the image height, the bands [(out_y0, out_y1, in_y0, in_y1)] and row_inputs(L, oc, row, H_w)."""
    assert row.expect not in GENERIC, row.name
    mid = band_rows(row, cu) if row.persistent else MIDDLE_ROWS
    # the offsets scale with the width, the focus estimate's block radius (all-focus rows hold its rows too) with the height: the height
    # whose own parameters give it back
    H_w = 4 * row.W
    for _ in range(8):
        top, bottom = _layout(L, row, mid, *_params(L, row, H_w))
        if H_w == top + mid + bottom:
            break
        H_w = top + mid + bottom
    else:
        raise AssertionError((row.name, "no height gives itself back", H_w, top, mid, bottom))
    hp, lf, m = dc.row_inputs(L, oc, row, H_w)
    hp_first = dc.xcd_first_params(L, row, H_w) if row.order == "xcd" else None
    outs = [(top, top + mid)] if row.persistent else [(0, top), (top, top + mid), (top + mid, H_w)]
    bands = [out + tuple(held_rows(L, row, hp, out, H_w, hp_first)) for out in outs]
    return H_w, bands, hp, lf, m


def uses_negative_and_positive_oy(row, hp):
    """Does some image sample above (oy < 0) and some below (oy > 0) its pixel in the offsets the render uses?  Fixed focus: the integer
    focused offsets; all-focus: offset.y × f for the focus values f of the range (of one sign throughout the rows' ranges)."""
    if row.all_focus:
        assert hp.focus > 0 and hp.focus + hp.range > 0
        oy = hp.offsets[:, 1] * hp.focus
        return bool((oy <= -1).any()), bool((oy >= 1).any())
    oy = hp.focused_offsets[:, 1]
    return bool((oy < 0).any()), bool((oy > 0).any())
