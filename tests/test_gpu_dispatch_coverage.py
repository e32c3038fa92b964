"""Dispatch coverage: every blend kernel the dispatch tree in csrc/hip/lfi_dispatch.hpp can launch, in every template form it is
instantiated for, compared against the oracle under poison (tests/poison.py).

One table.  Each row names a shape, a view range, a method, all-focus or not, the view layout, the flags, the variant and the kind of
weights, and the kernel that lfi_last_kernel_name() must report for it.  Every row renders twice, under both poison bytes (so both sweep
directions of the kernels that alternate them): STD bit-exact, TEN_WM within one LSB of the oracle's M16 model and inside the interval of
the exact sum (tests/ten_interval.py; rows with `dyadic` weights: no accumulation error is possible, so byte for byte the exact model), the
per-batch rounding debug mode (LFI_FLAG_TEN_ROUND_PER_BATCH) byte for byte M16; views outside the range must still hold the poison.

Two more columns follow from the kernel and the layout: whether the launch reads the derived planar copy of the inputs (READS_COPY), and
whether, in the planar view layout, it goes through the RGBA scratch copy and the conversion (every kernel outside WRITES_PLANES).  The
row's fresh context shows both after its first render, before any download: lfi_memory_info's derived_bytes > 0 exactly when the launch
read the copy, workspace_bytes > 0 exactly when it used the scratch copy (no focus map, no download has run).

Rows marked `persistent` have more tiles than 2 × the device's CUs, so that the persistent kernels walk their tile loops (a small image
gives every workgroup one tile).  A CPU test (no gpu mark) reads every note_kernel(c, "…") name under csrc/hip/ and fails if the table
has no row for one of them, or misses one of the chunk counts / output forms a kernel is instantiated for.
"""
import os
import re
from dataclasses import dataclass

import numpy as np
import pytest

import poison
import ten_interval
from conftest import ROOT

TEN_TOL_LSB = 1
HIP_DIR = os.path.join(ROOT, "lfinterpolator_amd", "csrc", "hip")
MEASUREMENT_ONLY = {"blend_p3<ABLATION>"}   # LFI_MEASUREMENT_BUILD only: not in the product library
ROUND = 2    # LFI_FLAG_TEN_ROUND_PER_BATCH
THREADS = min(os.cpu_count() or 1, 16)
READS_COPY = {"blend_p3<TEN_WM>", "blend_p3<TEN_WM,rgba>", "blend_planar<TEN_WM>", "blend_planar<STDF>", "blend_stdx<STD>"}
# planar view layout: the kernels that write the byte planes themselves (every shape here fits their 32-bit plane addressing)
WRITES_PLANES = {"blend_p3<TEN_WM>", "blend_stdx<STD>", "blend_stdxa<STD,allfocus>", "blend_persist<TEN_WM,allfocus>"}


@dataclass(frozen=True)
class Row:
    name: str
    cols: int
    rows: int
    W: int
    H: int               # rows of the image (persistent rows: at least; raised until n_tiles > 2 × CUs)
    V: int
    v0: int
    v1: int
    method: str          # "STD" / "TEN_WM"
    all_focus: bool
    layout: str          # "rgba" / "planar"
    flags: int
    variant: str         # of `method`; "auto" = the default
    weights: str         # "default" (build_params: in [0, 2), sums ≤ 2) / "wide" (one weight of 2.5: outside [0, 2)) /
                         # "dyadic" (the default ones floored to multiples of 2^-12: every fp32 partial sum is exact, see row_inputs)
    expect: str          # lfi_last_kernel_name()
    persistent: int = 0  # pixels per tile of the kernel when the row must run its tile loop, else 0
    order: str = ""      # blend_p3, planar layout: "plain" / "xcd" tile order (see test_dispatch_row)
    far: bool = False    # one image's focused x offset beyond the derived copy's reach (4·W + 4096): the route without the copy
    quant: int = 1       # the input bytes rounded down to multiples of it (dyadic rows: 16 makes fp16 ties and integer sums common)

    @property
    def n(self):
        return self.cols * self.rows

    @property
    def chunks(self):   # 64-image chunks of k_pad = n rounded up to 16
        return ((self.n + 15) // 16 * 16 + 63) // 64

    @property
    def reads_copy(self):
        return self.expect in READS_COPY

    @property
    def scratch(self):
        return self.layout == "planar" and self.expect not in WRITES_PLANES


def R(name, grid, W, H, V, method, expect, v=None, af=False, layout="rgba", flags=0, variant="auto", weights="default", persistent=0, order="",
      far=False, quant=1):
    v0, v1 = v if v else (0, V)
    return Row(name, grid[0], grid[1], W, H, V, v0, v1, method, af, layout, flags, variant, weights, expect, persistent, order, far, quant)


G1, G1S, G2, G3, G4 = (8, 8), (3, 3), (9, 9), (12, 12), (15, 15)   # k_pad 64, 16, 80..128 (2 chunks), 144 (3), 225 -> 240 (4)
MATRIX = [
    # ---- TEN_WM, RGBA views ----
    R("p3_rgba_2ch", G2, 300, 5, 9, "TEN_WM", "blend_p3<TEN_WM,rgba>"),
    R("p3_rgba_3ch", G3, 257, 4, 7, "TEN_WM", "blend_p3<TEN_WM,rgba>"),
    R("p3_rgba_4ch_range", G4, 200, 3, 70, "TEN_WM", "blend_p3<TEN_WM,rgba>", v=(3, 67)),
    R("p3_rgba_2ch_tiles", G2, 1000, 8, 8, "TEN_WM", "blend_p3<TEN_WM,rgba>", persistent=128),
    R("planar_ten_1ch", G1, 200, 6, 8, "TEN_WM", "blend_planar<TEN_WM>"),
    R("planar_ten_small_k", G1S, 130, 5, 70, "TEN_WM", "blend_planar<TEN_WM>", v=(1, 69)),
    R("planar_ten_tiles", G1, 1000, 8, 16, "TEN_WM", "blend_planar<TEN_WM>", persistent=128),
    R("persist_ten_af", G1, 200, 6, 8, "TEN_WM", "blend_persist<TEN_WM,allfocus>", af=True),
    R("persist_ten_af_4ch_range", G4, 150, 3, 40, "TEN_WM", "blend_persist<TEN_WM,allfocus>", af=True, v=(5, 37)),
    R("persist_ten_af_tiles", (4, 4), 1000, 8, 4, "TEN_WM", "blend_persist<TEN_WM,allfocus>", af=True, persistent=128),
    R("persist_ten", G2, 200, 4, 70, "TEN_WM", "blend_persist<TEN_WM>", variant="persist_m2_nt"),
    R("wave_ten", (4, 4), 300, 5, 8, "TEN_WM", "blend_wave<TEN_WM>", variant="wave_m2_nt"),
    R("ten_direct", G2, 130, 4, 9, "TEN_WM", "blend_ten_direct", variant="direct_p1m2"),
    R("ten_direct_wide_weights", G1, 130, 4, 9, "TEN_WM", "blend_ten_direct", weights="wide"),
    R("ten_direct_af", (4, 4), 100, 4, 5, "TEN_WM", "blend_ten_direct", af=True, variant="direct_p1m2"),
    R("ten_m16", G2, 100, 4, 5, "TEN_WM", "blend_ten_m16", flags=ROUND),
    R("ten_m16_af", (4, 4), 100, 4, 5, "TEN_WM", "blend_ten_m16", af=True, flags=ROUND),
    # ---- STD, RGBA views ----
    R("stdx_rgba_2ch", G2, 300, 5, 9, "STD", "blend_stdx<STD>"),
    R("stdx_rgba_3ch_range", G3, 257, 4, 70, "STD", "blend_stdx<STD>", v=(2, 69)),
    R("stdx_rgba_4ch", G4, 200, 3, 7, "STD", "blend_stdx<STD>"),
    R("stdx_rgba_2ch_tiles", G2, 1000, 8, 8, "STD", "blend_stdx<STD>", persistent=128),
    R("planar_stdf", G1, 200, 6, 8, "STD", "blend_planar<STDF>"),
    R("planar_stdf_range", G1S, 130, 5, 70, "STD", "blend_planar<STDF>", v=(3, 68)),
    R("planar_stdf_tiles", G1, 1000, 8, 16, "STD", "blend_planar<STDF>", persistent=128),
    R("stdxa_1ch", G1, 200, 5, 8, "STD", "blend_stdxa<STD,allfocus>", af=True),
    R("stdxa_2ch", G2, 130, 4, 9, "STD", "blend_stdxa<STD,allfocus>", af=True),
    R("stdxa_3ch_range", G3, 150, 3, 70, "STD", "blend_stdxa<STD,allfocus>", af=True, v=(1, 66)),
    R("stdxa_4ch", G4, 129, 3, 5, "STD", "blend_stdxa<STD,allfocus>", af=True),
    R("stdxa_2ch_tiles", G2, 1000, 8, 4, "STD", "blend_stdxa<STD,allfocus>", af=True, persistent=128),
    R("afs_3ch", G3, 150, 4, 9, "STD", "blend_afs<STD,allfocus>", af=True, variant="filtered_gather_once"),
    R("afs_4ch_range", G4, 129, 3, 70, "STD", "blend_afs<STD,allfocus>", af=True, variant="filtered_gather_once", v=(4, 69)),
    R("afs_3ch_tiles", G3, 1000, 8, 4, "STD", "blend_afs<STD,allfocus>", af=True, variant="filtered_gather_once", persistent=64),
    R("persist_std", G2, 200, 4, 70, "STD", "blend_persist<STD>", variant="persist_m2_nt"),
    R("persist_std_af", G1, 200, 4, 9, "STD", "blend_persist<STD,allfocus>", af=True, variant="persist_m2_nt"),
    R("persist_std_tiles", G1, 1000, 8, 8, "STD", "blend_persist<STD>", variant="persist_m2_nt", persistent=128),
    R("wave_std", (4, 4), 300, 5, 8, "STD", "blend_wave<STD>", variant="wave_m2_nt"),
    R("wave_std_wide_weights", G1, 150, 4, 9, "STD", "blend_wave<STD>", weights="wide"),
    R("std_mfma", G2, 130, 4, 9, "STD", "blend_std_mfma", variant="mfma_p1m2"),
    R("std_valu", (4, 4), 100, 4, 5, "STD", "blend_std_valu", variant="valu"),
    R("std_vfma", (4, 4), 100, 4, 5, "STD", "blend_std_vfma", variant="vfma"),
    R("std_vfma_af", (4, 4), 100, 4, 5, "STD", "blend_std_vfma", af=True, variant="vfma"),
    # ---- planar views written by the kernels themselves ----
    R("p3_1ch", G1, 300, 5, 9, "TEN_WM", "blend_p3<TEN_WM>", layout="planar"),
    R("p3_1ch_4passes", G1, 200, 4, 200, "TEN_WM", "blend_p3<TEN_WM>", layout="planar"),
    R("p3_1ch_300views_range", G1S, 130, 3, 300, "TEN_WM", "blend_p3<TEN_WM>", layout="planar", v=(5, 290)),
    R("p3_2ch", G2, 257, 4, 9, "TEN_WM", "blend_p3<TEN_WM>", layout="planar"),
    R("p3_3ch_range", G3, 200, 3, 70, "TEN_WM", "blend_p3<TEN_WM>", layout="planar", v=(2, 68)),
    R("p3_4ch", G4, 130, 3, 7, "TEN_WM", "blend_p3<TEN_WM>", layout="planar"),
    # launch_blend sets LFI_KFLAG_PLAIN_TILE_ORDER iff planar_phases_tuned(c): the copy's phases fit the current offsets (after lfi_prepare) ...
    R("p3_1ch_tiles_plain_order", G1, 1000, 8, 16, "TEN_WM", "blend_p3<TEN_WM>", layout="planar", persistent=128, order="plain"),
    # ... and not after a second lfi_set_params with another focus and no re-tune (a focus sweep): XCD-contiguous runs of tiles
    R("p3_2ch_tiles_xcd_order", G2, 1000, 8, 8, "TEN_WM", "blend_p3<TEN_WM>", layout="planar", persistent=128, order="xcd"),
    R("stdx_planar_1ch", G1, 300, 5, 9, "STD", "blend_stdx<STD>", layout="planar"),
    R("stdx_planar_2ch_range", G2, 200, 4, 70, "STD", "blend_stdx<STD>", layout="planar", v=(1, 66)),
    R("stdx_planar_3ch", G3, 130, 3, 7, "STD", "blend_stdx<STD>", layout="planar"),
    R("stdx_planar_4ch", G4, 129, 3, 5, "STD", "blend_stdx<STD>", layout="planar"),
    R("stdx_planar_1ch_tiles", G1, 1000, 8, 8, "STD", "blend_stdx<STD>", layout="planar", persistent=128),
    R("stdxa_planar_1ch", G1, 200, 5, 8, "STD", "blend_stdxa<STD,allfocus>", af=True, layout="planar"),
    R("stdxa_planar_2ch", G2, 130, 4, 9, "STD", "blend_stdxa<STD,allfocus>", af=True, layout="planar"),
    R("stdxa_planar_3ch", G3, 150, 3, 7, "STD", "blend_stdxa<STD,allfocus>", af=True, layout="planar"),
    R("stdxa_planar_4ch_range", G4, 129, 3, 70, "STD", "blend_stdxa<STD,allfocus>", af=True, layout="planar", v=(6, 68)),
    R("persist_ten_af_planar", G1, 200, 6, 8, "TEN_WM", "blend_persist<TEN_WM,allfocus>", af=True, layout="planar"),
    # the other variants, where the route reaches a kernel with a planar-view epilogue
    R("p3_planar_variant", G2, 200, 4, 9, "TEN_WM", "blend_p3<TEN_WM>", layout="planar", variant="planar_m2_nt"),
    R("stdx_planar_gather_once_2ch", G2, 200, 4, 9, "STD", "blend_stdx<STD>", layout="planar", variant="filtered_gather_once"),
    R("persist_ten_af_planar_persist", G1, 200, 6, 8, "TEN_WM", "blend_persist<TEN_WM,allfocus>", af=True, layout="planar", variant="persist_m2_nt"),
    R("persist_ten_af_planar_wave", (4, 4), 150, 5, 8, "TEN_WM", "blend_persist<TEN_WM,allfocus>", af=True, layout="planar", variant="wave_m2_nt"),
    R("stdxa_planar_gather_once_1ch", G1, 200, 5, 8, "STD", "blend_stdxa<STD,allfocus>", af=True, layout="planar", variant="filtered_gather_once"),
    R("stdxa_planar_gather_once_2ch", G2, 130, 4, 9, "STD", "blend_stdxa<STD,allfocus>", af=True, layout="planar", variant="filtered_gather_once"),
    # ---- planar views through the RGBA scratch copy and the conversion (debug modes, other variants, weights outside [0, 2)) ----
    R("scratch_ten_m16", G2, 130, 4, 9, "TEN_WM", "blend_ten_m16", layout="planar", flags=ROUND),
    R("scratch_ten_wide_range", G1, 150, 4, 9, "TEN_WM", "blend_ten_direct", layout="planar", weights="wide", v=(2, 7)),
    R("scratch_std_valu", (4, 4), 100, 4, 5, "STD", "blend_std_valu", layout="planar", variant="valu"),
    R("scratch_persist_std_range", G2, 200, 4, 70, "STD", "blend_persist<STD>", layout="planar", variant="persist_m2_nt", v=(3, 67)),
    R("scratch_afs", G4, 129, 3, 9, "STD", "blend_afs<STD,allfocus>", af=True, layout="planar", variant="filtered_gather_once"),
    R("scratch_wave_ten", (4, 4), 300, 5, 8, "TEN_WM", "blend_wave<TEN_WM>", layout="planar", variant="wave_m2_nt"),
    R("scratch_wave_std", (4, 4), 300, 5, 8, "STD", "blend_wave<STD>", layout="planar", variant="wave_m2_nt"),
    # ---- the default TEN_WM route when the derived copy cannot serve the offsets ----
    R("persist_ten_copy_out_of_reach", G1, 130, 4, 9, "TEN_WM", "blend_persist<TEN_WM>", far=True),
    R("scratch_persist_ten_copy_out_of_reach", G2, 130, 4, 9, "TEN_WM", "blend_persist<TEN_WM>", layout="planar", far=True),
    # ---- TEN_WM with no accumulation error at all: byte for byte the exact sum's, fp16 ties and integer sums included ----
    R("p3_1ch_dyadic", G1, 300, 5, 9, "TEN_WM", "blend_p3<TEN_WM>", layout="planar", weights="dyadic"),
    R("p3_4ch_dyadic_q16", G4, 130, 3, 7, "TEN_WM", "blend_p3<TEN_WM>", layout="planar", weights="dyadic", quant=16),
    R("p3_rgba_2ch_dyadic_q16", G2, 300, 5, 9, "TEN_WM", "blend_p3<TEN_WM,rgba>", weights="dyadic", quant=16),
    R("planar_ten_dyadic", G1, 200, 6, 8, "TEN_WM", "blend_planar<TEN_WM>", weights="dyadic"),
    R("persist_ten_af_dyadic_q16", G1, 200, 6, 8, "TEN_WM", "blend_persist<TEN_WM,allfocus>", af=True, weights="dyadic", quant=16),
    R("persist_ten_dyadic", G2, 200, 4, 16, "TEN_WM", "blend_persist<TEN_WM>", variant="persist_m2_nt", weights="dyadic"),
    R("wave_ten_dyadic_q16", (4, 4), 300, 5, 8, "TEN_WM", "blend_wave<TEN_WM>", variant="wave_m2_nt", weights="dyadic", quant=16),
    R("ten_direct_dyadic", G2, 200, 6, 9, "TEN_WM", "blend_ten_direct", variant="direct_p1m2", weights="dyadic"),
]


def _note_kernel_names():
    """Every kernel name a note_kernel(c, …) call under csrc/hip/ can report: the string literals of its argument (both arms of ternaries)."""
    names = set()
    for f in sorted(os.listdir(HIP_DIR)):
        if not f.endswith((".hpp", ".hip")):
            continue
        text = open(os.path.join(HIP_DIR, f)).read()
        for call in re.finditer(r"note_kernel\(\s*c\s*,(.*?)\);", text, flags=re.S):
            names.update(re.findall(r'"([^"]+)"', call.group(1)))
    return names


def test_every_noted_kernel_has_a_coverage_row():
    names = _note_kernel_names()
    assert len(names) >= 19 and MEASUREMENT_ONLY <= names, sorted(names)
    covered = {r.expect for r in MATRIX}
    missing = sorted(names - MEASUREMENT_ONLY - covered)
    assert not missing, f"kernels without a row in tests/test_gpu_dispatch_coverage.py MATRIX: {missing}"
    assert not covered - names, sorted(covered - names)
    assert len({r.name for r in MATRIX}) == len(MATRIX)


def test_matrix_reaches_every_chunk_count_and_output_form():
    def forms(kernel, layout=None):
        return {r.chunks for r in MATRIX if r.expect == kernel and (layout is None or r.layout == layout)}
    assert forms("blend_p3<TEN_WM>") == {1, 2, 3, 4}
    assert forms("blend_p3<TEN_WM,rgba>") == {2, 3, 4}             # one chunk: blend_planar serves RGBA views
    assert forms("blend_stdx<STD>", "planar") == {1, 2, 3, 4}
    assert forms("blend_stdx<STD>", "rgba") == {2, 3, 4}            # one chunk, RGBA views: blend_planar<STDF>
    assert forms("blend_stdxa<STD,allfocus>", "planar") == {1, 2, 3, 4}
    assert forms("blend_stdxa<STD,allfocus>", "rgba") == {1, 2, 3, 4}
    assert forms("blend_afs<STD,allfocus>") == {3, 4}
    p3_one = [r for r in MATRIX if r.expect == "blend_p3<TEN_WM>" and r.chunks == 1]
    assert any(r.v1 - r.v0 <= 64 for r in p3_one) and any(64 < r.v1 - r.v0 <= 256 for r in p3_one) and any(r.v1 - r.v0 > 256 for r in p3_one)
    for kernel in ("blend_p3<TEN_WM>", "blend_p3<TEN_WM,rgba>", "blend_stdx<STD>", "blend_stdxa<STD,allfocus>", "blend_afs<STD,allfocus>",
                   "blend_persist<TEN_WM,allfocus>", "blend_persist<STD>", "blend_planar<TEN_WM>", "blend_planar<STDF>"):
        assert any(r.persistent for r in MATRIX if r.expect == kernel), kernel
    assert {r.order for r in MATRIX if r.expect == "blend_p3<TEN_WM>" and r.persistent} == {"plain", "xcd"}
    assert {r.layout for r in MATRIX if r.far} == {"rgba", "planar"}
    # the output forms: every kernel that writes planar views does so in some row, and some row reaches each kernel that reads the copy
    assert WRITES_PLANES <= {r.expect for r in MATRIX if r.layout == "planar" and not r.scratch}
    assert READS_COPY <= {r.expect for r in MATRIX}


def _cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _height(row, cu):
    if not row.persistent:
        return row.H
    tiles_x = (row.W + row.persistent - 1) // row.persistent
    return max(row.H, 2 * cu // tiles_x + 8)


def _map(W, H, seed):
    rng = np.random.default_rng(seed)
    lv = np.repeat(np.repeat(rng.integers(0, 256, size=((H + 3) // 4, (W + 36) // 37)), 4, axis=0), 37, axis=1)[:H, :W]
    noise = rng.integers(0, 256, size=(H, W))
    lv = np.where(rng.random((H, W)) < 0.3, noise, lv)
    m = np.repeat(lv[..., None].astype(np.uint8), 4, axis=-1)
    m[..., 3] = 255
    return m


DYADIC_TIES = 50     # fp16 ties a dyadic row must hold before its launch, so that it does test the RN-even conversion


def row_inputs(L, oc, row, H):
    """A row's host parameters, input images and focus map (all-focus rows; else None) at image height H: what test_dispatch_row renders
    and what tests/test_ten_interval.py holds the interval's own width to on the CPU."""
    W, n = row.W, row.n
    focus, frange = (0.1, 0.3) if row.all_focus else (0.23, 0.0)
    hp = L.build_params(row.cols, row.rows, W, H, "0.071,0.071,0.93,0.93", focus, frange, 3.0, 1.783, row.V)
    if row.weights == "wide":
        hp.weights = hp.weights.copy()
        hp.weights[:, n // 2] = 0x4100     # fp16 2.5
    if row.weights == "dyadic":
        # multiples of 2^-12 that sum to at most 2: every product with a byte and every partial sum is a multiple of 2^-12 below 512,
        # 21 bits, exact in fp32 in any order of accumulation
        w = np.floor(ten_interval.weights_f64(hp.weights) * 4096.0) / 4096.0
        assert (w.astype(np.float16) == w).all()
        hp.weights = w.astype(np.float16).view(np.uint16)
    if row.far:
        hp.focused_offsets = hp.focused_offsets.copy()
        hp.focused_offsets[n // 2, 0] = 4 * W + 5000
    lf = oc.synthetic_lf(n, W, H, 0x5EED + n + W)
    if row.quant > 1:
        lf = (lf // row.quant * row.quant).astype(np.uint8)
        lf[..., 3] = 255
    return hp, lf, _map(W, H, n + W) if row.all_focus else None


def ten_row_interval(oc, row, hp, lf, m, threads=THREADS):
    """S, ε, lo, hi of a TEN_WM row (all views; zero outside the row's range).  A dyadic row: ε = 0 after its preconditions are checked."""
    S, eps = ten_interval.exact_sums(oc, lf, hp, v0=row.v0, v1=row.v1, threads=threads, all_focus=row.all_focus, map_plane=m, focus=hp.focus,
                                     rng=hp.range)
    if row.weights == "dyadic":
        w = ten_interval.weights_f64(hp.weights)
        assert (w * 4096.0 == np.floor(w * 4096.0)).all() and (w >= 0).all() and w.sum(axis=1).max() <= 2.0, row.name
        assert (S * 4096.0 == np.floor(S * 4096.0)).all() and S.max() < 512.0
        n_ties = ten_interval.ties(S[row.v0:row.v1])
        assert n_ties >= DYADIC_TIES, (row.name, n_ties)
        eps = np.zeros_like(eps)
    lo, hi = ten_interval.interval(S, eps)
    return S, eps, lo, hi


XCD_FIRST_FOCUS = 0.6   # order == "xcd": the focus the planar copy is built and tuned for before the row's own parameters are set


def xcd_first_params(L, row, H):
    """order == "xcd": the parameters of the focus sweep's first step (a larger focus than the row's own)."""
    return L.build_params(row.cols, row.rows, row.W, H, "0.071,0.071,0.93,0.93", XCD_FIRST_FOCUS, 0.0, 3.0, 1.783, row.V)


def row_context(L, row, hp, lf, m, H, window=None):
    """A fresh context set up for the row at image height H, ready to render; window = (out_y0, out_y1, in_y0, in_y1): a row window
    (lfi_set_row_window) set before the upload, so that only the held rows of the whole-image arrays are copied."""
    ctx = L.Context(0)
    ctx.set_grid(row.cols, row.rows, row.W, H)
    if window is not None:
        ctx.set_row_window(*window)
    ctx.upload_grid(lf)
    ctx.set_output_layout(row.layout)
    if row.order == "xcd":
        # the planar copy built and tuned for a larger focus; then a focus sweep's next step: smaller offsets (the copy still covers
        # them), no re-tune — unless every image's integer offset moved by a multiple of 128 pixels, the phases no longer fit
        hp_first = xcd_first_params(L, row, H)
        ctx.set_params(hp_first, row.flags)
        ctx.prepare(row.method)
        assert ((hp.focused_offsets[:, 0] - hp_first.focused_offsets[:, 0]) % 128 != 0).any()
    ctx.set_params(hp, row.flags)
    if row.order == "plain":
        ctx.prepare(row.method)
    if row.variant != "auto":
        ctx.set_variant(row.method, row.variant)
    if row.all_focus:
        ctx.upload_map(0, m)
        ctx.upload_map(1, m)
    return ctx


def row_expected(oc, row, hp, lf, m):
    """The oracle's views [v0, v1) of the row, the LSB tolerance against them, and for TEN_WM outside the per-batch debug mode (M16 byte
    for byte, by design not the exact sum's bytes) the interval of the exact sum: S, eps, lo, hi (else four times None)."""
    kw = dict(v0=row.v0, v1=row.v1, threads=THREADS, all_focus=row.all_focus, map_plane=m, focus=hp.focus, rng=hp.range)
    if row.method == "STD":
        want, tol = oc.blend_std(lf, hp.focused_offsets, hp.offsets, hp.weights, **kw), 0
    else:
        want = oc.blend_ten(lf, hp.focused_offsets, hp.offsets, hp.weights, model=oc.TEN_M16, **kw)
        tol = 0 if row.flags & ROUND else TEN_TOL_LSB
    S = eps = lo = hi = None
    if row.method == "TEN_WM" and not row.flags & ROUND:
        S, eps, lo, hi = (a[row.v0:row.v1] for a in ten_row_interval(oc, row, hp, lf, m))
    return want[row.v0:row.v1], tol, S, eps, lo, hi


def check_paths(ctx, row):
    """The row's fresh context after its first render, before any download (which may allocate a staging plane)."""
    mi = ctx.memory_info()
    got = {"reads_copy": mi.derived_bytes > 0, "scratch": mi.workspace_bytes > 0}
    assert got == {"reads_copy": row.reads_copy, "scratch": row.scratch}, (row.name, got)


def check_rendered(row, tag, byte, got, want, tol, S, eps, lo, hi):
    """Views [v0, v1) as downloaded (or a band of their rows) against row_expected's (the same rows): the table's contract."""
    bad = poison.mismatch(got, want, tol)
    assert bad == 0, (row.name, tag, hex(byte), bad)
    if lo is not None:
        out = ten_interval.outside(got, lo, hi)
        differ = int((got[..., :3] != ten_interval.quantise(S)).sum())
        print(f"TEN_INTERVAL {row.name}{tag} {row.expect} {hex(byte)} bytes={lo.size} differ_from_exact={differ} outside={out}")
        assert out == 0, (row.name, tag, hex(byte), out, "needed multiples of eps, largest:", float(ten_interval.report(got, S, eps).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("row", MATRIX, ids=lambda r: r.name)
def test_dispatch_row(row, gpu, oracle_c):
    cu = _cu_count()
    H = _height(row, cu)
    W = row.W
    if row.persistent:
        tiles = (W + row.persistent - 1) // row.persistent * H
        assert tiles > 2 * cu, (tiles, cu)
    hp, lf, m = row_inputs(gpu, oracle_c, row, H)
    ctx = row_context(gpu, row, hp, lf, m, H)
    want, tol, S, eps, lo, hi = row_expected(oracle_c, row, hp, lf, m)
    outside = None if row.V <= 80 else [0, row.v0 - 1, row.v1, row.V - 1]

    def check(byte):
        got = poison.render_range(ctx, row.method, row.v0, row.v1, all_focus=row.all_focus, byte=byte, outside=outside,
                                  inspect=(lambda: check_paths(ctx, row)) if byte == poison.POISON[0] else None)
        assert ctx.last_kernel_name() == row.expect, (row.name, ctx.last_kernel_name())
        check_rendered(row, "", byte, got, want, tol, S, eps, lo, hi)
    poison.twice(check)
    ctx.close()


@pytest.mark.gpu
def test_poison_helper_reports_unrendered_views(gpu, oracle_c):
    """The helper's own check: correct bytes rendered once, then poisoned and NOT rendered again — every comparison must report it."""
    cols, rows, W, H, V = 4, 4, 130, 5, 6
    hp = gpu.build_params(cols, rows, W, H, "0,0,1,1", 0.23, 0.0, 3.0, 1.783, V)
    lf = oracle_c.synthetic_lf(cols * rows, W, H, 99)
    want = oracle_c.blend_std(lf, hp.focused_offsets, hp.offsets, hp.weights)
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, W, H)
    ctx.upload_grid(lf)
    ctx.set_params(hp)
    for layout in ("rgba", "planar"):
        ctx.set_output_layout(layout)
        for b in poison.POISON:
            poison.render(ctx, "STD", byte=b)
            assert poison.mismatch(ctx.download_views(), want) == 0
            assert poison.written_outside(ctx, 0, V, b) == []
            ctx.poison(poison.RENDER, b)      # … and no launch
            ctx.sync()
            got = ctx.download_views()
            assert poison.mismatch(got, want) > 0 and (got == poison.untouched_view(ctx, b)).all(), layout
            assert poison.written_outside(ctx, 2, 3, b) == []
            # a view range rendered WITHOUT poisoning first leaves the full render's bytes outside it: the range check must see them
            ctx.render("STD")
            ctx.render("STD", v0=2, v1=3)
            ctx.sync()
            assert poison.written_outside(ctx, 2, 3, b) == [v for v in range(V) if v != 2]
    ctx.close()


@pytest.mark.gpu
def test_poison_never_changes_a_later_result(gpu, oracle_c):
    """Poison-then-call gives the bytes of the call alone, for every poison bit: renders that read the planar input copy (rebuilt after
    LFI_POISON_DERIVED), renders through the planar layout's RGBA scratch copy, focus maps (the padded planes of the estimate rebuilt after
    LFI_POISON_FOCUS_WORKSPACE) — also a focus map of smaller shifts and radius after a larger one in the same context, whose workspace is then
    larger than it needs.  LFI_POISON_DERIVED is refused once the planar copy is the only copy of the inputs."""
    import lfinterpolator_amd as L
    cols, rows, W, H, V = 9, 9, 300, 40, 9
    lf = oracle_c.synthetic_lf(cols * rows, W, H, 4242)
    lf = (lf // 16 * 16).astype(np.uint8)
    lf[..., 3] = 255
    big = gpu.build_params(cols, rows, W, H, "0.071,0.071,0.93,0.93", 0.4, 0.5, 7.0, 1.783, V)
    big.block_radius = np.array((9, 5), np.int32)
    small = gpu.build_params(cols, rows, W, H, "0.071,0.071,0.93,0.93", 0.1, 0.15, 7.0, 1.783, V)
    small.block_radius = np.array((3, 2), np.int32)
    want_map0 = oracle_c.focus_estimate(lf, small.offsets, small.focus_map_ids, small.focus, small.range, small.block_radius, threads=THREADS)
    assert len(np.unique(want_map0[..., 0])) > 2

    def sequence(ctx, bits):
        out = {}
        ctx.set_output_layout("rgba")
        ctx.set_params(big)
        ctx.focus_map()                       # the larger geometry first: the workspace is sized for it
        ctx.set_params(small)
        for what, fn in (("map", lambda: ctx.focus_map()),
                         ("ten", lambda: ctx.render("TEN_WM")),
                         ("std", lambda: ctx.render("STD")),
                         ("af_std", lambda: ctx.render("STD", all_focus=True))):
            # (the maps are the focus map's output, not a cache: poisoned before it only, not before the renders that read them)
            ctx.poison(bits if what == "map" else bits & ~L.LFI_POISON_MAPS, poison.POISON[0])
            fn()
            ctx.sync()
            out[what] = (ctx.download_map(0), ctx.download_map(1)) if what == "map" else ctx.download_views()
        ctx.set_output_layout("planar")
        for what, variant in (("p_ten", "auto"), ("p_std", "auto"), ("p_valu", "valu")):
            method = "TEN_WM" if what == "p_ten" else "STD"
            ctx.set_variant(method, variant)
            ctx.poison(bits, poison.POISON[1])
            ctx.render(method)
            ctx.sync()
            out[what] = ctx.download_views()
            ctx.set_variant(method, "auto")
        return out

    ref_ctx = gpu.Context(0)
    ref_ctx.set_grid(cols, rows, W, H)
    ref_ctx.upload_grid(lf)
    ref = sequence(ref_ctx, 0)
    ref_ctx.close()
    assert (ref["map"][0] == want_map0).all()
    assert (ref["std"] == oracle_c.blend_std(lf, small.focused_offsets, small.offsets, small.weights, threads=THREADS)).all()
    for bit in (L.LFI_POISON_VIEWS, L.LFI_POISON_SCRATCH, L.LFI_POISON_MAPS, L.LFI_POISON_FOCUS_WORKSPACE, L.LFI_POISON_DERIVED, poison.ALL):
        ctx = gpu.Context(0)
        ctx.set_grid(cols, rows, W, H)
        ctx.upload_grid(lf)
        got = sequence(ctx, bit)
        for what, want in ref.items():
            if what == "map":
                assert (got[what][0] == want[0]).all() and (got[what][1] == want[1]).all(), (bit, what)
            else:
                assert (got[what] == want).all(), (bit, what, poison.mismatch(got[what], want))
        ctx.release_inputs()
        with pytest.raises(L.LfiError):
            ctx.poison(L.LFI_POISON_DERIVED, 0)
        ctx.poison(poison.RENDER | poison.FOCUS, 0)   # everything else still may be poisoned
        ctx.render("TEN_WM")
        ctx.sync()
        assert (ctx.download_views() == ref["p_ten"]).all(), bit
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flat", [False, True], ids=["quantised", "flat_images"])
def test_focus_map_every_variant_under_poison(flat, gpu, oracle_c):
    """Every focus-map variant under poison of the maps and the workspace, twice (both poison bytes: flat images give a constant map,
    which one poison byte could equal)."""
    cols, rows, W, H = 6, 5, 300, 70
    hp = gpu.build_params(cols, rows, W, H, "0.071,0.071,0.93,0.93", 0.22, 0.3, 7.0, 1.783, 2)
    lf = oracle_c.synthetic_lf(cols * rows, W, H, 1717)
    lf = np.full_like(lf, 90) if flat else (lf // 16 * 16).astype(np.uint8)
    lf[..., 3] = 255
    want0 = oracle_c.focus_estimate(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, threads=THREADS)
    want1 = oracle_c.focus_filter(want0, hp.block_radius)
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, W, H)
    ctx.upload_grid(lf)
    ctx.set_params(hp)
    for variant in ctx.list_variants("FOCUS"):
        ctx.set_variant("FOCUS", variant)

        def check(byte):
            poison.focus_map(ctx, byte)
            assert (ctx.download_map(0) == want0).all() and (ctx.download_map(1) == want1).all(), (variant, hex(byte))
        poison.twice(check)
    ctx.close()
