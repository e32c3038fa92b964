"""The per-view-rows family (launch_view_rows in csrc/hip/lfi_dispatch.hpp: blend_vfocus.hpp, blend_vfocus_af.hpp) under test: its
coverage table VIEW_MATRIX — the counterpart of test_gpu_dispatch_coverage.MATRIX for the launches that lfi_set_view_offsets,
lfi_set_view_float_offsets and lfi_view_focus_maps route —, the oracle's expected values per view, the per-view check of the older tests
(test_gpu_view_focus.py, test_gpu_view_centres.py, test_gpu_view_maps.py) and the CLI runner.

A row names a shape, a view range, the kind of per-view rows, the source of an integer row's samples, the view layout, the flags, the
weights, how its offsets are made, an optional row window and an optional step before the rows are set, and the kernel name
lfi_last_kernel_name() must report per method.  tests/test_gpu_view_rows_coverage.py renders every row for both methods under both poison
bytes; tests/test_view_rows_table.py (CPU) holds the table to the kernels' names and tile constants and the interval to being a check.

What a view is held to: view v of an integer row samples image g at pixel + D[v][g], view v of a float row at (int)fma(f, O[v][g], pixel) with
f from the map the view reads, so the oracle's one-view render of weight row v with D[v] / O[v] (and that map) is the exact answer — STD byte for
byte, TEN_WM within one LSB of M16 and inside the interval of the exact sum (tests/ten_interval.py).  These kernels accumulate
fmaf(byte, w, acc) over ascending images: the products are exact and each addend costs one rounding of at most half an ulp of a partial sum,
which is below ten_interval.epsilon (one ulp per addend, k_pad addends).
"""
import functools
import subprocess
from dataclasses import dataclass

import numpy as np

import ten_interval

TEN_TOL_LSB = 1
TRAJ = "0.071,0.071,0.93,0.93"
ASPECT, EFFECT = 1.783, 3.0
UNIFIED = 1           # LFI_FLAG_UNIFIED_FOCUS_MAP
DYADIC_TIES = 50      # fp16 ties a dyadic row must hold, so that it does test the RN-even conversion
METHODS = ("STD", "TEN_WM")
KINDS = ("int", "float", "view_maps")
KERNEL = {("int", "rgba"): "blend_vfocus<{},rgba_src>", ("int", "planar"): "blend_vfocus<{}>",
          ("float", ""): "blend_vfocus_af<{}>", ("view_maps", ""): "blend_vfocus_af<{},view_maps>"}


def check_views(got, want, method):
    """got: the rendered views; want: per view the oracle's STD view, or for TEN_WM its (M16, exact, S, ε) tuple: the two byte models, the
    exact sums [H][W][3] float64 and the accumulation bound (ten_interval.epsilon of the view's weight row).  STD byte for byte, TEN_WM
    within the TEN_WM contract: ≤ TEN_TOL_LSB from M16, < 1e-3 of the bytes off the exactly-summed model, and every byte inside the
    interval of the exact sum."""
    if method == "STD":
        for v, w in enumerate(want):
            assert (got[v] == w).all(), ("STD view", v, int((got[v] != w).sum()))
    else:
        m16 = np.stack([w[0] for w in want])
        exact = np.stack([w[1] for w in want])
        S = np.stack([w[2] for w in want])
        eps = np.array([w[3] for w in want], np.float64)
        assert np.abs(got.astype(int) - m16.astype(int)).max() <= TEN_TOL_LSB
        assert (got != exact).mean() < 1e-3
        assert (got[..., 3] == 255).all()
        lo, hi = ten_interval.interval(S, eps)
        out = ten_interval.outside(got, lo, hi)
        assert out == 0, (out, "needed multiples of eps, largest:", float(ten_interval.report(got, S, eps).max()))


def ten_want(oc, lf, focused, offs, w_row, **kw):
    """One view's TEN_WM entry of check_views' `want`: (M16, exact, S, ε) of the oracle's render with the one weight row w_row [1][N]."""
    return (oc.blend_ten(lf, focused, offs, w_row, model=oc.TEN_M16, **kw)[0], oc.blend_ten(lf, focused, offs, w_row, model=oc.TEN_EXACT, **kw)[0],
            oc.blend_f64(lf, focused, offs, w_row, **kw)[0], float(ten_interval.epsilon(w_row, lf.shape[0])[0]))


def random_maps(H, W, seed):
    """Two different maps in which every focus byte 0…255 occurs (where the image has 256 pixels or more)."""
    rng = np.random.default_rng(seed)
    maps = []
    for _ in range(2):
        m = np.zeros((H, W, 4), np.uint8)
        m[..., 0] = rng.permutation(np.arange(H * W) % 256).reshape(H, W)
        m[..., 1:3] = m[..., :1]
        m[..., 3] = 255
        maps.append(m)
    return maps


def run_cli(native, *args):
    return subprocess.run([native.build.CLI, *args], capture_output=True, text=True, timeout=300)


# ---- the table ----------------------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Row:
    name: str
    cols: int
    rows: int
    W: int
    H: int
    V: int
    v0: int
    v1: int
    kind: str            # "int" (lfi_set_view_offsets) / "float" (lfi_set_view_float_offsets) / "view_maps" (… + lfi_view_focus_maps)
    source: str          # int rows: "planar" (the derived copy) / "rgba" (grid_device_ptr() without grid_modified(): the RGBA planes); else ""
    layout: str          # "rgba" / "planar" views
    flags: int
    weights: str         # "default" / "wide" (one weight of fp16 2.5) / "dyadic" (floored to multiples of 2^-12: no accumulation error)
    quant: int           # the input bytes rounded down to multiples of it
    ramp: tuple          # int rows: D = build_view_offsets over focus_ramp(*ramp); float rows: (focus, range), O = build_view_centred_offsets
    edit: str            # "" / "reach_W": shifts of exactly ±W and one far beyond the image written into D
    window: tuple        # () or the output rows (y0, y1); the input rows come from input_rows / input_rows_all_focus
    before: str          # "" / "plain": a plain TEN_WM render at focus ramp[0] first (the planar copy then has to grow) /
                         # "release": lfi_prepare + lfi_release_inputs at the parameters' focus (the planar copy is the only copy)

    @property
    def n(self):
        return self.cols * self.rows

    @property
    def chunks(self):   # 64-image chunks of k_pad = n rounded up to 16
        return ((self.n + 15) // 16 * 16 + 63) // 64

    @property
    def out_rows(self):
        return self.window[1] - self.window[0] if self.window else self.H

    def expect(self, method):
        """What lfi_last_kernel_name() must report."""
        return KERNEL[self.kind, self.source].format(method)


def R(name, grid, W, H, V, kind="int", v=None, source=None, layout="rgba", flags=0, weights="default", quant=1, ramp=None, edit="", window=(),
      before=""):
    v0, v1 = v if v else (0, V)
    source = ("planar" if source is None else source) if kind == "int" else ""
    ramp = ramp if ramp else ((0.0, 0.6) if kind == "int" else (0.1, 0.3))
    return Row(name, grid[0], grid[1], W, H, V, v0, v1, kind, source, layout, flags, weights, quant, ramp, edit, tuple(window), before)


def _both(name, *a, **kw):
    """A float shape: run with the context's map pair (`float`) and with a map pair per view (`view_maps`)."""
    return [R(name, *a, kind="float", **kw), R(name + "_view_maps", *a, kind="view_maps", **kw)]


G1, G1S, G2, G3, G4 = (8, 8), (3, 3), (9, 9), (12, 12), (15, 15)   # k_pad 64, 16, 96 (2 chunks), 144 (3), 240 (4)
VIEW_MATRIX = [
    # ---- integer rows, the planar copy as the source ----
    R("vf_255", G1, 255, 6, 17),
    R("vf_256_planar", G1S, 256, 7, 8, layout="planar"),
    R("vf_257_4ch_range", G4, 257, 5, 9, v=(1, 9)),
    R("vf_513_3tiles_planar", G3, 513, 5, 9, layout="planar"),
    # the last chunk of views runs past v1 into the padding views
    R("vf_259_v64_range", G2, 259, 5, 64, v=(5, 64)),
    R("vf_259_v64_range_planar", G2, 259, 5, 64, v=(5, 64), layout="planar"),
    # shifts of exactly ±W (the largest a planar copy is padded for: the 8-byte window and its pull-back to pitch − 8) and one far beyond
    R("vf_reach_W", (4, 4), 130, 6, 9, edit="reach_W"),
    R("vf_reach_W_planar", (4, 4), 130, 6, 9, edit="reach_W", layout="planar"),
    # the copy built for focus 0.02, then per-view offsets that reach much further
    R("vf_copy_grows", G1, 200, 6, 9, ramp=(0.02, 0.9), before="plain"),
    R("vf_released_planar", (4, 4), 64, 9, 8, ramp=(0.0, 0.5), before="release", layout="planar"),
    R("vf_window_planar", (4, 4), 72, 50, 7, ramp=(0.0, 0.5), window=(23, 50), layout="planar"),
    # ---- integer rows, the RGBA planes as the source ----
    R("vf_rgba_src", (4, 3), 45, 19, 9, source="rgba", ramp=(0.0, 0.8)),
    R("vf_rgba_src_259_planar", G2, 259, 5, 9, source="rgba", layout="planar"),
    R("vf_rgba_src_257_4ch", G4, 257, 5, 9, source="rgba"),
    # ---- integer rows, weights ----
    R("vf_wide", G1, 130, 4, 9, weights="wide"),
    R("vf_dyadic_q16", G1, 259, 5, 9, weights="dyadic", quant=16),
    R("vf_dyadic_q16_4ch", G4, 130, 3, 9, weights="dyadic", quant=16, layout="planar"),
    R("vf_rgba_src_dyadic_q16", G1, 259, 5, 9, source="rgba", weights="dyadic", quant=16),
    # ---- float rows: each shape with the context's maps and with per-view maps ----
    *_both("af_255", G1, 255, 6, 17),
    *_both("af_256", G1S, 256, 7, 8),
    *_both("af_257_4ch_range", G4, 257, 5, 9, v=(1, 9)),
    *_both("af_513_planar", G3, 513, 5, 9, layout="planar"),
    *_both("af_259_v64_range_planar", G2, 259, 5, 64, v=(5, 64), layout="planar"),
    *_both("af_unified", (4, 4), 130, 6, 9, flags=UNIFIED),
    *_both("af_dyadic_q16", G1, 259, 5, 9, weights="dyadic", quant=16),
    # lfi_view_focus_maps refuses a row window, so no per-view maps exist behind one: the context's maps only
    R("af_window_planar", (4, 4), 72, 50, 7, kind="float", ramp=(0.1, 0.4), window=(23, 50), layout="planar"),
]


@dataclass
class RowInputs:
    hp: object            # HostParams of the parameters the rows are set on
    lf: np.ndarray        # [N][H][W][4]
    offsets: np.ndarray   # D [V][N][2] int32 as handed to lfi_set_view_offsets / O [V][N][2] float32
    oracle_offsets: np.ndarray   # what the oracle gets: D clamped to ±W, ±H (a shift beyond the image samples its edge like ±W / ±H) / O
    maps: object          # float: the context's pair; view_maps: {v: pair}; int: None
    ids: object           # view_maps: build_view_focus_ids
    in_rows: tuple        # windowed rows: the input rows to hold
    hp_before: object     # before == "plain": the parameters of the first, plain render


def row_inputs(L, oc, row):
    """Everything a row renders from, and what the oracle gets.  Cached per row name: both methods share it and nothing changes it."""
    return _row_inputs(L, oc, row)


@functools.lru_cache(maxsize=None)
def _row_inputs(L, oc, row):
    cols, rows, W, H, V, n = row.cols, row.rows, row.W, row.H, row.V, row.n
    a, b = row.ramp
    if row.kind == "int":
        focus = L.focus_ramp(a, b, V)
        f0 = b if row.before == "release" else a      # released inputs: the copy is padded for the parameters' focus, the ramp's largest
        hp = L.build_params(cols, rows, W, H, TRAJ, float(f0), 0.0, EFFECT, ASPECT, V)
        off = L.build_view_offsets(cols, rows, W, H, TRAJ, ASPECT, focus)
        if row.edit == "reach_W":
            off[:, 0, 0] = W
            off[:, 1, 0] = -W
            off[2, 2] = (2 ** 31 - 1, -2 ** 31)
        want_off = off.copy()
        want_off[..., 0] = np.clip(want_off[..., 0], -W, W)
        want_off[..., 1] = np.clip(want_off[..., 1], -H, H)
    else:
        hp = L.build_params(cols, rows, W, H, TRAJ, a, b, EFFECT, ASPECT, V)
        off, _ = L.build_view_centred_offsets(cols, rows, W, H, TRAJ, ASPECT, np.full(V, a, np.float32))
        want_off = off
    if row.weights == "wide":
        hp.weights = hp.weights.copy()
        hp.weights[:, n // 2] = 0x4100     # fp16 2.5
    if row.weights == "dyadic":
        w = np.floor(ten_interval.weights_f64(hp.weights) * 4096.0) / 4096.0
        assert (w.astype(np.float16) == w).all()
        hp.weights = w.astype(np.float16).view(np.uint16)
    lf = oc.synthetic_lf(n, W, H, 0x5EED + n + W)
    if row.quant > 1:
        lf = (lf // row.quant * row.quant).astype(np.uint8)
        lf[..., 3] = 255
    maps = ids = hp_before = None
    if row.kind == "float":
        maps = random_maps(H, W, 11)
    elif row.kind == "view_maps":
        maps = {v: random_maps(H, W, 100 + v) for v in range(V)}
        ids = L.build_view_focus_ids(cols, rows, TRAJ, V)
    in_rows = ()
    if row.window:
        if row.kind == "int":
            in_rows = L.input_rows(row.window, want_off.reshape(-1, 2), H)
        else:
            in_rows = L.input_rows_all_focus(row.window, off.reshape(-1, 2), [], hp.focus, hp.range, hp.block_radius, H)
    if row.before == "plain":
        hp_before = L.build_params(cols, rows, W, H, TRAJ, a, 0.0, EFFECT, ASPECT, V)
    lf.setflags(write=False)
    return RowInputs(hp, lf, off, want_off, maps, ids, in_rows, hp_before)


def map_of(row, inp, method, v):
    """The map plane view v of a float row reads: map 1 for STD and under LFI_FLAG_UNIFIED_FOCUS_MAP, else map 0."""
    pair = inp.maps[v] if row.kind == "view_maps" else inp.maps
    return pair[1 if (method == "STD" or row.flags & UNIFIED) else 0]


@dataclass
class Expected:
    std: np.ndarray = None    # STD: [v1 − v0][rows][W][4]
    m16: np.ndarray = None    # TEN_WM …
    S: np.ndarray = None      # [v1 − v0][rows][W][3] float64
    eps: np.ndarray = None    # [v1 − v0]
    lo: np.ndarray = None
    hi: np.ndarray = None
    ties: int = 0             # dyadic rows: fp16 ties among the sums


def expected(L, oc, row, method):
    """The oracle's values of views [v0, v1) of a row (the window's rows, where it has one), per view from the view's own D[v] / O[v],
    weight row and map.  STD: the bytes.  TEN_WM: the M16 bytes, the exact sums S (blend_f64), ε (ten_interval.epsilon; 0 for a dyadic
    row after its preconditions are asserted, as test_gpu_dispatch_coverage.ten_row_interval does) and the interval [lo, hi]."""
    return _expected(L, oc, row, method)


@functools.lru_cache(maxsize=None)
def _expected(L, oc, row, method):
    inp = row_inputs(L, oc, row)
    hp, lf = inp.hp, inp.lf
    y0, y1 = row.window if row.window else (0, row.H)
    std, m16, S = [], [], []
    for v in range(row.v0, row.v1):
        w = hp.weights[v:v + 1]
        if row.kind == "int":
            args, kw = (lf, inp.oracle_offsets[v], hp.offsets, w), {}
        else:
            args = (lf, hp.focused_offsets, inp.oracle_offsets[v], w)
            kw = dict(all_focus=True, map_plane=map_of(row, inp, method, v), focus=hp.focus, rng=hp.range)
        if method == "STD":
            std.append(oc.blend_std(*args, **kw)[0, y0:y1])
        else:
            m16.append(oc.blend_ten(*args, model=oc.TEN_M16, **kw)[0, y0:y1])
            S.append(oc.blend_f64(*args, **kw)[0, y0:y1])
    if method == "STD":
        return Expected(std=np.stack(std))
    S = np.stack(S)
    eps = ten_interval.epsilon(hp.weights[row.v0:row.v1], row.n)
    n_ties = 0
    if row.weights == "dyadic":
        # multiples of 2^-12 that sum to at most 2: every product with a byte and every partial sum is a multiple of 2^-12 below 512,
        # 21 bits, exact in fp32 in any order of accumulation
        w = ten_interval.weights_f64(hp.weights)
        assert (w * 4096.0 == np.floor(w * 4096.0)).all() and (w >= 0).all() and w.sum(axis=1).max() <= 2.0, row.name
        assert (S * 4096.0 == np.floor(S * 4096.0)).all() and S.max() < 512.0, row.name
        n_ties = ten_interval.ties(S)
        assert n_ties >= DYADIC_TIES, (row.name, n_ties)
        eps = np.zeros_like(eps)
    lo, hi = ten_interval.interval(S, eps)
    return Expected(m16=np.stack(m16), S=S, eps=eps, lo=lo, hi=hi, ties=n_ties)
