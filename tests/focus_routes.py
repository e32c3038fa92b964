"""The focus-map estimate's plan and routing restated on the CPU — test infrastructure, written from the definitions (the header
of csrc/hip/focus_factored.hpp, include/lfi.h) and not from the scheduler's code — and the table of small cases that reach every leaf of the
estimate's decision tree.  tests/test_focus_routes_table.py holds the table to its claims on the CPU; tests/test_gpu_focus_routes.py runs it and
compares lfi_focus_route_info's record and the maps with what this file expects, `==` throughout.

The plan.  Candidate i of a sweep of `steps` is f_i = fmaf(range / (steps - 1), i, focus) in float32 (fma32: exact, one rounding).  Image g is
sampled for pixel coordinate c at T = (int)fmaf(f_i, offset_g, c) — the oracle's own C function gives it (warp_axis) — and the factored estimate
replaces T by the uniform shift U = c + floor(f_i * offset_g), the product exact in double.  Coordinate c is FLAGGED for candidate i on an axis
where, for any sampled image and any of the three taps t * radius (t = -1, 0, 1), the two clamped tap coordinates differ; the tap bits say at
which taps.  A pass is 32 candidates.  Its flagged (row, candidate) pairs are numbered in order of (row, candidate): the pair's line slot; pairs
whose slot is below R_cap = 4 * H have a row line, the others do not.  Columns likewise with C_cap = 4 * W.  row_entries / col_entries are the
pass's numbers of pairs.

The classes of a flagged (pixel, candidate), by who computes its key (focus_factored.hpp):
  row_line      row flagged with a slot, column unflagged: nine samples of the row's lines
  col_line      column flagged with a slot, row unflagged: nine samples of the column's lines
  corner        both flagged, both with a slot: the corner taps tap by tap, the rest from the lines and E
  a_row_noslot  both flagged, the row without a slot: the whole key tap by tap, sequence (A)
  a_col_noslot  both flagged, the row with and the column without a slot: the whole key, sequence (A)'s `whole` branch
  b             row flagged without a slot, column unflagged: sequence (B)
  c             column flagged without a slot, row unflagged: sequence (C)
"""
import functools
import os
import re
from fractions import Fraction

import numpy as np

from focus_curve_ref import map_byte

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "lfinterpolator_amd", "csrc", "hip")
TRAJ = "0.071,0.071,0.93,0.93"
CLASSES = ["row_line", "col_line", "corner", "a_row_noslot", "a_col_noslot", "b", "c"]


# ---- the constants, from the headers -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def constants():
    """what the routes hang on, parsed where it is defined: a change there fails tests/test_focus_routes_table.py instead of moving a route"""
    ff = open(os.path.join(HIP, "focus_factored.hpp")).read()
    sched = open(os.path.join(HIP, "lfi_focus_sched.hpp")).read()
    dev = open(os.path.join(HIP, "lfi_device.hpp")).read()

    def one(text, pattern):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return m[0]

    k = {}
    k["FRT_MAX_DX"], k["FRT_MAX_DY"] = (int(v) for v in one(ff, r"constexpr int FRT_MAX_DX = (\d+), FRT_MAX_DY = (\d+);"))
    k["FRT_TW"] = int(one(ff, r"constexpr int FRT_TW = (\d+);"))
    rpw = int(one(ff, r"#define FRT_RPW (\d+)"))
    lwaves = int(one(ff, r"#define FRT_LWAVES (\d+)"))
    assert one(ff, r"constexpr int FRT_NW = ([^,]+), FRT_TH = FRT_RPW \* FRT_NW;") == "FRT_RPW == 4 ? 12 - FRT_LWAVES : 12"
    k["FRT_TH"] = rpw * (12 - lwaves if rpw == 4 else 12)
    assert one(ff, r"constexpr int FRT_PR = ([^;]+);") == "FRT_TH + FRT_MAX_DY"
    k["FRT_PR"] = k["FRT_TH"] + k["FRT_MAX_DY"]
    k["FOCUS_STEPS"] = int(one(dev, r"constexpr int FOCUS_STEPS = (\d+);"))
    k["FOCUS_MAX_PASSES"] = int(one(dev, r"constexpr int FOCUS_MAX_PASSES = (\d+);"))
    k["R_CAP_FACTOR"] = int(one(sched, r"w\.R_cap = (\d+) \* H;"))
    k["C_CAP_FACTOR"] = int(one(sched, r"w\.C_cap = (\d+) \* W;"))
    k["PLANES_LIMIT"] = int(one(sched, r"pad_bytes > \(\(size_t\)(\d+) << 30\)")) << 30
    k["TYPED_LIMIT"] = 1 << int(one(sched, r"pad_bytes < \(\(size_t\)1 << (\d+)\)"))
    k["SHIFT_LIMIT"] = float(one(sched, r"fmax \* ox < (1e\d+) &&"))
    k["PICK_SEP_MAX_RX"] = int(one(sched, r"if\(ppl == 2 && rx <= (\d+) && e_32bit && !direct_range\)"))
    return k


# ---- arithmetic ----------------------------------------------------------------------------------------------------------------------------

def _round_f32(v: Fraction) -> np.float32:
    """the float32 nearest to the exact value v, ties to even"""
    x = F32(float(v))
    near = {float(c) for c in (x, np.nextafter(x, F32(np.inf)), np.nextafter(x, F32(-np.inf)))}
    return F32(min(near, key=lambda c: (abs(Fraction(c) - v), int(F32(c).view(np.uint32)) & 1)))


def fma32(a, b, c) -> np.float32:
    """fmaf(a, b, c): the exact a * b + c rounded once"""
    return _round_f32(Fraction(float(F32(a))) * Fraction(float(F32(b))) + Fraction(float(F32(c))))


def candidates(focus, rng, steps):
    """f_i = fmaf(range / (float)(steps - 1), (float)i, focus), [steps] float32"""
    step = F32(F32(rng) / F32(steps - 1))
    return np.array([fma32(step, F32(i), F32(focus)) for i in range(steps)], F32)


def sweep_shift(f, off):
    """focus_sweep_shift: floor of the product of two floats, exact in double"""
    return int(np.floor(np.float64(F32(f)) * np.float64(F32(off))))


def warp_axes(oc, f, off, W, H):
    """(int)fmaf(f, off.x, x) for every column and (int)fmaf(f, off.y, y) for every row, by the oracle's own warp (lfo_warp_coords with a map
    whose byte is 0 and range 0: the decoded focus is fmaf(0, 0, f) = f)"""
    o = np.array([[off[0], off[1]]], F32)
    xy = oc.warp_coords(0, W, H, np.zeros((1, 2), np.int32), o, all_focus=True, map_plane=np.zeros((H, W, 4), np.uint8), focus=float(F32(f)), rng=0.0)
    return xy[0, :, 0].astype(np.int64), xy[:, 0, 1].astype(np.int64)


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------

class Plan:
    """Everything the definitions give for one estimate: W, H, radius, the sampled images' offsets [n][2], the sweep.
    Xe / Xu [steps][n][3][W], Ye / Yu [steps][n][3][H]: the clamped tap coordinates, exact and by the uniform shift;
    tapx [steps][3][W], tapy [steps][3][H] bool, badx [steps][W], bady [steps][H] bool;
    row_entries, col_entries [passes]; row_slot [steps][H], col_slot [steps][W] (-1: unflagged); cls [steps][H][W] (0: unflagged, else 1 + index
    into CLASSES)."""

    def __init__(self, oc, W, H, radius, offs, focus, rng, steps=32):
        k = constants()
        S = k["FOCUS_STEPS"]
        assert steps % S == 0
        self.W, self.H, self.radius, self.offs, self.focus, self.rng, self.steps = W, H, (int(radius[0]), int(radius[1])), np.asarray(offs, F32), focus, rng, steps
        self.passes = steps // S
        self.R_cap, self.C_cap = k["R_CAP_FACTOR"] * H, k["C_CAP_FACTOR"] * W
        self.f = candidates(focus, rng, steps)
        n = len(self.offs)
        rx, ry = self.radius
        self.shifts = np.array([[[sweep_shift(f, o[0]), sweep_shift(f, o[1])] for o in self.offs] for f in self.f], np.int64)
        self.Xe, self.Xu = np.empty((steps, n, 3, W), np.int64), np.empty((steps, n, 3, W), np.int64)
        self.Ye, self.Yu = np.empty((steps, n, 3, H), np.int64), np.empty((steps, n, 3, H), np.int64)
        xs, ys = np.arange(W), np.arange(H)
        for i, f in enumerate(self.f):
            for g, o in enumerate(self.offs):
                tx, ty = warp_axes(oc, f, o, W, H)
                for t in range(3):
                    self.Xe[i, g, t] = np.clip(tx + (t - 1) * rx, 0, W - 1)
                    self.Ye[i, g, t] = np.clip(ty + (t - 1) * ry, 0, H - 1)
                    self.Xu[i, g, t] = np.clip(xs + self.shifts[i, g, 0] + (t - 1) * rx, 0, W - 1)
                    self.Yu[i, g, t] = np.clip(ys + self.shifts[i, g, 1] + (t - 1) * ry, 0, H - 1)
        self.tapx, self.tapy = (self.Xe != self.Xu).any(axis=1), (self.Ye != self.Yu).any(axis=1)
        self.badx, self.bady = self.tapx.any(axis=1), self.tapy.any(axis=1)
        self.row_entries = [int(self.bady[p * S:(p + 1) * S].sum()) for p in range(self.passes)]
        self.col_entries = [int(self.badx[p * S:(p + 1) * S].sum()) for p in range(self.passes)]
        self.row_slot, self.col_slot = self._slots(self.bady, S), self._slots(self.badx, S)
        by, bx = self.bady[:, :, None], self.badx[:, None, :]
        rs = (self.row_slot < self.R_cap)[:, :, None]
        cs = (self.col_slot < self.C_cap)[:, None, :]
        c = np.zeros((steps, H, W), np.int8)
        c[by & ~bx & rs] = 1
        c[bx & ~by & cs] = 2
        c[by & bx & rs & cs] = 3
        c[by & bx & ~rs] = 4
        c[by & bx & rs & ~cs] = 5
        c[by & ~bx & ~rs] = 6
        c[bx & ~by & ~cs] = 7
        self.cls = c

    @staticmethod
    def _slots(bad, S):
        """base plus the popcount below i: the flagged pairs of a pass numbered in order of (coordinate, candidate)"""
        slot = np.full(bad.shape, -1, np.int64)
        for p in range(bad.shape[0] // S):
            b = bad[p * S:(p + 1) * S]                  # [32][L]
            order = np.cumsum(b.T.reshape(-1)) - 1      # (coordinate, candidate) order
            slot[p * S:(p + 1) * S] = np.where(b, order.reshape(b.T.shape).T, -1)
        return slot

    def classes(self):
        """the classes that occur, as names"""
        return {CLASSES[v - 1] for v in np.unique(self.cls) if v}


def keys(lf, ids, X, Y):
    """The comparison key of every pixel for ONE candidate from clamped tap coordinates X [n][3][W], Y [n][3][H]: 16 * (the sum over the nine
    taps of the largest channel's range over the sampled images), or, where that sum is 0, the number of taps one of whose channels is 0 in
    every sampled image (the reference's FLT_MIN start value: tests/focus_steps_ref.py)."""
    S = 0
    tiny = 0
    for tx in range(3):
        for ty in range(3):
            px = np.stack([lf[g][np.ix_(Y[k, ty], X[k, tx])][..., :3] for k, g in enumerate(ids)]).astype(np.int64)
            hi, lo = px.max(axis=0), px.min(axis=0)
            r = (hi - lo).max(axis=-1)
            S = S + r
            tiny = tiny + ((r == 0) & (hi.min(axis=-1) == 0))
    return np.where(S > 0, 16 * S, tiny)


def key_planes(plan, lf, ids):
    """(exact [steps][H][W], uniform [steps][H][W]): every candidate's keys by the reference's coordinates and by the uniform shift"""
    exact = np.stack([keys(lf, ids, plan.Xe[i], plan.Ye[i]) for i in range(plan.steps)])
    unif = np.stack([keys(lf, ids, plan.Xu[i], plan.Yu[i]) for i in range(plan.steps)])
    return exact, unif


def map0_of(plan, key):
    """map 0's byte plane [H][W] from the keys: the first strictly smallest"""
    return map_byte(plan.f[np.argmin(key, axis=0)], plan.focus, plan.rng)


def naive_map0(plan, exact, unif, cls_name):
    """map 0 as a kernel gives it that skipped the class (or read a stale slot): the uniform-shift key at the class's pairs"""
    return map0_of(plan, np.where(plan.cls == 1 + CLASSES.index(cls_name), unif, exact))


# ---- the route -----------------------------------------------------------------------------------------------------------------------------

class PadState:
    """what a context remembers of its padded planes between estimate calls: the geometry they were padded for and, per
    slot, the image they hold.  `dirty`: images uploaded since."""

    def __init__(self):
        self.shift, self.radius, self.ids, self.dirty, self.valid = [0, 0], None, [], set(), False


def pad_request(offs, focus, rng):
    """the padding an estimate asks for: the largest |shift| of any candidate of any sweep length, + 1; None where it is absurd"""
    k = constants()
    fmax = abs(float(F32(focus)))
    S = k["FOCUS_STEPS"]
    for steps in range(S, S * k["FOCUS_MAX_PASSES"] + 1, S):
        fmax = max(fmax, abs(float(fma32(F32(F32(rng) / F32(steps - 1)), F32(steps - 1), F32(focus)))))
    o = np.abs(np.asarray(offs, np.float64))
    ox, oy = float(o[:, 0].max()), float(o[:, 1].max())
    if not (fmax * ox < k["SHIFT_LIMIT"] and fmax * oy < k["SHIFT_LIMIT"]):
        return None
    return int(np.ceil(fmax * ox)) + 1, int(np.ceil(fmax * oy)) + 1


def group_size(offs, f_pass, direct, pad_bytes):
    """candidates per group of the range pass: 8 where every image's shifts span at most FRT_MAX_DX x FRT_MAX_DY within every group of 8
    consecutive candidates of the pass, else 4 by the same rule, else 0 (focus_range); 0 too for the direct variant and for planes that typed
    loads cannot address"""
    k = constants()
    if direct or pad_bytes >= k["TYPED_LIMIT"]:
        return 0
    for cpw in (8, 4):
        ok = True
        for o in offs:
            s = np.array([[sweep_shift(f, o[0]), sweep_shift(f, o[1])] for f in f_pass]).reshape(len(f_pass) // cpw, cpw, 2)
            span = s.max(axis=1) - s.min(axis=1)
            ok = ok and bool((span[:, 0] <= k["FRT_MAX_DX"]).all() and (span[:, 1] <= k["FRT_MAX_DY"]).all())
        if ok:
            return cpw
    return 0


def keys_ppl(W, rx):
    return 2 if rx % 2 == 0 and W >= 2 else 1


def expected_route(W, H, radius, offs, ids, focus, rng, steps=32, variant="factored", consumer="pick", state=None, need_shift=(0, 0), slot_reuse=False,
                   plan=None):
    """lfi_focus_route's fields for one factored job on a context in `state` (None: fresh), as a dict without calls / jobs; updates `state`.
    consumer: "pick" (lfi_focus_map, lfi_view_focus_maps) or "tiles".  The per-pass counts are the plan's, where one is given."""
    k = constants()
    S = k["FOCUS_STEPS"]
    rx, ry = int(radius[0]), int(radius[1])
    direct = variant == "factored_direct"
    state = state if state is not None else PadState()
    ids = [int(g) for g in ids]
    n = len(ids)
    empty = dict(estimate="", declined="", passes=0, range_striped=0, range_kernel="", consumer="", consumer_striped=0, planes_padded=0, planes_kept=0,
                 pad_shift=[0, 0], We_p=0, He_p=0, Wp=0, Hp=0, R_cap=0, C_cap=0, range_cpw=[], row_entries=[], col_entries=[])
    need = pad_request(offs, focus, rng)
    if need is None:
        return dict(empty, declined="shift")
    need = [max(need[0], need_shift[0]), max(need[1], need_shift[1])]
    same_ids = len(state.ids) == n if slot_reuse else state.ids == ids
    kept = state.valid and same_ids and state.radius == (rx, ry) and state.shift[0] >= need[0] and state.shift[1] >= need[1]
    if kept:
        Sx, Sy = state.shift
    else:
        grow = lambda want, had: ((want + want // 4 if had > 0 and want > had else want) + 7) // 8 * 8
        Sx, Sy = grow(need[0], state.shift[0]), grow(need[1], state.shift[1])
    We_p, He_p = (W + 2 * rx + 255) // 256 * 256, (H + 2 * ry + 3) // 4 * 4
    Px, Py = Sx + rx, Sy + ry
    Wp = (Px + max(W + Sx + rx, We_p - rx + Sx) + 3) // 4 * 4
    Hp = Py + max(H + Sy + ry, He_p - ry + Sy)
    pad_bytes = 4 * (n * Hp + k["FRT_PR"] + 16) * Wp
    if pad_bytes > k["PLANES_LIMIT"]:
        return dict(empty, declined="planes")
    if kept:
        redo = [j for j in range(n) if state.ids[j] != ids[j] or ids[j] in state.dirty]
    else:
        redo = list(range(n))
        state.shift, state.radius = [Sx, Sy], (rx, ry)
    state.ids, state.dirty, state.valid = ids, set(), True
    f = candidates(focus, rng, steps)
    cpw = [group_size(np.asarray(offs, F32), f[p * S:(p + 1) * S], direct, pad_bytes) for p in range(steps // S)]
    last = cpw[-1]
    striped = int((We_p // k["FRT_TW"] if last else We_p // 256) >= 8)
    ppl = keys_ppl(W, rx)
    blocks_x = (W + 64 * ppl - 1) // (64 * ppl)
    carry = steps > S
    if consumer == "tiles":
        name, cstriped = "focus_tile_costs<%d>" % ppl, 0
    elif ppl == 2 and rx <= k["PICK_SEP_MAX_RX"] and 2 * He_p * We_p < (1 << 31) and not direct:
        name, cstriped = "focus_pick_sep_carry" if carry else "focus_pick_sep", 0
    else:
        name, cstriped = ("focus_pick_carry<%d>" if carry else "focus_pick<%d>") % ppl, int(blocks_x >= 8)
    return dict(estimate=variant, declined="", passes=steps // S, range_striped=striped,
                range_kernel="focus_range_t<%d>" % last if last else "focus_range<4>", consumer=name, consumer_striped=cstriped,
                planes_padded=len(redo), planes_kept=n - len(redo), pad_shift=[Sx, Sy], We_p=We_p, He_p=He_p, Wp=Wp, Hp=Hp,
                R_cap=k["R_CAP_FACTOR"] * H, C_cap=k["C_CAP_FACTOR"] * W, range_cpw=cpw,
                row_entries=plan.row_entries if plan is not None else None, col_entries=plan.col_entries if plan is not None else None)


def assert_variant(ctx, variant, hp, steps=32, consumer="pick"):
    """for the suites that run VARIANTS = auto / factored_direct / packed_p2: the last estimate call of `ctx` was answered by the estimate the
    variant names (packed_p2: the packed kernel for a map, lfi_focus_curve's kernels for tiles) with every pass run, and under `auto` the
    range pass of every pass of the sweep is the one the restatement expects"""
    got = ctx.focus_route()
    factored = variant != "packed_p2"
    want = {"auto": "factored", "factored_direct": "factored_direct", "packed_p2": "focus_curve" if consumer == "tiles" else "packed_p2"}[variant]
    assert (got["estimate"], got["declined"], got["passes"]) == (want, "", steps // 32 if factored else 0), (variant, got)
    if variant == "auto":
        ids = hp.focus_map_ids
        route = expected_route(ctx.width, ctx.height, hp.block_radius, hp.offsets[ids], ids, hp.focus, hp.range, steps, "factored", consumer)
        assert (got["range_kernel"], got["range_cpw"], got["consumer"]) == (route["range_kernel"], route["range_cpw"], route["consumer"]), (got, route)
    return got


def route_matches(got, want):
    """the fields of `want` (None: not restated) against the record; the list of differing fields"""
    return [name for name, v in want.items() if v is not None and got[name] != v]


# ---- the table -----------------------------------------------------------------------------------------------------------------------------

# Every leaf of the estimate's decision tree the table must reach (leaves_of computes a case's from the restatement alone).
LEAVES = (
    # the range pass: groups of 8, of 4, the fall-back under `factored`, the direct variant; the order of the work items
    ["focus_range_t<8>", "focus_range_t<4>", "focus_range<4> fall-back", "focus_range<4> direct", "focus_range_t<8> striped", "focus_range_t<4> striped",
     "focus_range<4> striped", "focus_range_t plain order", "focus_range<4> plain order"]
    # the consumers
    + ["focus_pick_sep", "focus_pick_sep_carry", "focus_pick<2>", "focus_pick_carry<2>", "focus_pick<1>", "focus_pick_carry<1>", "pick striped", "pick plain order",
       "radius_x 64", "radius_x 66", "W = 1", "focus_tile_costs<1>", "focus_tile_costs<2>"]
    + ["one sampled view", "two sampled views", "negative focus"]
    + ["class " + c for c in CLASSES]
    + ["both overflows", "column overflow beside flagged rows", "rows above R_cap by at most 4", "rows below R_cap by at most 4", "columns at C_cap exactly",
       "columns above C_cap by at most 4", "columns below C_cap by at most 4"]
    + ["sweep: first pass overflows, a later one does not", "sweep: a later pass overflows, the first does not", "64 candidates", "256 candidates"]
    + ["declined: shift", "declined: planes", "row window"]
    + ["planes kept", "planes rebuilt", "planes grown by a quarter", "planes kept but for the uploaded image", "slot-stable re-padding"]
)


def case(name, cols, rows, W, H, f, r, radii=None, steps=32, leaves=(), classes=(), more=(), seed=0):
    return dict(name=name, cols=cols, rows=rows, W=W, H=H, focus=f, range=r, radii=radii, steps=steps, leaves=tuple(leaves), classes=tuple(classes),
                more=tuple(more), seed=seed)


def build(L, oc, c):
    """a case's parameters and inputs: build_params on TRAJ, synthetic_lf quantised to 16 levels with a black region (ties, FLT_MIN taps)"""
    hp = L.build_params(c["cols"], c["rows"], c["W"], c["H"], TRAJ, c["focus"], c["range"], 3.0, 1.783, 2)
    if c["radii"]:
        hp.block_radius = np.array(c["radii"], np.int32)
    W, H = c["W"], c["H"]
    lf = oc.synthetic_lf(c["cols"] * c["rows"], W, H, 4242 + c["seed"] + 7 * W + H)
    lf = (lf // 16 * 16).astype(np.uint8)
    lf[:, : H // 3, W // 2:, :3] = 0
    lf[..., 3] = 255
    return hp, lf


def plan_of(L, oc, c, hp=None):
    hp = hp or build(L, oc, c)[0]
    return Plan(oc, c["W"], c["H"], hp.block_radius, hp.offsets[hp.focus_map_ids], hp.focus, hp.range, c["steps"])


def leaves_of(c, hp, plan):
    """the leaves a case reaches on a fresh context, by the restatement: under `factored` and `factored_direct`, lfi_focus_map; the tile costs
    for the cases that ask for them (more: "tiles")"""
    out = set()
    W, H = c["W"], c["H"]
    offs, ids = hp.offsets[hp.focus_map_ids], hp.focus_map_ids
    for variant in ("factored", "factored_direct"):
        r = expected_route(W, H, hp.block_radius, offs, ids, hp.focus, hp.range, c["steps"], variant)
        if r["declined"]:
            out.add("declined: " + r["declined"])
            continue
        for cpw in r["range_cpw"]:
            out.add("focus_range_t<%d>" % cpw if cpw else "focus_range<4> direct" if variant == "factored_direct" else "focus_range<4> fall-back")
        out.add(r["range_kernel"] + " striped" if r["range_striped"] else ("focus_range_t" if r["range_cpw"][-1] else "focus_range<4>") + " plain order")
        out.add(r["consumer"])
        if r["consumer"].startswith("focus_pick") and "sep" not in r["consumer"]:
            out.add("pick striped" if r["consumer_striped"] else "pick plain order")
        if "tiles" in c["more"]:
            out.add(expected_route(W, H, hp.block_radius, offs, ids, hp.focus, hp.range, c["steps"], variant, "tiles")["consumer"])
    out |= {"row window"} if "row_window" in c["more"] else set()
    if out <= {"declined: shift", "declined: planes"}:
        return out
    rx = int(hp.block_radius[0])
    out |= {"radius_x %d" % rx} if rx in (64, 66) else set()
    out |= {"W = 1"} if W == 1 else set()
    out |= {"one sampled view"} if len(ids) == 1 else {"two sampled views"} if len(ids) == 2 else set()
    out |= {"negative focus"} if hp.focus < 0 else set()
    out |= {"class " + n for n in plan.classes()}
    over_r = [e - plan.R_cap for e in plan.row_entries]
    over_c = [e - plan.C_cap for e in plan.col_entries]
    for dr, dc, rows_flagged in zip(over_r, over_c, plan.row_entries):
        out |= {"both overflows"} if dr > 0 and dc > 0 else set()
        out |= {"column overflow beside flagged rows"} if dc > 0 and dr <= 0 and rows_flagged > 0 else set()
        out |= {"rows above R_cap by at most 4"} if 0 < dr <= 4 else set()
        out |= {"rows below R_cap by at most 4"} if -4 <= dr < 0 else set()
        out |= {"columns at C_cap exactly"} if dc == 0 else set()
        out |= {"columns above C_cap by at most 4"} if 0 < dc <= 4 else set()
        out |= {"columns below C_cap by at most 4"} if -4 <= dc < 0 else set()
    over = [dr > 0 or dc > 0 for dr, dc in zip(over_r, over_c)]
    if len(over) > 1:
        out |= {"sweep: first pass overflows, a later one does not"} if over[0] and not all(over[1:]) else set()
        out |= {"sweep: a later pass overflows, the first does not"} if not over[0] and any(over[1:]) else set()
        out |= {"%d candidates" % c["steps"]}
    return out


# The cases.  cols x rows, W x H, focus, range, radii; `leaves`: what the case is in the table for (it may reach more); `classes`: the classes of
# flagged pairs it claims — tests/test_focus_routes_table.py shows for each that skipping the class changes map 0 in a claiming case;
# `more`: the other estimate calls the GPU test runs on it ("tiles", "tile_steps", "view_maps").
CASES = [
    # the range pass
    case("t4", 4, 4, 64, 16, -4, 8, (4, 2), leaves=["focus_range_t<4>", "focus_range_t plain order", "negative focus"]),
    case("fallback", 4, 4, 64, 16, -9, 18, (4, 2), leaves=["focus_range<4> fall-back", "focus_range<4> plain order"]),
    case("t8_striped", 2, 2, 300, 6, 0.2, 0.3, (4, 2), leaves=["focus_range_t<8> striped", "focus_range<4> direct"]),
    case("t4_striped", 4, 4, 300, 8, -1, 2, (4, 2), leaves=["focus_range_t<4> striped"]),
    case("direct_striped", 2, 1, 1800, 4, 0.2, 0.3, (4, 1), leaves=["focus_range<4> striped", "pick striped", "two sampled views"]),
    # the consumers
    case("pick1_striped", 3, 3, 450, 5, 0.22, 0.3, (3, 1), leaves=["focus_pick<1>", "pick striped"], more=["tiles"]),
    case("rx64", 3, 3, 70, 8, 0.22, 0.3, (64, 2), leaves=["radius_x 64", "focus_pick_sep", "focus_pick<2>", "pick plain order"], more=["tiles"]),
    case("rx66", 3, 3, 70, 8, 0.22, 0.3, (66, 2), leaves=["radius_x 66", "focus_pick<2>"]),
    case("w1", 3, 3, 1, 9, -0.5, 1.0, (2, 2), leaves=["W = 1", "focus_pick<1>"], more=["tiles"]),
    case("one_view", 1, 1, 20, 10, 0.2, 0.3, (2, 1), leaves=["one sampled view", "focus_range_t<8>"]),
    case("two_views", 2, 1, 7, 5, 0.3, 0.5, (1, 1), leaves=["two sampled views", "columns above C_cap by at most 4", "class c"], seed=1),
    # the line buffers' caps
    case("both_overflows", 4, 4, 8, 8, -1, 2, (2, 2), leaves=["both overflows", "class a_row_noslot", "class a_col_noslot", "class c"],
         more=["tiles", "view_maps"]),
    case("col_overflow", 4, 4, 8, 24, -1, 2, (2, 2), leaves=["column overflow beside flagged rows", "class a_col_noslot", "class c"], more=["tiles"]),
    case("rows_above", 8, 8, 33, 17, 0.1, 0.4, leaves=["rows above R_cap by at most 4", "class b", "class a_row_noslot"], seed=10),
    case("rows_below", 8, 8, 33, 17, 0.1, 0.35, leaves=["rows below R_cap by at most 4", "class row_line", "class col_line", "class corner"]),
    case("cols_below", 8, 8, 12, 40, -0.5, 0.98, (4, 2), leaves=["columns below C_cap by at most 4"]),
    case("cols_at_cap", 8, 8, 12, 40, -0.5, 1.0, (4, 2), leaves=["columns at C_cap exactly"]),
    case("cols_above", 8, 8, 12, 40, -0.5, 1.05, (4, 2), leaves=["columns above C_cap by at most 4", "class c"], seed=6),
    # sweeps of several passes: every pass rewrites the plan, Er, Ec and K
    case("sweep64_first", 4, 4, 16, 12, -0.5, 0.5, (2, 2), 64, leaves=["sweep: first pass overflows, a later one does not", "64 candidates", "focus_pick_sep_carry",
                                                                       "focus_pick_carry<2>"], more=["tile_steps"]),
    case("sweep64_later", 4, 4, 8, 8, -0.2, 1.0, (2, 2), 64, leaves=["sweep: a later pass overflows, the first does not", "64 candidates"], more=["tile_steps"]),
    case("sweep256_first", 4, 4, 8, 8, -1, 1.0, (2, 2), 256, leaves=["sweep: first pass overflows, a later one does not", "256 candidates"], more=["tile_steps"]),
    case("sweep256_later", 4, 4, 8, 8, -0.2, 1.0, (1, 1), 256, leaves=["sweep: a later pass overflows, the first does not", "256 candidates", "focus_pick_carry<1>"]),
    # the factored estimate declines, another variant answers; a row window
    case("declined_shift", 2, 2, 8, 8, 3e6, 1.0, (2, 2), leaves=["declined: shift"], more=["tiles"]),
    case("declined_planes", 2, 2, 8, 8, 40000.0, 1.0, (2, 2), leaves=["declined: planes"]),
    case("row_window", 4, 4, 33, 24, 0.1, 0.2, (2, 2), leaves=["row window"], more=["row_window"]),
]

# The oracle's map 0 of a case shows at least this many distinct values (the focus tests' measure of a map that is not degenerate): 5, but for
DISTINCT_MIN = {
    "one_view": 1,          # one sampled image has no dispersion: every candidate ties, the map is 0 by definition
    "declined_shift": 1,    # every sample of every candidate clamps to the same edge pixel
    "declined_planes": 1,
    "w1": 2,                # nine pixels in a column
    "two_views": 2,         # 35 pixels, two images
}

# The classes whose skipping changes map 0 of the case (naive_map0), as the exact restatement found them: the table test recomputes each.
CLASS_SHOWS = {
    "t4": ["row_line", "col_line", "corner", "b"],
    "fallback": ["row_line", "col_line", "corner"],
    "rx64": ["row_line", "col_line", "corner", "a_row_noslot", "b", "c"],
    "two_views": ["col_line", "c"],
    "both_overflows": ["row_line", "col_line", "corner", "a_row_noslot", "a_col_noslot", "c"],
    "col_overflow": ["row_line", "col_line", "a_col_noslot", "c"],
    "rows_above": ["row_line", "col_line", "corner", "a_row_noslot", "b"],
    "rows_below": ["row_line", "col_line", "corner"],
    "cols_at_cap": ["row_line", "col_line", "corner"],
    "cols_above": ["row_line", "col_line", "corner", "a_col_noslot", "c"],
    "sweep64_first": ["row_line", "col_line", "corner", "a_col_noslot", "b", "c"],
    "sweep64_later": ["row_line", "col_line", "corner"],
    "sweep256_first": ["col_line", "corner", "a_row_noslot", "a_col_noslot", "c"],
    "sweep256_later": ["row_line", "corner", "a_row_noslot", "a_col_noslot", "c"],
}


def pixel_costs(key):
    """the focus curve's per-pixel cost S from the keys: the FLT_MIN terms dropped (include/lfi.h)"""
    return np.where(key >= 16, key // 16, 0)


# ---- the padded planes between calls -------------------------------------------------------------------------------------------------------

# One context, lfi_focus_map after each step: (what, focus, range, radii, image of the sampled ones uploaded again or None).
PAD_SHAPE = dict(cols=4, rows=4, W=40, H=20)
PAD_SEQUENCE = [
    ("fresh", 0.1, 0.2, (2, 2), None),
    ("again", 0.1, 0.2, (2, 2), None),
    ("a smaller interval", 0.1, 0.1, (2, 2), None),
    ("a larger interval", 0.1, 1.3, (2, 2), None),
    ("one image uploaded again", 0.1, 1.3, (2, 2), 1),
    ("another radius", 0.1, 0.5, (4, 2), None),
]


def pad_sequence_routes(L, steps=PAD_SEQUENCE):
    """[(hp, expected route, leaves)] of PAD_SEQUENCE on one context, variant `factored`"""
    state, out = PadState(), []
    for what, f, r, radii, again in steps:
        hp = L.build_params(PAD_SHAPE["cols"], PAD_SHAPE["rows"], PAD_SHAPE["W"], PAD_SHAPE["H"], TRAJ, f, r, 3.0, 1.783, 2)
        hp.block_radius = np.array(radii, np.int32)
        ids = hp.focus_map_ids
        if again is not None:
            state.dirty.add(int(ids[again]))
        had = list(state.shift)
        r_ = expected_route(PAD_SHAPE["W"], PAD_SHAPE["H"], radii, hp.offsets[ids], ids, f, r, 32, "factored", state=state)
        need = pad_request(hp.offsets[ids], f, r)
        leaves = set()
        if r_["planes_padded"] == 0:
            leaves.add("planes kept")
        elif r_["planes_padded"] == len(ids):
            leaves.add("planes rebuilt")
            plain = [(v + 7) // 8 * 8 for v in need]
            if r_["pad_shift"] != plain and (need[0] > had[0] > 0 or need[1] > had[1] > 0):
                leaves.add("planes grown by a quarter")
        else:
            leaves.add("planes kept but for the uploaded image")
        out.append((what, hp, again, r_, leaves))
    return out


def slot_order(prev, ids):
    """lfi_view_focus_maps' slots: an image the planes already hold (prev, slot by slot) keeps its slot where the sets have the same size; the
    others take the free slots in ascending order"""
    n = len(ids)
    out, placed = [-1] * n, [False] * n
    if len(prev) == n:
        for k in range(n):
            for j in range(n):
                if not placed[j] and ids[j] == prev[k]:
                    out[k], placed[j] = int(ids[j]), True
                    break
    free = [k for k in range(n) if out[k] < 0]
    for j in range(n):
        if not placed[j]:
            out[free.pop(0)] = int(ids[j])
    return out


def view_maps_route(W, H, radius, O, ids_vk, focus, rng, variant="factored", state=None):
    """lfi_view_focus_maps' record on a context in `state`: the last view's job, the batch's planes_padded / planes_kept, jobs = the views"""
    state = state if state is not None else PadState()
    V = len(ids_vk)
    prev, rows, need = list(state.ids), [], [0, 0]
    for v in range(V):
        row = slot_order(prev, [int(g) for g in ids_vk[v]])
        prev = row
        rows.append(row)
        want = pad_request(O[v][row], focus, rng)
        need = [max(need[0], want[0]), max(need[1], want[1])]
    padded = kept = 0
    for v in range(V):
        r = expected_route(W, H, radius, O[v][rows[v]], rows[v], focus, rng, 32, variant, state=state, need_shift=need, slot_reuse=True)
        padded, kept = padded + r["planes_padded"], kept + r["planes_kept"]
    return dict(r, planes_padded=padded, planes_kept=kept, jobs=V, row_entries=None, col_entries=None), rows
