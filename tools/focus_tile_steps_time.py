"""Fine focus tiles (lfi_focus_tiles_steps): what all tiles' focus curves cost with 64, 128 and 256 candidates, against lfi_focus_tiles (32
candidates) and the whole-frame lfi_focus_curve, on this build and — for the rows both builds have — on another build of the library (the
parent commit's) in the same process.  Per case (the shapes and the scene of tools/focus_tiles_time.py: BASELINE configs 2 and 5, the
structured scene of lfi_fill_synthetic_scene, 32 sampled images), ONE process, HIP events around the calls (they are synchronous: the
device-to-host copy is inside), medians of `runs` timed runs after `warm` warm-ups:
  (a) lfi_focus_tiles(16, 9) — on the OTHER build (LFI_OTHER_LIB=path/to/liblfi_hip.so; without it the row is left out) and on this one,
      alternating, `rounds` times each, on two contexts that hold the same scene; the spread of the repeated medians is the margin;
  (b) lfi_focus_curve(0, 0, W, H, steps), likewise on both builds (one round: it is the slow path);
  (c) lfi_focus_tiles_steps(16, 9, steps);
  (d) lfi_focus_tiles_steps(1, 1, steps);
for steps = 64, 128, 256, and (c) at 32 (= lfi_focus_tiles).  Bar 1: (c), (d) <= 1.10 x steps / 32 x (a) of the other build; bar 2: (d) < (b).
usage: [LFI_OTHER_LIB=...] python tools/focus_tile_steps_time.py [runs=20] [warm=3] [rounds=3] [case ...]   cases: 8x8, 4k (default: both)"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, ".")
import numpy as np

import lfinterpolator_amd as L

CASES = {
    # name: cols, rows, W, H, trajectory, focus, range, views
    "8x8": (8, 8, 1920, 1080, "0,0,1,1", 0.0, 0.5, 64),
    "4k": (15, 15, 3840, 2160, "0.071,0.071,0.93,0.93", 0.22, 0.17, 32),
}
TILES = (16, 9)
STEPS = (64, 128, 256)
args = sys.argv[1:]
runs = int(args[0]) if args else 20
warm = int(args[1]) if len(args) > 1 else 3
rounds = int(args[2]) if len(args) > 2 else 3
names = args[3:] or list(CASES)
other_path = os.environ.get("LFI_OTHER_LIB")


def context_on(path):
    """a Context whose calls go to another build of the library: the signatures of this build's functions, for the symbols that build exports"""
    cur = L.load_hip_library()
    lib = C.CDLL(path)
    for name in L.abi.ABI_SYMBOLS:
        if hasattr(lib, name):
            getattr(lib, name).restype = getattr(cur, name).restype
            getattr(lib, name).argtypes = getattr(cur, name).argtypes
    ctx = L.Context.__new__(L.Context)
    ctx._lib = lib
    handle = C.c_void_p()
    assert lib.lfi_create(0, C.byref(handle)) == 0
    ctx._h, ctx.device, ctx._keep, ctx._pinned = handle, 0, None, []
    ctx.cols = ctx.rows = ctx.width = ctx.height = ctx.views = 0
    return ctx


def timed(ctx, fn, n=None, w=None):
    for _ in range(warm if w is None else w):
        fn()
        ctx.sync()
    ev = []
    for _ in range(runs if n is None else n):
        ctx.timer_start()
        fn()
        ev.append(ctx.timer_stop())
    return round(float(np.median(ev)), 4)


for name in names:
    cols, rows, W, H, traj, f, r, V = CASES[name]
    hp = L.build_params(cols, rows, W, H, traj, f, r, 3.0, 1.0, V)
    row = {"case": name, "grid": f"{cols}x{rows}", "res": f"{W}x{H}", "focus": f, "range": r, "n_ids": int(len(hp.focus_map_ids)), "tiles": "16x9",
           "runs": runs, "warm": warm, "rounds": rounds, "other_lib": bool(other_path)}
    ctxs = {"this": L.Context(0)}
    if other_path:
        ctxs["other"] = context_on(other_path)
    for ctx in ctxs.values():
        ctx.set_grid(cols, rows, W, H)
        ctx.set_params(hp)
        ctx.fill_synthetic_scene(0x1F1F)
        ctx.sync()
    this = ctxs["this"]
    medians = {k: [] for k in ctxs}
    for _ in range(rounds):                      # other, this, other, this, …
        for k in sorted(ctxs):
            medians[k].append(timed(ctxs[k], lambda c=ctxs[k]: c.focus_tiles(*TILES)))
    for k in sorted(ctxs):
        row[f"a_{k}_medians_ms"] = medians[k]
        row[f"a_{k}_ms"] = round(float(np.median(medians[k])), 4)
        row[f"a_{k}_spread_ms"] = round(max(medians[k]) - min(medians[k]), 4)
    base = row["a_other_ms"] if other_path else row["a_this_ms"]
    row["g_times"] = "a_other" if other_path else "a_this"
    row["c_32_raw_ms"] = timed(this, lambda: this._lib.lfi_focus_tiles_steps(this._h, *TILES, 32, None, (L.abi.FocusCurveResult * 144)()))
    for steps in STEPS:
        slow = max(3, runs // 4)                 # the curve path takes tens to hundreds of milliseconds a call
        for k in sorted(ctxs):
            row[f"b_{k}_{steps}_ms"] = timed(ctxs[k], lambda c=ctxs[k]: c.focus_curve(0, 0, W, H, steps=steps), n=slow, w=1)
        row[f"c_{steps}_ms"] = timed(this, lambda: this.focus_tiles(*TILES, steps=steps))
        assert this.focus_tiles_passes() == steps // 32
        row[f"d_{steps}_ms"] = timed(this, lambda: this.focus_tiles(1, 1, steps=steps))
        assert this.focus_tiles_passes() == steps // 32
        G = steps // 32
        row[f"c_{steps}_over_G_a"] = round(row[f"c_{steps}_ms"] / (G * base), 4)
        row[f"d_{steps}_over_G_a"] = round(row[f"d_{steps}_ms"] / (G * base), 4)
        row[f"b_over_d_{steps}"] = round(row[f"b_this_{steps}_ms"] / row[f"d_{steps}_ms"], 2)
        whole, best, _ = this.focus_tiles(1, 1, steps=steps)
        curve, cbest, _ = this.focus_curve(0, 0, W, H, steps=steps)
        assert (whole[0, 0] == curve).all() and best[0, 0] == cbest
    row["workspace_bytes"] = int(this.memory_info().workspace_bytes)
    row["box_ten_wm_launch_ms"] = round(this.benchmark("TEN_WM", warmup=3, runs=20).median_ms, 4)
    for ctx in ctxs.values():
        ctx.close()
    print(json.dumps(row), flush=True)
