"""Fine focus maps (lfi_set_focus_steps): what lfi_focus_map costs with 32, 64, 128 and 256 candidates, against the same call on another
build of the library (the parent commit's) in the same process.  Per case (the shapes and the scene of tools/focus_tiles_time.py: BASELINE
configs 2 and 5, the structured scene of lfi_fill_synthetic_scene, 32 sampled images), ONE process, HIP events around the GPU work, medians of
`runs` timed runs after `warm` warm-ups:
  (a) lfi_focus_map at 32 steps on the OTHER build (LFI_OTHER_LIB=path/to/liblfi_hip.so; without it the row is left out);
  (b) the same at 32 steps on this build — (a) and (b) alternate, `rounds` times each, on two contexts that hold the same scene; the spread
      of the medians of the repeated (a) runs is the margin (b) is judged by;
  (c)-(e) 64, 128 and 256 steps on this build — the expectation is "not above G x (a)", G = steps / 32 (the padded planes and the plan are shared);
  (f) "packed_p2" at 128 steps (one run: it takes seconds at 4K).
The two contexts are not interchangeable (where their buffers lie differs): a CONTROL run with LFI_OTHER_LIB pointing at a copy of this
build's own library shows what the slots alone contribute, and (a) is compared with that run's (a).
Also: the share of pixels whose 128-step map-0 byte differs from the 32-step byte.
usage: [LFI_OTHER_LIB=...] python tools/focus_steps_time.py [runs=20] [warm=3] [rounds=3] [case ...]   cases: 8x8, 4k (default: both)"""
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


def timed(ctx, fn, n=None):
    for _ in range(warm):
        fn()
        ctx.sync()
    ev = []
    for _ in range(runs if n is None else n):
        ctx.timer_start()
        fn()
        ev.append(ctx.timer_stop())
    return round(float(np.median(ev)), 4), [round(x, 4) for x in ev]


for name in names:
    cols, rows, W, H, traj, f, r, V = CASES[name]
    hp = L.build_params(cols, rows, W, H, traj, f, r, 3.0, 1.0, V)
    row = {"case": name, "grid": f"{cols}x{rows}", "res": f"{W}x{H}", "focus": f, "range": r, "n_ids": int(len(hp.focus_map_ids)), "runs": runs,
           "warm": warm, "rounds": rounds, "other_lib": bool(other_path)}
    ctxs = {"b": L.Context(0)}
    if other_path:
        ctxs["a"] = context_on(other_path)
    for ctx in ctxs.values():
        ctx.set_grid(cols, rows, W, H)
        ctx.set_params(hp)
        ctx.fill_synthetic_scene(0x1F1F)
        ctx.sync()
    this = ctxs["b"]
    medians = {k: [] for k in ctxs}
    for _ in range(rounds):                      # a, b, a, b, …
        for k in sorted(ctxs):
            medians[k].append(timed(ctxs[k], ctxs[k].focus_map)[0])
    for k in sorted(ctxs):
        row[f"{k}_32_medians_ms"] = medians[k]
        row[f"{k}_32_ms"] = round(float(np.median(medians[k])), 4)
        row[f"{k}_32_spread_ms"] = round(max(medians[k]) - min(medians[k]), 4)
    base = row["a_32_ms"] if other_path else row["b_32_ms"]
    row["g_times"] = "a" if other_path else "b"
    maps = {32: this.download_map(0)}
    for key, steps in (("c", 64), ("d", 128), ("e", 256)):
        this.set_focus_steps(steps)
        row[f"{key}_{steps}_ms"], row[f"reps_{key}"] = timed(this, this.focus_map)
        row[f"{key}_over_G_times_32"] = round(row[f"{key}_{steps}_ms"] / (steps // 32 * base), 4)
        if steps == 128:
            this.sync()
            maps[128] = this.download_map(0)
    row["share_of_pixels_128_differs_from_32"] = round(float((maps[128][..., 0] != maps[32][..., 0]).mean()), 4)
    this.set_variant("FOCUS", "packed_p2")
    this.set_focus_steps(128)
    this.focus_map()
    this.sync()
    row["f_packed_p2_128_ms"], _ = timed(this, this.focus_map, n=1)
    assert (this.download_map(0) == maps[128]).all()
    row["workspace_bytes"] = int(this.memory_info().workspace_bytes)
    # the headline launch time of this box, as the other notes record it — last: a context that has rendered holds views and a derived copy,
    # and the two contexts of (a) and (b) must differ in the library alone
    row["box_ten_wm_launch_ms"] = round(this.benchmark("TEN_WM", warmup=3, runs=20).median_ms, 4)
    for ctx in ctxs.values():
        ctx.close()
    print(json.dumps(row), flush=True)
