"""Autofocus (lfi_focus_curve): what the focus curve costs, against the focus map it shares its sampling with.  Per case (BASELINE configs 2
and 5 shapes, the structured scene of lfi_fill_synthetic_scene, 32 sampled images), in ONE process on one context, HIP events around the GPU
work, `runs` timed runs after `warm` warm-ups:
  (a) lfi_focus_curve, whole frame, 32 steps;
  (b) lfi_focus_map with the estimate variant "packed_p2" (focus_estimate_packed<2, 4>: the kernel the curve shares its sampling with) — the bar
      is (a) <= 1.10 x (b);
  (c) lfi_focus_map with the default variant ("factored"): what reusing its range pass for whole-frame curves would be worth — a record;
  (d) lfi_focus_curve on a 256 x 256 region, 32 steps (click-to-focus): event time and the call's host wall time, against
  (e) lfi_focus_map (default) + lfi_download_map(0) of the same context, host wall time — the bar is (d) < (e).
The events of (a) and (d) include the call's device-to-host copy of steps * 8 + 16 bytes (the call is synchronous).
usage: python tools/focus_curve_time.py [runs=20] [warm=3] [case ...]   cases: 8x8, 4k (default: both)"""
import json
import sys
import time

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
names = args[2:] or list(CASES)


def timed(ctx, fn):
    """(median event ms, median host wall ms, all event ms) of fn, which may or may not synchronise itself"""
    for _ in range(warm):
        fn()
        ctx.sync()
    ev, wall = [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        ctx.timer_start()
        fn()
        ev.append(ctx.timer_stop())
        wall.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ev)), 4), round(float(np.median(wall)), 4), [round(x, 4) for x in ev]


for name in names:
    cols, rows, W, H, traj, f, r, V = CASES[name]
    hp = L.build_params(cols, rows, W, H, traj, f, r, 3.0, 1.0, V)
    with L.Context(0) as ctx:
        ctx.set_grid(cols, rows, W, H)
        ctx.set_params(hp)
        ctx.fill_synthetic_scene(0x1F1F)
        ctx.sync()
        row = {"case": name, "grid": f"{cols}x{rows}", "res": f"{W}x{H}", "focus": f, "range": r, "n_ids": int(len(hp.focus_map_ids)), "runs": runs,
               "warm": warm}
        # the headline launch time of this box (config-2-like TEN_WM launch of the case's own shape), as the other notes record it
        row["box_ten_wm_launch_ms"] = round(ctx.benchmark("TEN_WM", warmup=3, runs=20).median_ms, 4)
        row["a_curve_whole_ms"], row["a_wall_ms"], row["reps_a"] = timed(ctx, lambda: ctx.focus_curve(0, 0, W, H, 32))
        cost, best, bf = ctx.focus_curve(0, 0, W, H, 32)
        row["a_best_index"], row["a_best_focus"] = best, float(bf)
        ctx.set_variant("FOCUS", "packed_p2")
        row["b_map_packed_p2_ms"], _, row["reps_b"] = timed(ctx, ctx.focus_map)
        ctx.set_variant("FOCUS", "auto")
        row["c_map_factored_ms"], _, row["reps_c"] = timed(ctx, ctx.focus_map)
        row["a_over_b"] = round(row["a_curve_whole_ms"] / row["b_map_packed_p2_ms"], 4)
        row["bar_a_le_1p10_b"] = bool(row["a_over_b"] <= 1.10)
        x0, y0 = (W - 256) // 2, (H - 256) // 2
        row["d_curve_256_ms"], row["d_wall_ms"], row["reps_d"] = timed(ctx, lambda: ctx.focus_curve(x0, y0, x0 + 256, y0 + 256, 32))

        def map_and_download():
            ctx.focus_map()
            ctx.download_map(0)
        row["e_map_download_ms"], row["e_wall_ms"], row["reps_e"] = timed(ctx, map_and_download)
        row["bar_d_lt_e_wall"] = bool(row["d_wall_ms"] < row["e_wall_ms"])
        row["workspace_bytes"] = int(ctx.memory_info().workspace_bytes)
    print(json.dumps(row), flush=True)
