"""Focus tiles (lfi_focus_tiles): what all tiles' focus curves cost, against the focus map whose estimate they share and against the
per-region call they replace.  Per case (the shapes and the scene of tools/focus_curve_time.py: BASELINE configs 2 and 5, the structured scene
of lfi_fill_synthetic_scene, 32 sampled images), in ONE process on one context, HIP events around the GPU work and the host's wall clock around
the call, medians of `runs` timed runs after `warm` warm-ups:
  (a) lfi_focus_map, default variant ("factored");
  (b) lfi_focus_curve, whole frame, 32 steps;
  (c) 144 calls of lfi_focus_curve over the rectangles of a 16 x 9 grid, host wall time;
  (d) lfi_focus_tiles(1, 1);
  (e) lfi_focus_tiles(16, 9) — the bar is (d) and (e) <= 1.25 x (a) in event time; (b) / (d) and (c) / (e) are records.
The events of (b), (d), (e) include the call's device-to-host copy (the calls are synchronous).  Rows (a)-(c) need nothing of lfi_focus_tiles
and also run on a build without it ("rows" = abc), e.g. the parent commit's, for a comparison on one box in one session.
usage: python tools/focus_tiles_time.py [runs=20] [warm=3] [rows=abcde] [case ...]   cases: 8x8, 4k (default: both)"""
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
rows_wanted = args[2] if len(args) > 2 else "abcde"
names = args[3:] or list(CASES)
TILES = (16, 9)


def tile_rect(W, H, nx, ny, tx, ty):
    return tx * W // nx, ty * H // ny, (tx + 1) * W // nx, (ty + 1) * H // ny


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
               "warm": warm, "rows": rows_wanted, "tiles": f"{TILES[0]}x{TILES[1]}"}
        # the headline launch time of this box (config-2-like TEN_WM launch of the case's own shape), as the other notes record it
        row["box_ten_wm_launch_ms"] = round(ctx.benchmark("TEN_WM", warmup=3, runs=20).median_ms, 4)
        rects = [tile_rect(W, H, *TILES, tx, ty) for ty in range(TILES[1]) for tx in range(TILES[0])]
        if "a" in rows_wanted:
            row["a_map_factored_ms"], row["a_wall_ms"], row["reps_a"] = timed(ctx, ctx.focus_map)
        if "b" in rows_wanted:
            row["b_curve_whole_ms"], row["b_wall_ms"], row["reps_b"] = timed(ctx, lambda: ctx.focus_curve(0, 0, W, H, 32))
        if "c" in rows_wanted:
            def curve_per_tile():
                for rect in rects:
                    ctx.focus_curve(*rect, 32)
            row["c_144_curves_ms"], row["c_wall_ms"], row["reps_c"] = timed(ctx, curve_per_tile)
        if "d" in rows_wanted:
            row["d_tiles_1x1_ms"], row["d_wall_ms"], row["reps_d"] = timed(ctx, lambda: ctx.focus_tiles(1, 1))
        if "e" in rows_wanted:
            row["e_tiles_16x9_ms"], row["e_wall_ms"], row["reps_e"] = timed(ctx, lambda: ctx.focus_tiles(*TILES))
            cost, best, bf = ctx.focus_tiles(*TILES)
            row["e_best_index_min_max"] = [int(best.min()), int(best.max())]
        if "a" in rows_wanted and "d" in rows_wanted:
            row["d_over_a"] = round(row["d_tiles_1x1_ms"] / row["a_map_factored_ms"], 4)
        if "a" in rows_wanted and "e" in rows_wanted:
            row["e_over_a"] = round(row["e_tiles_16x9_ms"] / row["a_map_factored_ms"], 4)
        if "b" in rows_wanted and "d" in rows_wanted:
            row["b_over_d"] = round(row["b_curve_whole_ms"] / row["d_tiles_1x1_ms"], 2)
        if "c" in rows_wanted and "e" in rows_wanted:
            row["c_wall_over_e_wall"] = round(row["c_wall_ms"] / row["e_wall_ms"], 2)
        row["workspace_bytes"] = int(ctx.memory_info().workspace_bytes)
    print(json.dumps(row), flush=True)
