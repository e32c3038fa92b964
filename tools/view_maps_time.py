"""Per-view focus maps (lfi_view_focus_maps): what a view-centred all-focus render with every view's own map costs, against the loop it
replaces.  Per case, HIP events around the GPU work, median of `reps` repetitions after a warm-up:
  (a) lfi_view_focus_maps for all V views (estimate + filter), and the padded planes: `padded_first` when the workspace starts empty,
      `padded_next` for a repeated call (its first view finds the last view's planes), against V x n_ids for a loop over lfi_focus_map —
      counted by the slot rule of lfi_view_focus_maps (pad_slot_order), replayed here on the same ids;
  (b) the all-focus render over the per-view maps, STD and TEN_WM (blend_vfocus_af's view_maps variant);
  (c) the alternative without this call: V x (lfi_set_params with O[v], ids_v and weight row v, lfi_focus_map, a one-view all-focus render);
  (d) lfi_focus_map's steady state at the same shape (one map at the trajectory's centre), for comparison with (a) / V.
Also checks that (c) and (a)+(b) give the same maps and STD bytes for the first and the last view.
usage: python tools/view_maps_time.py [reps=5] [--ab] [case ...]   cases: 8x8, 4k (default: both); --ab: (a) and (b) only (for a kernel trace)"""
import json
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
only_ab = "--ab" in args
args = [a for a in args if a != "--ab"]
reps = int(args[0]) if args else 5
names = args[1:] or list(CASES)


def median_ms(ctx, fn, warm=True):
    if warm:
        fn()
        ctx.sync()
    t = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        t.append(ctx.timer_stop())
    return round(float(np.median(t)), 4), [round(x, 4) for x in t]


def padded(ids, slots):
    """planes lfi_view_focus_maps pads for ids [V][n] when the planes hold `slots` (None: nothing padded yet)"""
    count = 0
    for row in ids:
        row = [int(g) for g in row]
        if slots is None or len(slots) != len(row):
            count += len(row)
            slots = list(row)
            continue
        keep = [s if s in row else None for s in slots]
        rest = [g for g in row if g not in keep]
        count += len(rest)
        slots = [s if s is not None else rest.pop(0) for s in keep]
    return count, slots


for name in names:
    cols, rows, W, H, traj, f, r, V = CASES[name]
    hp = L.build_params(cols, rows, W, H, traj, f, r, 3.0, 1.0, V)
    O, _ = L.build_view_centred_offsets(cols, rows, W, H, traj, 1.0, np.full(V, f, np.float32))
    ids = L.build_view_focus_ids(cols, rows, traj, V)
    n_first, last = padded(ids, None)
    n_next, _ = padded(ids, last)
    ctx = L.Context(0)
    ctx.set_grid(cols, rows, W, H)
    ctx.fill_synthetic(0x1F1F)
    ctx.set_params(hp)
    ctx.set_view_float_offsets(O)
    t_est, all_est = median_ms(ctx, lambda: ctx.view_focus_maps(ids))
    row = {"case": name, "grid": f"{cols}x{rows}", "res": f"{W}x{H}", "views": V, "focus": f, "range": r, "n_ids": int(ids.shape[1]),
           "a_view_focus_maps_ms": t_est, "a_per_view_ms": round(t_est / V, 4), "padded_first": n_first, "padded_next": n_next,
           "padded_loop": V * int(ids.shape[1]), "reps_a": all_est}
    views = {}
    for method in ("STD", "TEN_WM"):
        ctx.prepare(method, all_focus=True)
        t_r, all_r = median_ms(ctx, lambda: ctx.render(method, all_focus=True))
        row[f"b_render_{method}_ms"] = t_r
        row[f"b_kernel_{method}"] = ctx.last_kernel_name()
        row[f"reps_b_{method}"] = all_r
        ctx.render(method, all_focus=True)
        ctx.sync()
        views[method] = {v: ctx.download_view(v) for v in (0, V - 1)}
    maps = {v: (ctx.download_view_map(v, 0), ctx.download_view_map(v, 1)) for v in (0, V - 1)}
    ctx.close()
    if only_ab:
        print(json.dumps(row), flush=True)
        continue

    hp_v = [L.HostParams(hp.focused_offsets, np.ascontiguousarray(O[v]), np.ascontiguousarray(hp.weights[v:v + 1]),
                         np.ascontiguousarray(ids[v]), f, r, hp.block_radius) for v in range(V)]
    loop = L.Context(0)
    loop.set_grid(cols, rows, W, H)
    loop.fill_synthetic(0x1F1F)
    loop.set_params(hp_v[0])
    same = True
    for method in ("STD", "TEN_WM"):
        def run_loop():
            for v in range(V):
                loop.set_params(hp_v[v])
                loop.focus_map()
                loop.render(method, all_focus=True)
        t_l, all_l = median_ms(loop, run_loop)
        row[f"c_loop_{method}_ms"] = t_l
        row[f"c_kernel_{method}"] = loop.last_kernel_name()
        row[f"reps_c_{method}"] = all_l
        row[f"speedup_{method}"] = round(t_l / (t_est + row[f"b_render_{method}_ms"]), 2)
    for v in (0, V - 1):
        loop.set_params(hp_v[v])
        loop.focus_map()
        loop.render("STD", all_focus=True)
        loop.sync()
        same &= bool((loop.download_map(0) == maps[v][0]).all() and (loop.download_map(1) == maps[v][1]).all())
        same &= bool((loop.download_view(0) == views["STD"][v]).all())
    row["loop_maps_and_std_bytes_equal"] = same
    loop.close()

    centre = L.Context(0)
    centre.set_grid(cols, rows, W, H)
    centre.fill_synthetic(0x1F1F)
    centre.set_params(hp)
    row["d_focus_map_ms"], row["reps_d"] = median_ms(centre, centre.focus_map)
    centre.close()
    print(json.dumps(row), flush=True)
