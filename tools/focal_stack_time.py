"""Per-view focus (lfi_set_view_offsets): one launch of a focal stack / focus pull against the loop it replaces — V × (lfi_set_params with
view v's offsets and weight row + a one-view render), each launch reading the whole grid.  HIP events around the GPU work of both (the
loop's host-side staging included, as a caller pays it); median of `reps` repetitions after a warm-up.  Also checks that the two give the
same bytes for STD (the loop's kernels are bit-exact too).
usage: python tools/focal_stack_time.py [reps=5] [case ...]   cases: wide, narrow, 4k (default: all three)"""
import json
import sys

sys.path.insert(0, ".")
import numpy as np

import lfinterpolator_amd as L

CASES = {
    # name: cols, rows, W, H, trajectory, focus from, focus to, views
    "wide": (8, 8, 1920, 1080, "0.5,0.5,0.5,0.5", 0.0, 0.5, 64),
    "narrow": (8, 8, 1920, 1080, "0.5,0.5,0.5,0.5", 0.20, 0.25, 64),
    "4k": (15, 15, 3840, 2160, "0.5,0.5,0.5,0.5", 0.22, 0.39, 32),
}
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
names = sys.argv[2:] or list(CASES)


def median_ms(ctx, fn):
    fn()  # warm-up (builds the planar copy, first-touch allocations)
    ctx.sync()
    t = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        t.append(ctx.timer_stop())
    return float(np.median(t)), t


for name in names:
    cols, rows, W, H, traj, f0, f1, V = CASES[name]
    focus = L.focus_ramp(f0, f1, V)
    hp = L.build_params(cols, rows, W, H, traj, float(focus[0]), 0.0, 3.0, 1.0, V)
    D = L.build_view_offsets(cols, rows, W, H, traj, 1.0, focus)
    hp_v = [L.HostParams(D[v], hp.offsets, np.ascontiguousarray(hp.weights[v:v + 1]), hp.focus_map_ids, float(focus[v]), 0.0, hp.block_radius)
            for v in range(V)]
    for method in ("STD", "TEN_WM"):
        one = L.Context(0)
        one.set_grid(cols, rows, W, H)
        one.fill_synthetic(0x1F1F)
        one.set_params(hp)
        one.set_view_offsets(D)
        one.prepare(method)
        t_one, all_one = median_ms(one, lambda: one.render(method))
        kernel = one.last_kernel_name()
        loop = L.Context(0)
        loop.set_grid(cols, rows, W, H)
        loop.fill_synthetic(0x1F1F)
        loop.set_params(hp_v[0])

        def run_loop():
            for v in range(V):
                loop.set_params(hp_v[v])
                loop.render(method)
        t_loop, all_loop = median_ms(loop, run_loop)
        same = None
        if method == "STD":  # spot-check: views 0 and V-1 of the one launch against the loop's renders
            same = True
            for v in (0, V - 1):
                loop.set_params(hp_v[v])
                loop.render(method)
                loop.sync()
                same &= bool((loop.download_view(0) == one.download_view(v)).all())
        print(json.dumps({"case": name, "method": method, "grid": f"{cols}x{rows}", "res": f"{W}x{H}", "views": V, "focus": [f0, f1],
                          "one_launch_ms": round(t_one, 4), "loop_ms": round(t_loop, 4), "speedup": round(t_loop / t_one, 2),
                          "one_launch_kernel": kernel, "loop_kernel": loop.last_kernel_name(), "std_bytes_equal": same,
                          "reps_one": [round(x, 4) for x in all_one], "reps_loop": [round(x, 4) for x in all_loop]}), flush=True)
        one.close()
        loop.close()
