"""View-centred all-focus renders (lfi_set_view_float_offsets): one launch of V views, each shifted about its own camera, against the loop
it replaces — V × (lfi_set_params with offsets = O[v] and weight row v + a one-view all-focus render over the same map).  HIP events around
the GPU work of both (the loop's host-side staging included, as a caller pays it); median of `reps` repetitions after a warm-up.  Both read
the same maps: --map own (default) the focus map lfi_focus_map estimates at the trajectory's centre on the synthetic light field, --map random
uniformly random focus bytes (every pixel's samples land on unrelated cache lines: the worst case for any gather).  Also checks that the two
give the same STD bytes for the first and the last view (the loop's kernels are bit-exact too).
usage: python tools/view_centre_time.py [reps=5] [--map own|random] [case ...]   cases: 8x8, 4k (default: both)"""
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
map_kind = "own"
if "--map" in args:
    i = args.index("--map")
    map_kind = args[i + 1]
    del args[i:i + 2]
reps = int(args[0]) if args else 5
names = args[1:] or list(CASES)


def median_ms(ctx, fn):
    fn()  # warm-up (first-touch allocations)
    ctx.sync()
    t = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        t.append(ctx.timer_stop())
    return float(np.median(t)), t


def context(cols, rows, W, H, hp, maps):
    ctx = L.Context(0)
    ctx.set_grid(cols, rows, W, H)
    ctx.fill_synthetic(0x1F1F)
    ctx.set_params(hp)
    for k in (0, 1):
        ctx.upload_map(k, maps[k])
    return ctx


for name in names:
    cols, rows, W, H, traj, f, r, V = CASES[name]
    hp = L.build_params(cols, rows, W, H, traj, f, r, 3.0, 1.0, V)
    O, _ = L.build_view_centred_offsets(cols, rows, W, H, traj, 1.0, np.full(V, f, np.float32))
    hp_v = [L.HostParams(hp.focused_offsets, O[v], np.ascontiguousarray(hp.weights[v:v + 1]), hp.focus_map_ids, f, r, hp.block_radius)
            for v in range(V)]
    if map_kind == "random":
        m = np.zeros((H, W, 4), np.uint8)
        m[..., 0] = np.random.default_rng(1).integers(0, 256, (H, W), dtype=np.uint8)
        m[..., 3] = 255
        maps = [m, m]
    else:
        with L.Context(0) as est:
            est.set_grid(cols, rows, W, H)
            est.fill_synthetic(0x1F1F)
            est.set_params(hp)
            est.focus_map()
            est.sync()
            maps = [est.download_map(0), est.download_map(1)]
    for method in ("STD", "TEN_WM"):
        one = context(cols, rows, W, H, hp, maps)
        one.set_view_float_offsets(O)
        one.prepare(method, all_focus=True)
        t_one, all_one = median_ms(one, lambda: one.render(method, all_focus=True))
        kernel = one.last_kernel_name()
        loop = context(cols, rows, W, H, hp_v[0], maps)

        def run_loop():
            for v in range(V):
                loop.set_params(hp_v[v])
                loop.render(method, all_focus=True)
        t_loop, all_loop = median_ms(loop, run_loop)
        same = None
        if method == "STD":
            same = True
            for v in (0, V - 1):
                loop.set_params(hp_v[v])
                loop.render(method, all_focus=True)
                loop.sync()
                same &= bool((loop.download_view(0) == one.download_view(v)).all())
        print(json.dumps({"case": name, "method": method, "grid": f"{cols}x{rows}", "res": f"{W}x{H}", "views": V, "focus": f, "range": r, "map": map_kind,
                          "one_launch_ms": round(t_one, 4), "loop_ms": round(t_loop, 4), "speedup": round(t_loop / t_one, 2),
                          "one_launch_kernel": kernel, "loop_kernel": loop.last_kernel_name(), "std_bytes_equal": same,
                          "reps_one": [round(x, 4) for x in all_one], "reps_loop": [round(x, 4) for x in all_loop]}), flush=True)
        one.close()
        loop.close()
