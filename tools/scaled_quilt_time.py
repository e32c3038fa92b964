"""Scaled quilts (lfi_download_quilt_scaled): what a 5 x 9 quilt costs with the views resized on the device, against the unscaled quilt.
Per case, in ONE process on one context (the synthetic grid, a TEN_WM render, 45 views, the RGBA view layout), medians of `runs` timed calls after
`warm` warm-ups, into host arrays allocated before the timing:
  (a) lfi_download_quilt 5 x 9 (through lfi_download_quilt_tiles with all 45 tiles: the same code path), whole call, host clock;
  (c) lfi_download_quilt_scaled 5 x 9 at half size per axis and at the tile size of an 8192 x 8192 quilt from 4K views (1638 x 910; from 1080p
      views the 4096 x 4096 quilt's 819 x 455), whole call, host clock;
and beside each the HIP-event time of the whole call (kernel + copies).  The calls are synchronous and give the caller no event between the kernel and
the copy, so the kernels' own times,
  (b) quilt_assemble and (d) quilt_scale,
come from a SECOND run of this tool under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/scaled_quilt_time.py …` and
  python tools/scaled_quilt_time.py --kernels DIR/…_kernel_trace.csv
which prints, per kernel name and grid, the number of launches and the median of End_Timestamp − Start_Timestamp (device clock).
Row (a) needs nothing of the scaled calls and also runs on a build without them ("rows" = a), e.g. the parent commit's, for a comparison on one box in
one session.  Reads nothing but the package.
usage: python tools/scaled_quilt_time.py [runs=20] [warm=3] [rows=ac] [case ...]   cases: 1080p, 4k (default: both)"""
import csv
import json
import sys
import time

sys.path.insert(0, ".")
import numpy as np

if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
    groups = {}
    with open(sys.argv[2], newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if "quilt_" not in name:
                continue
            key = (name.split("(")[0], r.get("Grid_Size_X", r.get("Grid_Size", "")), r.get("Grid_Size_Y", ""), r.get("Grid_Size_Z", ""))
            groups.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    for key, ms in sorted(groups.items()):
        print(json.dumps({"kernel": key[0], "grid": "x".join(key[1:]), "launches": len(ms), "median_ms": round(float(np.median(ms)), 4),
                          "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}), flush=True)
    sys.exit(0)

import lfinterpolator_amd as L

CASES = {
    # name: cols, rows, W, H, trajectory, focus, aspect, views, the 8192^2 (4K) / 4096^2 (1080p) quilt's tile
    "1080p": (15, 15, 1920, 1080, "0,0.5,1,0.5", 0.06, 2.276, 45, (819, 455)),     # BASELINE config 3's shape
    "4k": (8, 8, 3840, 2160, "0.0,0.0,1.0,1.0", 0.23, 1.783, 45, (1638, 910)),
}
TX, TY = 5, 9
args = sys.argv[1:]
runs = int(args[0]) if args else 20
warm = int(args[1]) if len(args) > 1 else 3
rows_wanted = args[2] if len(args) > 2 else "ac"
names = args[3:] or list(CASES)


def timed(ctx, fn):
    """(median host wall ms, median event ms, all wall ms) of the synchronous call fn"""
    for _ in range(warm):
        fn()
    ev, wall = [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        ctx.timer_start()
        fn()
        ev.append(ctx.timer_stop())
        wall.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(wall)), 4), round(float(np.median(ev)), 4), [round(x, 3) for x in wall]


for name in names:
    cols, rows, W, H, traj, f, aspect, V, lkg_tile = CASES[name]
    hp = L.build_params(cols, rows, W, H, traj, f, 0.0, 3.0, aspect, V)
    with L.Context(0) as ctx:
        ctx.set_grid(cols, rows, W, H)
        ctx.fill_synthetic(0x1F1F)
        ctx.set_params(hp)
        ctx.render("TEN_WM")
        ctx.sync()
        row = {"case": name, "grid": f"{cols}x{rows}", "res": f"{W}x{H}", "views": V, "quilt": f"{TX}x{TY}", "runs": runs, "warm": warm, "rows": rows_wanted}
        row["box_ten_wm_launch_ms"] = round(ctx.benchmark("TEN_WM", warmup=3, runs=20).median_ms, 4)
        if "a" in rows_wanted:
            out = np.empty((TY * H, TX * W, 4), np.uint8)
            out.fill(0xC3)   # touched before the timing: no page faults inside it
            row["a_unscaled_wall_ms"], row["a_unscaled_event_ms"], row["reps_a"] = timed(ctx, lambda: ctx.download_quilt_tiles(out, TX, TY, 0, TX * TY))
            row["a_bytes"] = int(out.nbytes)
            del out
        if "c" in rows_wanted:
            for label, (tw, th) in (("half", (W // 2, H // 2)), ("lkg", lkg_tile)):
                out = np.empty((TY * th, TX * tw, 4), np.uint8)
                out.fill(0xC3)
                wall, ev, reps = timed(ctx, lambda: ctx.download_quilt_scaled(TX, TY, tw, th, out=out))
                row[f"c_{label}_tile"], row[f"c_{label}_wall_ms"], row[f"c_{label}_event_ms"], row[f"reps_c_{label}"] = f"{tw}x{th}", wall, ev, reps
                row[f"c_{label}_bytes"] = int(out.nbytes)
                if "a" in rows_wanted:
                    row[f"c_{label}_over_a"] = round(wall / row["a_unscaled_wall_ms"], 4)
                del out
    print(json.dumps(row), flush=True)
