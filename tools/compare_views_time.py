"""Batch view comparison (lfi_compare_views): what comparing 64 views costs, against the one-view-per-call loop it replaces.
Per case and view layout, in ONE process on one context (the synthetic grid; STD rendered and kept with lfi_keep_views, then TEN_WM rendered: the
views compared are TEN_WM's, the references STD's), medians of `runs` timed calls after `warm` warm-ups, host clock around the synchronous call
(the HIP-event time of the whole call beside it):
  (a) lfi_compare_views against the kept views — nothing but the results crosses PCIe.  Also as a rate on the bytes of the views and their
      references, 2 · n · view bytes as stored on the device, and that rate as a fraction of 8 TB/s;
  (b) lfi_compare_views against page-locked host references (the STD views downloaded into lfi_alloc_pinned memory) — bounded by PCIe;
  (c) what a user has without the batch call: n lfi_compare_view calls on the same page-locked references.
The three must agree byte for byte ((c) runs the batch call's code for one view) — checked before anything is timed.
The kernels' own times come from a SECOND run of this tool under
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/compare_views_time.py …
and  python tools/compare_views_time.py --kernels DIR/…_kernel_trace.csv
which prints, per kernel name and grid, the number of launches and the median of End_Timestamp − Start_Timestamp (device clock).
Reads nothing but the package.
usage: python tools/compare_views_time.py [runs=10] [warm=2] [rows=abc] [case ...]   cases: 1080p, 4k (default: both)"""
import csv
import ctypes
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
            if "quality_" not in name:
                continue
            key = (name.split("(")[0], r.get("Grid_Size_X", r.get("Grid_Size", "")), r.get("Grid_Size_Y", ""), r.get("Grid_Size_Z", ""))
            groups.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    for key, ms in sorted(groups.items()):
        print(json.dumps({"kernel": key[0], "grid": "x".join(key[1:]), "launches": len(ms), "median_ms": round(float(np.median(ms)), 4),
                          "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}), flush=True)
    sys.exit(0)

import lfinterpolator_amd as L

CASES = {
    # name: cols, rows, W, H, trajectory, focus, aspect, views
    "1080p": (8, 8, 1920, 1080, "0.0,0.0,1.0,1.0", 0.23, 1.783, 64),
    "4k": (15, 15, 3840, 2160, "0,0.5,1,0.5", 0.06, 2.276, 64),
}
PEAK_BYTES_PER_S = 8e12   # HBM3E, specification
args = sys.argv[1:]
runs = int(args[0]) if args else 10
warm = int(args[1]) if len(args) > 1 else 2
rows_wanted = args[2] if len(args) > 2 else "abc"
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


def raw(recs, n):
    return ctypes.string_at(recs, ctypes.sizeof(L.ViewQuality) * n)


for name in names:
    cols, rows, W, H, traj, f, aspect, V = CASES[name]
    hp = L.build_params(cols, rows, W, H, traj, f, 0.0, 3.0, aspect, V)
    for layout in ("rgba", "planar"):
        with L.Context(0) as ctx:
            ctx.set_grid(cols, rows, W, H)
            ctx.fill_synthetic(0x1F1F)
            ctx.set_params(hp)
            ctx.set_output_layout(layout)
            ctx.render("STD")
            ctx.keep_views()
            refs = ctx.pinned_empty((V, H, W, 4))
            ctx.download_views(out=refs)
            ctx.render("TEN_WM")
            ctx.sync()
            view_bytes = int(ctx.view_layout().view_stride_bytes)
            row = {"case": name, "grid": f"{cols}x{rows}", "res": f"{W}x{H}", "views": V, "layout": layout, "runs": runs, "warm": warm, "rows": rows_wanted,
                   "view_bytes": view_bytes, "bytes_2n_views": 2 * V * view_bytes, "reference_bytes_host": int(refs.nbytes)}
            # the three ways agree
            kept, kept_all = ctx.compare_views()
            host, _ = ctx.compare_views(refs)
            assert raw(kept, V) == raw(host, V), "kept and host references disagree"
            for v in (0, V // 2, V - 1):
                one = ctx.compare_view(v, refs[v])
                assert bytes(one) == bytes(kept[v].q), v
            row["psnr_all"], row["ssim_all"] = round(kept_all.psnr_all, 4), round(kept_all.ssim_all, 6)
            row["max_abs_diff"] = max(r.max_abs_diff for r in kept)
            row["differing_fraction"] = round(sum(r.differing_bytes for r in kept) / (3.0 * V * W * H), 5)
            if "a" in rows_wanted:
                row["a_kept_wall_ms"], row["a_kept_event_ms"], row["reps_a"] = timed(ctx, lambda: ctx.compare_views())
                rate = row["bytes_2n_views"] / (row["a_kept_wall_ms"] * 1e-3)
                row["a_kept_TB_per_s"], row["a_kept_fraction_of_8TBs"] = round(rate / 1e12, 3), round(rate / PEAK_BYTES_PER_S, 3)
            if "b" in rows_wanted:
                row["b_pinned_wall_ms"], row["b_pinned_event_ms"], row["reps_b"] = timed(ctx, lambda: ctx.compare_views(refs))
                row["b_pinned_GB_per_s"] = round(refs.nbytes / (row["b_pinned_wall_ms"] * 1e-3) / 1e9, 2)

            def loop():
                for v in range(V):
                    ctx.compare_view(v, refs[v])

            if "c" in rows_wanted:
                row["c_loop_wall_ms"], row["c_loop_event_ms"], row["reps_c"] = timed(ctx, loop)
                for k in ("a_kept", "b_pinned"):
                    if f"{k}_wall_ms" in row:
                        row[f"{k}_over_c"] = round(row[f"{k}_wall_ms"] / row["c_loop_wall_ms"], 4)
        print(json.dumps(row), flush=True)
