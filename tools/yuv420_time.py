"""YUV 4:2:0 frames (lfi_download_views_yuv420, lfi_render_stream_yuv420): what the device-side conversion costs against the RGBA downloads it
replaces.  Per case and view layout, in ONE process on one context at a time (the synthetic grid, 64 views rendered with TEN_WM), medians of
`runs` timed calls after `warm` warm-ups, host clock around the synchronous calls, into page-locked host memory:
  (a) 64 lfi_download_view calls (existing code, the yardstick) against ONE lfi_download_views_yuv420 of the same 64 views;
  (b) lfi_render_stream with RGBA downloads (existing code; it needs the RGBA view layout, so the planar rows carry the RGBA layout's figure)
      against lfi_render_stream_yuv420, for a path of `path` views (default 256) in blocks of 64;
  (c) the kernel alone comes from a SECOND run of this tool under
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/yuv420_time.py 3 1 a
      and  python tools/yuv420_time.py --kernels DIR/…_kernel_trace.csv
      which prints, per grid of yuvs_convert launches (the kernel behind both calls, csrc/hip/yuv_surfaces.hpp; in the tool's order: per
      case, rgba then planar), the number of launches, the median of End_Timestamp − Start_Timestamp (device clock), the bytes the kernel
      moves (4 read per pixel from RGBA views, 3 from planar ones, 1.5 written) and the rate as a fraction of 8 TB/s.
Before anything is timed the frames of (a) are held against the numpy restatement of the definition on view 0 and the last view.
Reads nothing but the package and tests/yuv_ref.py.
usage: python tools/yuv420_time.py [runs=20] [warm=3] [rows=ab] [path=256] [case ...]   cases: 1080p, 4k (default: both)"""
import csv
import ctypes
import json
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np

PEAK_BYTES_PER_S = 8e12   # HBM3E, specification
V = 64

CASES = {
    # name: cols, rows, W, H, trajectory, focus, aspect
    "1080p": (8, 8, 1920, 1080, "0.0,0.0,1.0,1.0", 0.23, 1.783),
    "4k": (15, 15, 3840, 2160, "0,0.5,1,0.5", 0.06, 2.276),
}

if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
    with open(sys.argv[2], newline="") as f:
        trace = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    groups = {}
    for r in trace:
        name = r["Kernel_Name"].split("(")[0]
        if "yuvs_convert" not in name:
            continue
        grid = (int(r.get("Grid_Size_X", r.get("Grid_Size", 0))), int(r.get("Grid_Size_Y", 0) or 0), int(r.get("Grid_Size_Z", 0) or 0))
        groups.setdefault((name, grid), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    for (name, grid), ms in groups.items():
        row = {"kernel": name, "grid_threads": "x".join(map(str, grid)), "launches": len(ms), "median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4),
               "max_ms": round(max(ms), 4)}
        # grid = (64·⌈W/512⌉, 4·⌈H/8⌉, views) threads: the case is the one whose sizes give it
        for case, (_, _, W, H, _, _, _) in CASES.items():
            if grid in ((64 * -(-W // 512), 4 * -(-H // 8), V), (-(-W // 512), -(-H // 8), V)):   # in threads, or in workgroups
                planar = "ILb1E" in name or "<true" in name
                moved = V * W * H * ((3 if planar else 4) + 1.5)
                row.update(case=case, layout="planar" if planar else "rgba", bytes=int(moved), us_at_8TBs=round(moved / PEAK_BYTES_PER_S * 1e6, 1),
                           fraction_of_8TBs=round(moved / (float(np.median(ms)) * 1e-3) / PEAK_BYTES_PER_S, 4))
        print(json.dumps(row), flush=True)
    sys.exit(0)

import lfinterpolator_amd as L
import yuv_ref as ref

args = sys.argv[1:]
runs = int(args[0]) if args else 20
warm = int(args[1]) if len(args) > 1 else 3
rows_wanted = args[2] if len(args) > 2 else "ab"
path = int(args[3]) if len(args) > 3 else 256
names = args[4:] or list(CASES)


def timed(fn):
    """(median host wall ms, all wall ms) of the synchronous call fn"""
    for _ in range(warm):
        fn()
    wall = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(wall)), 4), [round(x, 3) for x in wall]


for name in names:
    cols, rows, W, H, traj, f, aspect = CASES[name]
    hp = L.build_params(cols, rows, W, H, traj, f, 0.0, 3.0, aspect, V)
    hp_path = L.build_params(cols, rows, W, H, traj, f, 0.0, 3.0, aspect, path)
    rgba_stream_ms = None
    for layout in ("rgba", "planar"):
        with L.Context(0) as ctx:
            ctx.set_grid(cols, rows, W, H)
            ctx.fill_synthetic(0x1F1F)
            ctx.set_params(hp)
            ctx.set_output_layout(layout)
            ctx.render("TEN_WM")
            ctx.sync()
            fb = ctx.yuv420_frame_bytes()
            row = {"case": name, "grid": f"{cols}x{rows}", "res": f"{W}x{H}", "views": V, "layout": layout, "runs": runs, "warm": warm, "rows": rows_wanted,
                   "rgba_bytes": V * W * H * 4, "yuv_bytes": V * fb}
            frames = ctx.pinned_empty((V, fb))
            view = ctx.pinned_empty((V, H, W, 4))
            ctx.download_views_yuv420(out=frames)
            for v in (0, V - 1):
                assert (frames[v] == ref.frame(ctx.download_view(v), ref.BT709, ref.LIMITED)).all(), (name, layout, v)
            if "a" in rows_wanted:
                row["a_rgba_64_calls_ms"], row["reps_a_rgba"] = timed(lambda: ctx.download_views(out=view))
                row["a_yuv_one_call_ms"], row["reps_a_yuv"] = timed(lambda: ctx.download_views_yuv420(out=frames))
                row["a_yuv_over_rgba"] = round(row["a_yuv_one_call_ms"] / row["a_rgba_64_calls_ms"], 4)
                if name == "4k":
                    row["condition_yuv_below_rgba"] = bool(row["a_yuv_one_call_ms"] < row["a_rgba_64_calls_ms"])
            if "b" in rows_wanted:
                row["path_views"] = path
                if layout == "rgba":
                    out = ctx.pinned_empty((path, H, W, 4))
                    rgba_stream_ms, row["reps_b_rgba"] = timed(lambda: ctx.render_stream("TEN_WM", hp_path.weights, out))
                    del out
                    ctx._lib.lfi_free_pinned(ctypes.c_void_p(ctx._pinned.pop()))   # the largest buffer goes before the next is made
                row["b_rgba_stream_ms"] = rgba_stream_ms            # of the RGBA layout: lfi_render_stream's downloads refuse the planar one
                out = ctx.pinned_empty((path, fb))
                row["b_yuv_stream_ms"], row["reps_b_yuv"] = timed(lambda: ctx.render_stream_yuv420("TEN_WM", hp_path.weights, out=out))
                row["b_yuv_over_rgba"] = round(row["b_yuv_stream_ms"] / rgba_stream_ms, 4)
            row["workspace_bytes"] = int(ctx.memory_info().workspace_bytes)
        print(json.dumps(row), flush=True)
