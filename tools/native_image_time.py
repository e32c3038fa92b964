"""Native lenticular images (lfi_download_native): what the display-sized picture costs against the scaled quilt a host-side interlace would start from.
Per case and view layout, in ONE process on one context at a time (the synthetic grid, 45 views rendered with TEN_WM), medians of `runs` timed
calls after `warm` warm-ups, host clock around the synchronous call (the HIP-event time of the whole call beside it), into pageable host arrays
that were touched before the timing:
  (a) lfi_download_quilt_scaled 5 x 9 at tiles of 819 x 455 and 1638 x 910 — existing code, the yardstick;
  (b) lfi_download_native with the same tiles to 3840 x 2160 (quilt_scale into the device-resident tiles, native_interlace, one copy);
  (c) lfi_download_native with tile = view size (no first stage: the views read in place) to 3840 x 2160.
Each row carries the bytes its variant copies to the host, and for native_interlace the bytes the kernel must read and write at least: it
writes out_w·out_h·4; it reads, per view (and colour plane in the planar layout), the 128-byte cache lines of the source rows it touches —
(distinct sy) x (row bytes rounded up to lines) — since neighbouring subpixels of one row spread over all views.
  (d) the interlace kernel alone comes from a SECOND run of this tool under
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/native_image_time.py …
      and  python tools/native_image_time.py --kernels DIR/…_kernel_trace.csv
      which prints, per context (in the tool's order), kernel, grid and — for native_interlace — the source of its tiles, the number of
      launches and the median of End_Timestamp − Start_Timestamp (device clock).
Before anything is timed (b) and (c) are checked against each other's definition: (b)'s tiles are (a)'s, so the native image must equal the
gather of (a)'s quilt, at a sample of rows.
Reads nothing but the package.
usage: python tools/native_image_time.py [runs=10] [warm=2] [rows=abc] [case ...]   cases: 1080p, 4k (default: both)"""
import csv
import json
import sys
import time

sys.path.insert(0, ".")
import numpy as np

if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
    with open(sys.argv[2], newline="") as f:
        trace = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    # the trace in launch order: a blend kernel opens a context (the tool's order: per case, rgba then planar); a native_interlace launch is
    # labelled with the kernel in front of it — the quilt_scale grid that made its tiles, or "in place"
    groups, context, before = {}, 0, ""
    for r in trace:
        name = r["Kernel_Name"].split("(")[0]
        grid = "x".join((r.get("Grid_Size_X", r.get("Grid_Size", "")), r.get("Grid_Size_Y", ""), r.get("Grid_Size_Z", "")))
        if "blend_" in name:
            context += 1
        if "native_interlace" in name or "quilt_scale" in name:
            label = "" if "quilt_scale" in name else ("tiles of quilt_scale " + before.split(" ")[-1] if "quilt_scale" in before else "in place")
            groups.setdefault((context, name, grid, label), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
        before = name + " " + grid
    for key, ms in sorted(groups.items()):
        print(json.dumps({"context": key[0], "kernel": key[1], "grid": key[2], "source": key[3], "launches": len(ms), "median_ms": round(float(np.median(ms)), 4),
                          "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}), flush=True)
    sys.exit(0)

import lfinterpolator_amd as L

CASES = {
    # name: cols, rows, W, H, trajectory, focus, aspect
    "1080p": (8, 8, 1920, 1080, "0.0,0.0,1.0,1.0", 0.23, 1.783),
    "4k": (15, 15, 3840, 2160, "0,0.5,1,0.5", 0.06, 2.276),
}
V, TILES_X, TILES_Y = 45, 5, 9
OUT_W, OUT_H = 3840, 2160
TILES = [(819, 455), (1638, 910)]
CALIBRATION = (47.5636, -5.4392, 0.0412, 338.0, False)   # lenses per inch, slant, centre, dpi, invert: of the order of a 4K lenticular panel
PEAK_BYTES_PER_S = 8e12   # HBM3E, specification
LINE = 128
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


def nearest(dst, src):
    o = np.arange(dst, dtype=np.int64)
    return ((2 * o + 1) * src) // (2 * dst)


def kernel_bytes(tw, th, planar_in_place):
    """(bytes native_interlace must read at least, bytes it writes) for T_v of tw x th"""
    rows = len(np.unique(nearest(OUT_H, th)))
    row_lines = (-(-tw // LINE) * LINE * 3) if planar_in_place else (-(-tw * 4 // LINE) * LINE)
    return V * rows * row_lines, OUT_W * OUT_H * 4


def selection(lens, ys):
    """[len(ys)][OUT_W][3]: the view every subpixel of rows ys selects"""
    x = np.arange(OUT_W, dtype=np.uint64)[None, :, None]
    y = np.asarray(ys, dtype=np.uint64)[:, None, None]
    c = np.arange(3, dtype=np.uint64)[None, None, :]
    phase = (np.uint64(lens.phase0) + (np.uint64(3) * x + c) * np.uint64(lens.x_step) + y * np.uint64(lens.y_step)) & np.uint64(0xFFFFFFFF)
    return ((phase * np.uint64(lens.views)) >> np.uint64(32)).astype(np.int64)


lens = L.lenticular(*CALIBRATION, OUT_W, OUT_H, V)
for name in names:
    cols, rows, W, H, traj, f, aspect = CASES[name]
    hp = L.build_params(cols, rows, W, H, traj, f, 0.0, 3.0, aspect, V)
    for layout in ("rgba", "planar"):
        with L.Context(0) as ctx:
            ctx.set_grid(cols, rows, W, H)
            ctx.fill_synthetic(0x1F1F)
            ctx.set_params(hp)
            ctx.set_output_layout(layout)
            ctx.render("TEN_WM")
            ctx.sync()
            row = {"case": name, "grid": f"{cols}x{rows}", "res": f"{W}x{H}", "views": V, "layout": layout, "runs": runs, "warm": warm, "rows": rows_wanted,
                   "out": f"{OUT_W}x{OUT_H}", "lens": [lens.x_step, lens.y_step, lens.phase0], "native_bytes": OUT_W * OUT_H * 4}
            native = np.full((OUT_H, OUT_W, 4), 0xC3, np.uint8)
            ys = [0, 1, OUT_H // 2, OUT_H - 1]
            k = selection(lens, ys)
            ch = np.arange(3)[None, None, :]
            for tw, th in TILES + [(W, H)]:
                if tw > W or th > H:
                    continue
                tag = f"{tw}x{th}"
                # the native image is the gather of the scaled quilt's tiles (for the views' own size: of the views)
                ctx.download_native(lens, OUT_W, OUT_H, tw, th, out=native)
                sx, sy = nearest(OUT_W, tw)[None, :, None], nearest(OUT_H, th)[ys][:, None, None]
                if (tw, th) == (W, H):
                    src = np.stack([ctx.download_view(v)[nearest(OUT_H, th)[ys]] for v in range(V)])   # [V][len(ys)][W][4]
                    want = src[k, np.arange(len(ys))[:, None, None], sx, ch]
                else:
                    quilt = ctx.download_quilt_scaled(TILES_X, TILES_Y, tw, th)
                    want = quilt[(k // TILES_X) * th + sy, (k % TILES_X) * tw + sx, ch]
                assert (native[ys][..., :3] == want).all() and (native[ys][..., 3] == 255).all(), (name, layout, tag)
                read, written = kernel_bytes(tw, th, layout == "planar" and (tw, th) == (W, H))
                row[f"d_{tag}_min_read_bytes"], row[f"d_{tag}_written_bytes"] = read, written
                row[f"d_{tag}_us_at_8TBs"] = round((read + written) / PEAK_BYTES_PER_S * 1e6, 2)
                if (tw, th) != (W, H):
                    quilt = np.full((TILES_Y * th, TILES_X * tw, 4), 0xC3, np.uint8)
                    row[f"a_{tag}_bytes"] = int(quilt.nbytes)
                    if "a" in rows_wanted:
                        row[f"a_{tag}_wall_ms"], row[f"a_{tag}_event_ms"], row[f"reps_a_{tag}"] = timed(
                            ctx, lambda: ctx.download_quilt_scaled(TILES_X, TILES_Y, tw, th, out=quilt))
                    if "b" in rows_wanted:
                        row[f"b_{tag}_wall_ms"], row[f"b_{tag}_event_ms"], row[f"reps_b_{tag}"] = timed(
                            ctx, lambda: ctx.download_native(lens, OUT_W, OUT_H, tw, th, out=native))
                    if "a" in rows_wanted and "b" in rows_wanted:
                        row[f"b_{tag}_over_a"] = round(row[f"b_{tag}_wall_ms"] / row[f"a_{tag}_wall_ms"], 4)
                elif "c" in rows_wanted:
                    row["c_wall_ms"], row["c_event_ms"], row["reps_c"] = timed(ctx, lambda: ctx.download_native(lens, OUT_W, OUT_H, tw, th, out=native))
            row["workspace_bytes"] = int(ctx.memory_info().workspace_bytes)
            if name == "4k" and "b_1638x910_over_a" in row:
                row["condition_b_below_a_at_1638x910"] = bool(row["b_1638x910_wall_ms"] < row["a_1638x910_wall_ms"])
        print(json.dumps(row), flush=True)
