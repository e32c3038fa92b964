"""Filtered native lenticular images (lfi_download_native under LFI_LENT_BILINEAR and LFI_LENT_BLEND): what the filters cost against the
nearest image and against the scaled quilt a host-side interlace would start from.  Modelled on tools/native_image_time.py.

45 views rendered with TEN_WM from the synthetic grid, a 3840 x 2160 native image, both view layouts, ONE process, one context at a time:
  4k     15 x 15 grid of 3840 x 2160 views: tiles of 819 x 455 and of 1638 x 910 (quilt_scale into the device-resident tiles, then the interlace)
  1080p  8 x 8 grid of 1920 x 1080 views, read in place (tile = view size, no first stage)
Per (case, layout, tile) the calls ALTERNATE inside every one of the `runs` timed rounds — nearest, BILINEAR, BLEND, BILINEAR | BLEND and, for
the 4k tiles, lfi_download_quilt_scaled 5 x 9 of the same tiles (existing code, the yardstick) — after `warm` untimed rounds; medians of the
host clock around the synchronous call and of the HIP-event time of the whole call, into pageable host arrays touched before the timing.
The flag-free call launches native_interlace, the kernel of the parent commit: it is the yardstick the filtered kernels are a ratio of.

  the interlace kernels alone come from a SECOND run of this tool under
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/native_filter_time.py …
      and  python tools/native_filter_time.py --kernels DIR/…_kernel_trace.csv [notes.md]
      which prints, per context (in the tool's order), source of the tiles and kernel: the launches, the median of End_Timestamp −
      Start_Timestamp (device clock) and its ratio to native_interlace on the same tiles, next to the ratio of samples loaded (nearest 1,
      BLEND 2, BILINEAR 4, both 8), and appends the table to the notes.

Writes its tables to `notes` (default profiles/r28_native_filter_notes.md).  Reads nothing but the package.
usage: python tools/native_filter_time.py [runs=20] [warm=3] [notes=profiles/r28_native_filter_notes.md] [case ...]   cases: 4k, 1080p (default: both)"""
import csv
import json
import sys
import time

sys.path.insert(0, ".")
import numpy as np

NOTES = "profiles/r28_native_filter_notes.md"
TILES = [(819, 455), (1638, 910)]
SAMPLES = {"native_interlace": 1, "native_filter<false, true>": 2, "native_filter<true, false>": 4, "native_filter<true, true>": 8}   # <BILINEAR, BLEND>

if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
    with open(sys.argv[2], newline="") as f:
        trace = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    # the trace in launch order: the first blend kernel after any other kernel opens a context (the tool's order: per case, rgba then planar);
    # an interlace launch is labelled with the quilt_scale launch in front of it — the i-th distinct grid of the context made TILES[i] — or "in place"
    groups, context, before, grids = {}, 0, "", []
    for r in trace:
        name = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("lfi::", "")
        grid = "x".join((r.get("Grid_Size_X", r.get("Grid_Size", "")), r.get("Grid_Size_Y", ""), r.get("Grid_Size_Z", "")))
        if "blend_" in name and "blend_" not in before:
            context, grids = context + 1, []
        if "quilt_scale" in name and grid not in grids:
            grids.append(grid)
        if "native_interlace" in name or "native_filter" in name:
            source = "tiles %dx%d" % TILES[grids.index(before.split(" ")[-1])] if "quilt_scale" in before else "in place"
            planar = name.split("<")[1].split(",")[0].strip(" >") == "true"
            kind = "native_interlace" if "native_interlace" in name else "native_filter<" + name.split("<")[1].split(",", 1)[1].strip()
            groups.setdefault((context, source, "planar" if planar else "rgba", kind), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
        before = name + " " + grid
    lines = ["", "## The interlace kernels alone (rocprofv3 --kernel-trace, device clock)", "",
             "| context | tiles | views read as | kernel <BILINEAR, BLEND> | launches | median ms | min | max | ratio to native_interlace | samples loaded |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for key, ms in sorted(groups.items()):
        base = groups.get(key[:3] + ("native_interlace",))
        row = {"context": key[0], "source": key[1], "views": key[2], "kernel": key[3], "launches": len(ms), "median_ms": round(float(np.median(ms)), 4),
               "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "ratio_to_interlace": round(float(np.median(ms) / np.median(base)), 2) if base else None,
               "samples": SAMPLES.get(key[3])}
        print(json.dumps(row), flush=True)
        lines.append("| {context} | {source} | {views} | {kernel} | {launches} | {median_ms} | {min_ms} | {max_ms} | {ratio_to_interlace} | {samples} x |".format(**row))
    if len(sys.argv) > 3:
        with open(sys.argv[3], "a") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)

import lfinterpolator_amd as L

CASES = {
    # name: cols, rows, W, H, trajectory, focus, aspect, tiles
    "4k": (15, 15, 3840, 2160, "0,0.5,1,0.5", 0.06, 2.276, TILES),
    "1080p": (8, 8, 1920, 1080, "0.0,0.0,1.0,1.0", 0.23, 1.783, [(1920, 1080)]),
}
V, TILES_X, TILES_Y = 45, 5, 9
OUT_W, OUT_H = 3840, 2160
CALIBRATION = (47.5636, -5.4392, 0.0412, 338.0, False)   # lenses per inch, slant, centre, dpi, invert: of the order of a 4K lenticular panel
FLAGS = {"nearest": 0, "bilinear": L.LFI_LENT_BILINEAR, "blend": L.LFI_LENT_BLEND, "bilinear_blend": L.LFI_LENT_BILINEAR | L.LFI_LENT_BLEND}
args = sys.argv[1:]
runs = int(args[0]) if args else 20
warm = int(args[1]) if len(args) > 1 else 3
notes = args[2] if len(args) > 2 else NOTES
names = args[3:] or list(CASES)


def alternating(ctx, calls):
    """{name: (median host wall ms, median event ms)} of the synchronous calls, every round running each of them once, in order"""
    for _ in range(warm):
        for fn in calls.values():
            fn()
    wall, ev = {k: [] for k in calls}, {k: [] for k in calls}
    for _ in range(runs):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            ctx.timer_start()
            fn()
            ev[k].append(ctx.timer_stop())
            wall[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (round(float(np.median(wall[k])), 4), round(float(np.median(ev[k])), 4)) for k in calls}


def with_flags(lens, flags):
    return L.Lenticular(lens.x_step, lens.y_step, lens.phase0, lens.views, lens.flags | flags)


lens = L.lenticular(*CALIBRATION, OUT_W, OUT_H, V)
table = ["# Filtered native images: what bilinear tiles and view blending cost", "",
         f"`python tools/native_filter_time.py {runs} {warm}`: {V} views, native image {OUT_W} x {OUT_H}, medians of {runs} alternating rounds after {warm} warm-ups; host clock around "
         "the synchronous call (HIP-event time of the whole call in brackets), milliseconds.  `quilt` is lfi_download_quilt_scaled 5 x 9 of the same tiles.", "",
         "| case | views read as | tiles | nearest | bilinear | blend | bilinear + blend | quilt | bilinear + blend below quilt |", "|---|---|---|---|---|---|---|---|---|"]
for name in names:
    cols, rows, W, H, traj, f, aspect, tiles = CASES[name]
    hp = L.build_params(cols, rows, W, H, traj, f, 0.0, 3.0, aspect, V)
    for layout in ("rgba", "planar"):
        with L.Context(0) as ctx:
            ctx.set_grid(cols, rows, W, H)
            ctx.fill_synthetic(0x1F1F)
            ctx.set_params(hp)
            ctx.set_output_layout(layout)
            ctx.render("TEN_WM")
            ctx.sync()
            native = np.full((OUT_H, OUT_W, 4), 0xC3, np.uint8)
            for tw, th in tiles:
                row = {"case": name, "grid": f"{cols}x{rows}", "res": f"{W}x{H}", "views": V, "layout": layout, "tile": f"{tw}x{th}", "out": f"{OUT_W}x{OUT_H}", "runs": runs,
                       "warm": warm, "native_bytes": int(native.nbytes)}
                calls = {k: (lambda fl=fl: ctx.download_native(with_flags(lens, fl), OUT_W, OUT_H, tw, th, out=native)) for k, fl in FLAGS.items()}
                # the filters are seen: each flag set's image differs from the nearest one, and alpha stays 255
                images = {}
                for k, fn in calls.items():
                    fn()
                    images[k] = native[::97].copy()
                    assert (images[k][..., 3] == 255).all() and (k == "nearest" or (images[k] != images["nearest"]).any()), (name, layout, k)
                if (tw, th) != (W, H):
                    quilt = np.full((TILES_Y * th, TILES_X * tw, 4), 0xC3, np.uint8)
                    row["quilt_bytes"] = int(quilt.nbytes)
                    calls["quilt"] = lambda: ctx.download_quilt_scaled(TILES_X, TILES_Y, tw, th, out=quilt)
                for k, (wall_ms, event_ms) in alternating(ctx, calls).items():
                    row[f"{k}_wall_ms"], row[f"{k}_event_ms"] = wall_ms, event_ms
                if "quilt_wall_ms" in row:
                    row["bilinear_blend_below_quilt"] = bool(row["bilinear_blend_wall_ms"] < row["quilt_wall_ms"])
                print(json.dumps(row), flush=True)
                cell = lambda k: f"{row[k + '_wall_ms']} ({row[k + '_event_ms']})" if k + "_wall_ms" in row else "—"
                table.append(f"| {name} | {layout} | {'in place' if (tw, th) == (W, H) else row['tile']} | {cell('nearest')} | {cell('bilinear')} | {cell('blend')} | "
                             f"{cell('bilinear_blend')} | {cell('quilt')} | {row.get('bilinear_blend_below_quilt', '—')} |")
with open(notes, "w") as f:
    f.write("\n".join(table) + "\n")
