"""Deep views (LFI_FLAG_DEEP_VIEWS): what the 10-bit planes cost, against the kernels they are modelled on.
In ONE process, two contexts over the same synthetic grid — one with the flag, one without — are timed alternately, launch by launch: per side the
median of `runs` device-event times (lfi_timer_start / lfi_timer_stop around one launch) after `warm` warm-ups of both.  Planar view layout on
both sides.
  ten    deep_blend<TEN_WM> against blend_p3<TEN_WM>.  Yardstick: the bytes moved per pixel — 3 per image in, and per view 3 out (bytes) against
         3 + 6 out (bytes + u16 codes): (3N + 9V) / (3N + 3V), 2.0 at 8 x 8 with 64 views.
  std    deep_blend<STD> against the chain kernels it is modelled on, the variants "wave_m2_nt" (the chain on v_mfma_f32_32x32x2_f32) and
         "vfma" (the vector pipe), and against the default band method.
  yuv    lfi_download_views_yuv into device P010 surfaces written in place: LFI_YUV_P010 | LFI_YUV_DEEP (deep_convert10) against LFI_YUV_P010
         (yuvs_convert10 from the planar views).  Yardstick: 6 bytes read per pixel against 3, 3 written by both: 9 / 6.  The time is the whole
         synchronous call's (one launch and the wait for it).
The kernels' own times come from a SECOND run of this tool under
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/deep_views_time.py runs=5 …
and  python tools/deep_views_time.py --kernels DIR/…_kernel_trace.csv
which prints, per kernel name and grid, the number of launches and the median of End_Timestamp − Start_Timestamp (device clock).
Writes one JSON line per row to stdout and, with out=PATH, the same rows as a markdown table to PATH.  Reads nothing but the package.
usage: python tools/deep_views_time.py [runs=20] [warm=3] [out=PATH] [case ...]   cases: 1080p, 4k (default: both; std rows at 1080p only)"""
import json
import sys

sys.path.insert(0, ".")
import numpy as np

if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
    import csv
    groups = {}
    with open(sys.argv[2], newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if not any(stem in name for stem in ("deep_", "blend_", "yuvs_convert10")):
                continue
            key = (name.split("(")[0], r.get("Grid_Size_X", r.get("Grid_Size", "")), r.get("Workgroup_Size_X", r.get("Workgroup_Size", "")))
            groups.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    for key, ms in sorted(groups.items()):
        print(json.dumps({"kernel": key[0], "grid": key[1], "workgroup": key[2], "launches": len(ms), "median_ms": round(float(np.median(ms)), 4),
                          "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}), flush=True)
    sys.exit(0)

import _ablib  # noqa: F401  (LFI_AB_LIB: another build's library, one process per library)
import lfinterpolator_amd as L

CASES = {
    # name: cols, rows, W, H, trajectory, focus, aspect, views
    "1080p": (8, 8, 1920, 1080, "0.0,0.0,1.0,1.0", 0.23, 1.783, 64),
    "4k": (15, 15, 3840, 2160, "0,0.5,1,0.5", 0.06, 2.276, 64),
}
runs, warm, out_path, names = 20, 3, None, []
for arg in sys.argv[1:]:
    if arg.startswith("runs="):
        runs = int(arg[5:])
    elif arg.startswith("warm="):
        warm = int(arg[5:])
    elif arg.startswith("out="):
        out_path = arg[4:]
    else:
        names.append(arg)
names = names or list(CASES)
rows_out = []


def alternate(sides):
    """sides: [(label, ctx, fn)]; one launch of each in turn, `warm` rounds untimed, `runs` timed: {label: (median ms, min, max)}"""
    times = {label: [] for label, _, _ in sides}
    for r in range(warm + runs):
        for label, ctx, fn in sides:
            ctx.timer_start()
            fn()
            ms = ctx.timer_stop()
            if r >= warm:
                times[label].append(ms)
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in times.items()}


def report(case, what, label, kernel, t, base=None, yardstick=None):
    row = {"case": case, "what": what, "side": label, "kernel": kernel, "median_ms": round(t[0], 4), "min_ms": round(t[1], 4), "max_ms": round(t[2], 4)}
    if base is not None:
        row["ratio_to_base"] = round(t[0] / base[0], 3)
    if yardstick is not None:
        row["bytes_yardstick"] = round(yardstick, 3)
    rows_out.append(row)
    print(json.dumps(row), flush=True)


def context(cols, rows, W, H, hp, flags):
    ctx = L.Context(0)
    ctx.set_grid(cols, rows, W, H)
    ctx.fill_synthetic(0x1F1F)
    ctx.set_output_layout("planar")
    ctx.set_params(hp, flags=flags)
    return ctx


for name in names:
    cols, rows, W, H, traj, f, aspect, V = CASES[name]
    N = cols * rows
    hp = L.build_params(cols, rows, W, H, traj, f, 0.0, 3.0, aspect, V)
    deep, plain = context(cols, rows, W, H, hp, L.LFI_FLAG_DEEP_VIEWS), context(cols, rows, W, H, hp, 0)
    for ctx in (deep, plain):
        ctx.prepare("TEN_WM")   # the copy tuned, the deep planes allocated: every timed render is only a launch
    t = alternate([("deep", deep, lambda: deep.render("TEN_WM")), ("plain", plain, lambda: plain.render("TEN_WM"))])
    deep_name, plain_name = deep.last_kernel_name(), plain.last_kernel_name()
    assert (deep.download_view(V // 2) == plain.download_view(V // 2)).all()   # the same bytes
    report(name, "ten", "plain", plain_name, t["plain"])
    report(name, "ten", "deep", deep_name, t["deep"], t["plain"], (3 * N + 9 * V) / (3 * N + 3 * V))
    if name == "1080p":
        deep.prepare("STD")
        sides = [("deep", deep, lambda: deep.render("STD"))]
        others = {}
        for variant in ("wave_m2_nt", "vfma", "auto"):
            c = context(cols, rows, W, H, hp, 0)
            c.set_variant("STD", variant)
            c.prepare("STD")
            others[variant] = c
            sides.append((variant, c, (lambda c=c: c.render("STD"))))
        t = alternate(sides)
        assert (deep.download_view(V // 2) == others["vfma"].download_view(V // 2)).all()
        for variant, c in others.items():
            report(name, "std", variant, c.last_kernel_name(), t[variant])
        for variant in ("wave_m2_nt", "vfma"):
            row_t = t["deep"]
            report(name, "std", f"deep vs {variant}", deep.last_kernel_name(), row_t, t[variant])
        for c in others.values():
            c.close()
        deep.render("TEN_WM")
    # frames: device P010 surfaces with pitches of 256, written in place
    import torch
    cw, ch = (W + 1) // 2, (H + 1) // 2
    y_pitch = (2 * W + 255) // 256 * 256
    c_pitch = (4 * cw + 255) // 256 * 256
    stride = H * y_pitch + ch * c_pitch
    frames = torch.zeros((V, stride), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for ctx in (deep, plain):
        ctx.sync()
    s_plain = L.YuvSurfaces.make(L.LFI_YUV_P010, "device", frames.data_ptr(), stride, y_pitch, H * y_pitch, c_pitch, 0, keep=frames)
    s_deep = L.YuvSurfaces.make(L.LFI_YUV_P010 | L.LFI_YUV_DEEP, "device", frames.data_ptr(), stride, y_pitch, H * y_pitch, c_pitch, 0, keep=frames)
    t = alternate([("deep", deep, lambda: deep.download_views_yuv(s_deep)), ("plain", deep, lambda: deep.download_views_yuv(s_plain))])
    report(name, "yuv", "plain", "yuvs_convert10<planar,P010>", t["plain"])
    report(name, "yuv", "deep", "deep_convert10<P010>", t["deep"], t["plain"], 9 / 6)
    del frames
    deep.close()
    plain.close()

if out_path:
    with open(out_path, "w") as fh:
        fh.write(f"| case | what | side | kernel | median ms | min | max | ratio to its base | bytes yardstick |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in rows_out:
            fh.write(f"| {r['case']} | {r['what']} | {r['side']} | `{r['kernel']}` | {r['median_ms']} | {r['min_ms']} | {r['max_ms']} | "
                     f"{r.get('ratio_to_base', '')} | {r.get('bytes_yardstick', '')} |\n")
        fh.write(f"\nmedians of {runs} device-event times per side, the sides alternating launch by launch in one process, {warm} warm-up rounds\n")
