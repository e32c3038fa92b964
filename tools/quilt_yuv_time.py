"""Quilt video frames (lfi_download_quilt_yuv): what one 5 x 9 quilt frame costs as YUV 4:2:0, against the RGBA scaled quilt of the same tiles.
Per case, in ONE process on one context (the synthetic grid, a TEN_WM render, 45 views), for each view layout, medians of `runs` timed calls
after `warm` warm-ups, into memory allocated and touched before the timing:
  (a) lfi_download_quilt_scaled 5 x 9, whole call into a page-locked RGBA image (the reference of bar 1: existing code);
  (b) lfi_download_quilt_yuv 5 x 9, whole call into a page-locked tight I420 frame (fused kernel, device-side pack, copies);  b / a next to 0.375
  (c) lfi_download_quilt_yuv into a device NV12 surface written in place (the fused kernel alone: no copy, nothing crosses PCIe);
  (d) 1080p only: the staged path at 819 x 455 tiles (quilt_scale + yuvs_convert + copy) into a page-locked I420 frame.
Host clock and, beside it, the HIP-event time of the whole call.  The kernels' own times — quilt_yuv_scale against quilt_scale for the same
tiles (bar 2: at most 1.10 x), and quilt_scale + yuvs_convert of the staged path — come from a SECOND run of this tool under
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/quilt_yuv_time.py …       (no counters in the same run)
and
  python tools/quilt_yuv_time.py --kernels DIR/…_kernel_trace.csv
which prints, per kernel name and grid, the number of launches and the median of End_Timestamp − Start_Timestamp (device clock).
Reads nothing but the package.
usage: python tools/quilt_yuv_time.py [runs=20] [warm=3] [case ...]   cases: 1080p, 4k (default: both)"""
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
            if "quilt_" not in name and "yuvs_convert" not in name:
                continue
            key = (name.split("(")[0], r.get("Grid_Size_X", r.get("Grid_Size", "")), r.get("Grid_Size_Y", ""), r.get("Grid_Size_Z", ""))
            groups.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    for key, ms in sorted(groups.items()):
        print(json.dumps({"kernel": key[0], "grid": "x".join(key[1:]), "launches": len(ms), "median_ms": round(float(np.median(ms)), 4),
                          "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}), flush=True)
    sys.exit(0)

import torch

import lfinterpolator_amd as L

CASES = {
    # name: cols, rows, W, H, trajectory, focus, aspect, views, the even tile (fused), the odd tile (staged; None: not measured)
    "1080p": (15, 15, 1920, 1080, "0,0.5,1,0.5", 0.06, 2.276, 45, (820, 456), (819, 455)),     # BASELINE config 3's shape
    "4k": (8, 8, 3840, 2160, "0.0,0.0,1.0,1.0", 0.23, 1.783, 45, (1638, 910), None),
}
TX, TY = 5, 9
args = sys.argv[1:]
runs = int(args[0]) if args else 20
warm = int(args[1]) if len(args) > 1 else 3
names = args[2:] or list(CASES)


def timed(ctx, fn):
    """(median host wall ms, median event ms) of the synchronous call fn"""
    for _ in range(warm):
        fn()
    ev, wall = [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        ctx.timer_start()
        fn()
        ev.append(ctx.timer_stop())
        wall.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(wall)), 4), round(float(np.median(ev)), 4)


def up(v, a):
    return (v + a - 1) // a * a


for name in names:
    cols, rows, W, H, traj, f, aspect, V, even, odd = CASES[name]
    hp = L.build_params(cols, rows, W, H, traj, f, 0.0, 3.0, aspect, V)
    for layout in ("rgba", "planar"):
        with L.Context(0) as ctx:
            ctx.set_grid(cols, rows, W, H)
            ctx.fill_synthetic(0x1F1F)
            ctx.set_params(hp)
            ctx.set_output_layout(layout)
            ctx.render("TEN_WM")
            ctx.sync()
            row = {"case": name, "layout": layout, "grid": f"{cols}x{rows}", "res": f"{W}x{H}", "views": V, "quilt": f"{TX}x{TY}", "runs": runs, "warm": warm}
            tw, th = even
            qw, qh = TX * tw, TY * th
            row["tile"] = f"{tw}x{th}"
            rgba = ctx.pinned_empty((qh, qw, 4))
            rgba.fill(0xC3)   # touched before the timing: no page faults inside it
            row["a_rgba_wall_ms"], row["a_rgba_event_ms"] = timed(ctx, lambda: ctx.download_quilt_scaled(TX, TY, tw, th, out=rgba))
            row["a_bytes"] = int(rgba.nbytes)
            frame = ctx.pinned_empty((qw * qh * 3 // 2,))
            frame.fill(0xC3)
            host = L.yuv_surfaces_packed("i420", "host", frame.ctypes.data, qw, qh, keep=frame)
            row["b_i420_wall_ms"], row["b_i420_event_ms"] = timed(ctx, lambda: ctx.download_quilt_yuv(TX, TY, 0, tw, th, "709", "limited", host))
            row["b_bytes"] = int(frame.nbytes)
            row["b_over_a_wall"] = round(row["b_i420_wall_ms"] / row["a_rgba_wall_ms"], 4)
            row["b_over_a_bytes"] = round(row["b_bytes"] / row["a_bytes"], 4)
            # a device NV12 surface with pitches of 256: written in place
            pitch = up(qw, 256)
            dev = torch.empty(pitch * qh * 3 // 2, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            surf = L.YuvSurfaces.make("nv12", "device", dev.data_ptr(), pitch * qh * 3 // 2, pitch, pitch * qh, pitch, 0, keep=dev)
            row["c_device_nv12_wall_ms"], row["c_device_nv12_event_ms"] = timed(ctx, lambda: ctx.download_quilt_yuv(TX, TY, 0, tw, th, "709", "limited", surf))
            if odd:
                ow, oh = odd
                sw, sh = TX * ow, TY * oh
                fb = sw * sh + 2 * ((sw + 1) // 2) * ((sh + 1) // 2)
                sframe = ctx.pinned_empty((fb,))
                sframe.fill(0xC3)
                shost = L.yuv_surfaces_packed("i420", "host", sframe.ctypes.data, sw, sh, keep=sframe)
                row["d_staged_tile"] = f"{ow}x{oh}"
                row["d_staged_wall_ms"], row["d_staged_event_ms"] = timed(ctx, lambda: ctx.download_quilt_yuv(TX, TY, 0, ow, oh, "709", "limited", shost))
                srgba = ctx.pinned_empty((sh, sw, 4))
                srgba.fill(0xC3)
                row["d_rgba_wall_ms"], row["d_rgba_event_ms"] = timed(ctx, lambda: ctx.download_quilt_scaled(TX, TY, ow, oh, out=srgba))
            del dev
        print(json.dumps(row), flush=True)
