"""RGB-D video frames (lfi_download_rgbd_yuv): what a view with its focus map beside it costs as YUV 4:2:0 frames.
Per case, in ONE process on one context (the synthetic grid, a view-centred all-focus STD render of 8 views, the focus map at the
trajectory's centre and the per-view maps), medians of `runs` timed calls after `warm` warm-ups, into memory allocated and touched before the
timing.  Tiles: the views' own size and half of it.  Rows: n = 1 with the context's map, n = 8 with the per-view maps (LFI_RGBD_VIEW_MAPS).
  (a) what a caller does today: lfi_download_view + lfi_download_map (n = 8: lfi_download_view_map) per view into page-locked RGBA images,
      8 bytes per pixel and view (existing code, untouched);
  (b) lfi_download_rgbd_yuv, whole call into page-locked tight I420 frames (the kernel, the copies): 3 bytes per pixel at the views' size;
  (c) lfi_download_rgbd_yuv into device NV12 surfaces written in place (the kernel alone: nothing crosses PCIe);
  (d) the three-channel body the depth half would otherwise run: lfi_download_quilt_yuv of a 2 x 1 quilt of two VIEWS at the same tile, into
      a device NV12 surface in place (n = 8: eight such calls, one per frame).
Host clock and, beside it, the HIP-event time of the whole call(s).  The kernels' own times — rgbd_yuv_scale against quilt_yuv_scale on the
2 x 1 quilt, same grid of workgroups — come from a SECOND run of this tool under
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/rgbd_yuv_time.py …       (no counters in the same run)
and
  python tools/rgbd_yuv_time.py --kernels DIR/…_kernel_trace.csv
which prints, per kernel name and grid, the number of launches and the median of End_Timestamp − Start_Timestamp (device clock).
Reads nothing but the package.
usage: python tools/rgbd_yuv_time.py [runs=20] [warm=3] [case ...]   cases: 1080p, 4k (default: both)"""
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
            if "rgbd_yuv_scale" not in name and "quilt_yuv_scale" not in name:
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
    # name: cols, rows, W, H, trajectory, focus, range, aspect
    "1080p": (8, 8, 1920, 1080, "0.0,0.0,1.0,1.0", 0.1, 0.3, 1.783),
    "4k": (15, 15, 3840, 2160, "0.071,0.071,0.93,0.93", 0.1, 0.3, 1.0),
}
V = 8
args = sys.argv[1:]
runs = int(args[0]) if args else 20
warm = int(args[1]) if len(args) > 1 else 3
names = args[2:] or list(CASES)


def timed(ctx, fn):
    """(median host wall ms, median event ms) of the synchronous call(s) fn"""
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


def nv12_device(w, h, n):
    """n NV12 surfaces of w x h with pitches of 256 in device memory: written in place"""
    pitch = up(w, 256)
    stride = pitch * h * 3 // 2
    dev = torch.empty(stride * n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return L.YuvSurfaces.make("nv12", "device", dev.data_ptr(), stride, pitch, pitch * h, pitch, 0, keep=dev)


for name in names:
    cols, rows, W, H, traj, f, rng, aspect = CASES[name]
    hp = L.build_params(cols, rows, W, H, traj, f, rng, 3.0, aspect, V)
    O, _ = L.build_view_centred_offsets(cols, rows, W, H, traj, aspect, np.full(V, f, np.float32))
    ids = L.build_view_focus_ids(cols, rows, traj, V)
    with L.Context(0) as ctx:
        ctx.set_grid(cols, rows, W, H)
        ctx.fill_synthetic(0x1F1F)
        ctx.set_params(hp)
        ctx.set_view_float_offsets(O)
        ctx.focus_map()
        ctx.view_focus_maps(ids)
        ctx.render("STD", all_focus=True)
        ctx.sync()
        lib, h = ctx._lib, ctx._h
        images = ctx.pinned_empty((2 * V, H, W, 4))
        images.fill(0xC3)   # touched before the timing: no page faults inside it
        for tw, th in ((W, H), (W // 2, H // 2)):
            for n, flags in ((1, 0), (V, L.LFI_RGBD_VIEW_MAPS)):
                row = {"case": name, "grid": f"{cols}x{rows}", "res": f"{W}x{H}", "tile": f"{tw}x{th}", "n": n, "view_maps": bool(flags), "runs": runs, "warm": warm}

                def today():
                    for v in range(n):
                        ctx._check(lib.lfi_download_view(h, v, images[2 * v].ctypes.data, W * 4))
                        if flags:
                            ctx._check(lib.lfi_download_view_map(h, v, 1, images[2 * v + 1].ctypes.data, W * 4))
                        else:
                            ctx._check(lib.lfi_download_map(h, 1, images[2 * v + 1].ctypes.data, W * 4))

                row["a_today_wall_ms"], row["a_today_event_ms"] = timed(ctx, today)
                row["a_bytes"] = 8 * W * H * n
                frames = ctx.pinned_empty((n, 2 * tw * th * 3 // 2))
                frames.fill(0xC3)
                host = L.yuv_surfaces_packed("i420", "host", frames.ctypes.data, 2 * tw, th, keep=frames)
                row["b_i420_wall_ms"], row["b_i420_event_ms"] = timed(ctx, lambda: ctx.download_rgbd_yuv(0, n, 1, flags, tw, th, "709", "limited", host))
                row["b_bytes"] = int(frames.nbytes)
                row["b_over_a_wall"] = round(row["b_i420_wall_ms"] / row["a_today_wall_ms"], 4)
                row["b_over_a_bytes"] = round(row["b_bytes"] / row["a_bytes"], 4)
                surf = nv12_device(2 * tw, th, n)
                row["c_device_nv12_wall_ms"], row["c_device_nv12_event_ms"] = timed(ctx, lambda: ctx.download_rgbd_yuv(0, n, 1, flags, tw, th, "709", "limited", surf))
                one = nv12_device(2 * tw, th, 1)

                def three_channel():
                    for v in range(n):
                        ctx.download_quilt_yuv(2, 1, min(v, V - 2), tw, th, "709", "limited", one)

                row["d_quilt_2x1_wall_ms"], row["d_quilt_2x1_event_ms"] = timed(ctx, three_channel)
                row["c_over_d_event"] = round(row["c_device_nv12_event_ms"] / row["d_quilt_2x1_event_ms"], 4)
                print(json.dumps(row), flush=True)
                del surf, one
