"""Chroma siting (lfi_set_yuv_siting): what the left-sited kernels cost beside the centre-sited ones.  ONE process, one context per case, both
sitings ALTERNATING launch by launch; per measurement the median of `runs` device-event times (lfi_timer_start / lfi_timer_stop on the
context's stream, set to a stream of the tool's own) after `warm` warm-ups, and the spread of `repeats` such medians:
  convert   lfi_download_views_yuv of 64 views into 16-byte aligned NV12 / I420 device surfaces written in place — ONE launch of yuvs_convert
            or yuvs_convert_left, from RGBA and from planar views;
  expand    lfi_upload_images_yuv of 64 frames from NV12 / I420 device surfaces read in place — ONE launch of yuvs_expand or yuvs_expand_left
            on the copy stream; the timed region ends with lfi_upload_wait, so it holds one host wait (the kernels alone: the trace below);
  quilt     lfi_download_quilt_yuv of an 8 x 8 quilt of even tiles (a quarter of the views' size each way) into an NV12 device surface:
            centre-sited the fused quilt_yuv_scale, left-sited quilt_scale + yuvs_convert_left.
A build without lfi_set_yuv_siting (the commit before it) runs the centre-sited half alone: the control of an A/B between two builds, run
from that build's directory.  The kernels alone come from a second run under
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/yuv_siting_time.py 5 1 1
and python tools/yuv_siting_time.py --kernels DIR/…_kernel_trace.csv, which prints per kernel and grid the number of launches and the median
of End_Timestamp − Start_Timestamp.  Before anything is timed one frame of each direction is held against the numpy restatements.
usage: python tools/yuv_siting_time.py [runs=20] [warm=3] [repeats=5] [case ...]   cases: 1080p, 4k (default: both)"""
import csv
import json
import sys

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np

CASES = {"1080p": (8, 8, 1920, 1080), "4k": (15, 15, 3840, 2160)}   # name: cols, rows, W, H
N = 64   # views converted, frames expanded

if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
    with open(sys.argv[2], newline="") as f:
        trace = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    groups = {}
    for r in trace:
        name = r["Kernel_Name"].split("(")[0]
        if "yuv" not in name and "quilt_scale" not in name:
            continue
        grid = (int(r.get("Grid_Size_X", r.get("Grid_Size", 0))), int(r.get("Grid_Size_Y", 0) or 0), int(r.get("Grid_Size_Z", 0) or 0))
        groups.setdefault((name, grid), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    for (name, grid), ms in groups.items():
        print(json.dumps({"kernel": name, "grid_threads": "x".join(map(str, grid)), "launches": len(ms), "median_ms": round(float(np.median(ms)), 4),
                          "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}), flush=True)
    sys.exit(0)

import torch

import lfinterpolator_amd as L
import yuv_in_ref as in_ref
import yuv_ref as out_ref
import yuv_surfaces_ref as sref

args = sys.argv[1:]
runs = int(args[0]) if args else 20
warm = int(args[1]) if len(args) > 1 else 3
repeats = int(args[2]) if len(args) > 2 else 5
names = args[3:] or list(CASES)
HAS_SITING = hasattr(L.Context, "set_yuv_siting")
SITINGS = ("centre", "left") if HAS_SITING else ("centre",)
if HAS_SITING:
    import yuv_left_ref as left_ref


def alternating(ctx, calls):
    """{siting: [repeats medians of `runs` device-event ms]}; calls[siting] sets the siting and makes the call, which ends on the host"""
    out = {s: [] for s in calls}
    for _ in range(repeats):
        ms = {s: [] for s in calls}
        for k in range(warm + runs):
            for s, call in calls.items():
                ctx.timer_start()
                call()
                t = ctx.timer_stop()
                if k >= warm:
                    ms[s].append(t)
        for s in calls:
            out[s].append(round(float(np.median(ms[s])), 4))
    return out


def report(row, key, medians):
    for s, m in medians.items():
        row[f"{key}_{s}_ms"] = round(float(np.median(m)), 4)
        row[f"{key}_{s}_spread"] = [min(m), max(m)]
    if "left" in medians:
        row[f"{key}_left_over_centre"] = round(row[f"{key}_left_ms"] / row[f"{key}_centre_ms"], 4)


def sited(ctx, in_s, out_s, fn):
    def call():
        if HAS_SITING:
            ctx.set_yuv_siting(in_s, out_s)
        fn()
    return call


for name in names:
    cols, rows, W, H = CASES[name]
    fb = in_ref.sizes(W, H)[2]
    assert W % 16 == 0 and (W * H) % 16 == 0 and fb % 16 == 0   # tight device surfaces are read and written in place
    stream = torch.cuda.Stream(device="cuda:0")
    with L.Context(0) as ctx:
        ctx.set_grid(cols, rows, W, H)
        grid = torch.zeros((cols * rows, H, W, 4), dtype=torch.uint8, device="cuda:0")   # attached, so that the images can be read back
        torch.cuda.synchronize()
        ctx.attach_grid(grid.data_ptr(), grid.numel())
        ctx.set_stream(stream.cuda_stream)
        ctx.fill_synthetic(7)
        ctx.set_params(L.build_params(cols, rows, W, H, "0,0.5,1,0.5", 0.1, 0.0, 3.0, 1.0, N))
        row = {"case": name, "grid": f"{cols}x{rows}", "res": f"{W}x{H}", "n": N, "runs": runs, "warm": warm, "repeats": repeats, "sitings": list(SITINGS)}
        dev = {f: torch.zeros((N, fb), dtype=torch.uint8, device="cuda:0") for f in ("i420", "nv12")}
        torch.cuda.synchronize()
        surf = {f: ctx.yuv_surfaces_packed(f, "device", dev[f].data_ptr(), keep=dev[f]) for f in dev}
        frame_ref = {"centre": out_ref.frame, **({"left": left_ref.frame} if HAS_SITING else {})}
        image_ref = {"centre": in_ref.rgba, **({"left": left_ref.rgba} if HAS_SITING else {})}
        # views -> frames
        for layout in ("rgba", "planar"):
            ctx.set_output_layout(layout)
            ctx.render("TEN_WM")
            ctx.sync()
            view0 = ctx.download_view(0)
            for f in dev:
                calls = {s: sited(ctx, "centre", s, lambda f=f: ctx.download_views_yuv(surf[f])) for s in SITINGS}
                for s, call in calls.items():
                    call()
                    torch.cuda.synchronize()
                    got = sref.gather(dev[f][:1].cpu().numpy(), sref.tight(sref.NV12 if f == "nv12" else sref.I420, W, H))[0]
                    assert (got == frame_ref[s](view0, out_ref.BT709, out_ref.LIMITED)).all(), (name, layout, f, s)
                report(row, f"convert_{layout}_{f}", alternating(ctx, calls))
        # the quilt: 8 x 8 tiles of a quarter of the views' size, one NV12 frame the size of four views
        tw, th = W // 4, H // 4
        qdev = torch.zeros((in_ref.sizes(8 * tw, 8 * th)[2],), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        qsurf = L.yuv_surfaces_packed("nv12", "device", qdev.data_ptr(), 8 * tw, 8 * th, keep=qdev)
        calls = {s: sited(ctx, "centre", s, lambda: ctx.download_quilt_yuv(8, 8, 0, tw, th, 0, 0, qsurf)) for s in SITINGS}
        for call in calls.values():
            call()
        report(row, "quilt_nv12", alternating(ctx, calls))
        # frames -> images: the frames just written, read in place; the timed region ends with the host's wait for the copy stream
        for f in dev:
            def upload(f=f):
                ctx.upload_images_yuv(surf[f], N)
                ctx.upload_wait()
            calls = {s: sited(ctx, s, "centre", upload) for s in SITINGS}
            frame0 = sref.gather(dev[f][:1].cpu().numpy(), sref.tight(sref.NV12 if f == "nv12" else sref.I420, W, H))[0]
            for s, call in calls.items():
                call()
                ctx.sync()
                torch.cuda.synchronize()
                assert (grid[0].cpu().numpy() == image_ref[s](frame0, W, H, in_ref.BT709, in_ref.LIMITED)).all(), (name, f, s)
            report(row, f"expand_{f}", alternating(ctx, calls))
        print(json.dumps(row), flush=True)
    del dev, qdev, grid
