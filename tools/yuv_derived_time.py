"""lfi_upload_images_yuv_derived: what a video time step costs on the input side when the frames go straight into the planar copy of the
inputs, against the two passes it replaces.  Per case, in ONE process, on the same frames, two contexts with the same parameters:
  (a) the existing path, on a context that holds its RGBA planes: lfi_upload_images_yuv (yuvs_expand) plus the planar_build its next render
      triggers (lfi_prepare brings the copy up to date exactly as that render would, and renders nothing) — the baseline;
  (b) the new call on a context whose inputs were released (lfi_prepare behind it only orders the compute stream after the copy stream);
from NV12 device surfaces read in place and from page-locked host I420 frames.  Each figure is the median of `runs` device-event times after
`warm` warm-ups: the contexts compute on a torch stream (lfi_set_stream) and torch events on that stream bracket a step, so a step counts from
the moment the stream reaches it to the moment the copy is ready for a render.  Before anything is timed the first and the last image of
(b)'s copy are held against (a)'s, byte for byte, and both layouts against each other.
The kernels alone come from a SECOND run of this tool under
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/yuv_derived_time.py 3 1
and  python tools/yuv_derived_time.py --kernels DIR/…_kernel_trace.csv
which prints, per kernel and grid of launches, the number of launches and the median of End_Timestamp − Start_Timestamp (device clock).
Reads nothing but the package and tests/.
usage: python tools/yuv_derived_time.py [runs=20] [warm=3] [case ...]   cases: 1080p, 4k (default: both)"""
import csv
import json
import sys

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np

CASES = {
    # name: cols, rows, W, H
    "1080p": (8, 8, 1920, 1080),
    "4k": (15, 15, 3840, 2160),
}
VIEWS = 8
HBM_PEAK_GBPS = 8000.0   # MI355X, HBM3E specification

if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
    with open(sys.argv[2], newline="") as f:
        trace = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    groups = {}
    for r in trace:
        name = r["Kernel_Name"].split("(")[0]
        if "yuvs_" not in name and "planar_build" not in name:
            continue
        grid = (int(r.get("Grid_Size_X", r.get("Grid_Size", 0))), int(r.get("Grid_Size_Y", 0) or 0), int(r.get("Grid_Size_Z", 0) or 0))
        groups.setdefault((name, grid), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    for (name, grid), ms in groups.items():
        print(json.dumps({"kernel": name, "grid_threads": "x".join(map(str, grid)), "launches": len(ms), "median_ms": round(float(np.median(ms)), 4),
                          "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}), flush=True)
    sys.exit(0)

import torch

import lfinterpolator_amd as L
import yuv_in_ref as ref
import yuv_surfaces_ref as sref

args = sys.argv[1:]
runs = int(args[0]) if args else 20
warm = int(args[1]) if len(args) > 1 else 3
names = args[2:] or list(CASES)

for name in names:
    cols, rows, W, H = CASES[name]
    n = cols * rows
    fb = ref.sizes(W, H)[2]
    nv12 = sref.tight(sref.NV12, W, H)
    hp = L.build_params(cols, rows, W, H, "0,0.5,1,0.5", 0.1, 0.0, 3.0, 1.0, VIEWS)
    stream = torch.cuda.Stream(device="cuda:0")
    with L.Context(0) as full, L.Context(0) as lean:
        some = np.random.default_rng(7).integers(0, 256, (4, fb), dtype=np.uint8)
        some_nv12 = sref.scatter(some, nv12, 0)
        i420_host, nv12_host = full.pinned_empty((n, fb)), np.empty((n, fb), np.uint8)
        for g in range(n):
            i420_host[g], nv12_host[g] = some[g % 4], some_nv12[(g + 1) % 4]   # the two sources differ: a call that did nothing would show
        nv12_dev = torch.from_numpy(nv12_host).to("cuda:0")
        torch.cuda.synchronize()
        assert nv12_dev.data_ptr() % 16 == 0 and W % 16 == 0 and (W * H) % 16 == 0 and fb % 16 == 0   # read in place
        row = {"case": name, "grid": f"{cols}x{rows}", "res": f"{W}x{H}", "images": n, "runs": runs, "warm": warm}
        for ctx in (full, lean):
            ctx.set_grid(cols, rows, W, H)
            ctx.set_stream(stream.cuda_stream)
            ctx.upload_images_yuv(ctx.yuv_surfaces_packed("i420", "host", i420_host.ctypes.data, keep=i420_host), n)
            ctx.set_params(hp)
            ctx.prepare("TEN_WM")
            ctx.sync()
        info = full.memory_info()
        row["before_input_bytes"], row["before_derived_bytes"] = info.grid_bytes, info.derived_bytes
        lean.release_inputs()
        info = lean.memory_info()
        row["after_input_bytes"], row["after_derived_bytes"] = info.grid_bytes, info.derived_bytes
        assert full.derived_layout() == lean.derived_layout()
        sources = {}
        for ctx, tag in ((full, "a"), (lean, "b")):
            sources[tag] = {"device_nv12": ctx.yuv_surfaces_packed("nv12", "device", nv12_dev.data_ptr(), keep=nv12_dev),
                            "host_i420": ctx.yuv_surfaces_packed("i420", "host", i420_host.ctypes.data, keep=i420_host)}

        def step_a(source):
            full.upload_images_yuv(sources["a"][source], n)
            full.prepare("TEN_WM")   # joins the upload and rebuilds the changed images' planes, as the next render would

        def step_b(source):
            lean.upload_images_yuv_derived(sources["b"][source], n)
            lean.prepare("TEN_WM")   # joins the upload; the copy is valid as it is

        def timed(fn, source):
            ms = []
            for k in range(warm + runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn(source)
                e1.record(stream)
                e1.synchronize()
                if k >= warm:
                    ms.append(e0.elapsed_time(e1))
            return round(float(np.median(ms)), 4)

        for source in ("device_nv12", "host_i420"):
            step_a(source)
            step_b(source)
            full.sync(), lean.sync()
            for g in (0, n - 1):
                assert (full.download_derived(g, 1) == lean.download_derived(g, 1)).all(), (name, source, g)
            row[f"a_{source}_ms"] = timed(step_a, source)
            row[f"b_{source}_ms"] = timed(step_b, source)
            row[f"b_over_a_{source}"] = round(row[f"b_{source}_ms"] / row[f"a_{source}_ms"], 4)
        row["model_b_over_a_device"] = round(4.5 / 12.5, 4)
        row["condition_b_not_slower_device"] = bool(row["b_over_a_device_nv12"] <= 1.0)
        # the whole step over the bytes the single pass has to move, 4.5 per pixel and image; the kernel's own time comes from the trace
        row["b_device_step_GBps"] = round(n * W * H * 4.5 / row["b_device_nv12_ms"] / 1e6, 1)
        row["b_device_step_fraction_of_hbm_peak"] = round(row["b_device_step_GBps"] / HBM_PEAK_GBPS, 4)
        print(json.dumps(row), flush=True)
    del nv12_dev
