"""YUV 4:2:0 input (lfi_upload_images_yuv420): what the device-side expansion costs against the RGBA uploads it replaces.  Per case, in ONE
process on one context (its grid a torch tensor attached with lfi_attach_grid, so that the result can be read back), medians of `runs` timed
repetitions after `warm` warm-ups, host clock, from page-locked host memory (lfi_alloc_pinned):
  (a) N lfi_upload_image_async + lfi_upload_wait of the grid's N RGBA images (existing code, the yardstick) against ONE
      lfi_upload_images_yuv420 + lfi_upload_wait of the same N images as I420 frames;
  (b) the kernel alone comes from a SECOND run of this tool under
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/yuv420_upload_time.py 3 1
      and  python tools/yuv420_upload_time.py --kernels DIR/…_kernel_trace.csv
      which prints, per grid of yuvs_expand launches (the kernel behind the call, csrc/hip/yuv_surfaces.hpp), the number of launches, the
      median of End_Timestamp − Start_Timestamp (device clock), the bytes the kernel moves (1.5 read per pixel, 4 written) and the rate as a
      fraction of 8 TB/s.
Before anything is timed the grid's first and last image after the YUV call are held against the numpy restatement of the definition.
Reads nothing but the package and tests/yuv_in_ref.py.
usage: python tools/yuv420_upload_time.py [runs=20] [warm=3] [case ...]   cases: 1080p, 4k (default: both)"""
import csv
import json
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np

PEAK_BYTES_PER_S = 8e12   # HBM3E, specification
CHUNK = 16                # frames per launch (lfi_upload_images_yuv420: at most 16 frames or 256 MiB)

CASES = {
    # name: cols, rows, W, H
    "1080p": (8, 8, 1920, 1080),
    "4k": (15, 15, 3840, 2160),
}

if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
    with open(sys.argv[2], newline="") as f:
        trace = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    groups = {}
    for r in trace:
        name = r["Kernel_Name"].split("(")[0]
        if "yuvs_expand" not in name:
            continue
        grid = (int(r.get("Grid_Size_X", r.get("Grid_Size", 0))), int(r.get("Grid_Size_Y", 0) or 0), int(r.get("Grid_Size_Z", 0) or 0))
        groups.setdefault((name, grid), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    for (name, grid), ms in groups.items():
        row = {"kernel": name, "grid_threads": "x".join(map(str, grid)), "launches": len(ms), "median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4),
               "max_ms": round(max(ms), 4)}
        # grid = (64·⌈W/512⌉, 4·⌈H/8⌉, frames) threads: the case is the one whose sizes give it
        for case, (_, _, W, H) in CASES.items():
            for per in (1, 64 * 4):   # in workgroups, or in threads
                if grid[0] * grid[1] == per * -(-W // 512) * -(-H // 8):
                    moved = grid[2] * W * H * 5.5
                    row.update(case=case, frames=grid[2], bytes=int(moved), us_at_8TBs=round(moved / PEAK_BYTES_PER_S * 1e6, 1),
                               fraction_of_8TBs=round(moved / (float(np.median(ms)) * 1e-3) / PEAK_BYTES_PER_S, 4))
        print(json.dumps(row), flush=True)
    sys.exit(0)

import torch

import lfinterpolator_amd as L
import yuv_in_ref as ref

args = sys.argv[1:]
runs = int(args[0]) if args else 20
warm = int(args[1]) if len(args) > 1 else 3
names = args[2:] or list(CASES)


def timed(fn):
    """(median host wall ms, all wall ms) of fn, which ends with a host wait"""
    for _ in range(warm):
        fn()
    wall = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(wall)), 4), [round(x, 3) for x in wall]


for name in names:
    cols, rows, W, H = CASES[name]
    n = cols * rows
    fb = ref.sizes(W, H)[2]
    with L.Context(0) as ctx:
        ctx.set_grid(cols, rows, W, H)
        grid = torch.zeros((n, H, W, 4), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ctx.attach_grid(grid.data_ptr(), grid.numel())
        frames = ctx.pinned_empty((n, fb))
        some = np.random.default_rng(7).integers(0, 256, (4, fb), dtype=np.uint8)
        for g in range(n):
            frames[g] = some[g % 4]
        rgba = ctx.pinned_empty((n, H, W, 4))
        rgba[...] = 0x80
        row = {"case": name, "grid": f"{cols}x{rows}", "res": f"{W}x{H}", "images": n, "runs": runs, "warm": warm, "rgba_bytes": n * W * H * 4,
               "yuv_bytes": n * fb, "bytes_ratio": round(fb / (W * H * 4), 4)}

        def yuv():
            ctx.upload_images_yuv420(frames)
            ctx.upload_wait()

        def rgba_uploads():
            for g in range(n):
                ctx.upload_image_async(g, rgba[g])
            ctx.upload_wait()

        yuv()
        torch.cuda.synchronize()
        for g in (0, n - 1):
            assert (grid[g].cpu().numpy() == ref.rgba(frames[g], W, H, ref.BT709, ref.LIMITED, ref.BILINEAR)).all(), (name, g)
        row["rgba_n_calls_ms"], row["reps_rgba"] = timed(rgba_uploads)
        row["yuv_one_call_ms"], row["reps_yuv"] = timed(yuv)
        row["yuv_over_rgba"] = round(row["yuv_one_call_ms"] / row["rgba_n_calls_ms"], 4)
        row["condition_yuv_below_rgba"] = bool(row["yuv_one_call_ms"] < row["rgba_n_calls_ms"])
        row["rgba_GBps"] = round(row["rgba_bytes"] / row["rgba_n_calls_ms"] / 1e6, 1)
        row["yuv_GBps"] = round(row["yuv_bytes"] / row["yuv_one_call_ms"] / 1e6, 1)
        row["launches_per_call"] = -(-n // CHUNK)
        row["workspace_bytes"] = int(ctx.memory_info().workspace_bytes)
        print(json.dumps(row), flush=True)
    del grid
