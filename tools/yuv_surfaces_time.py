"""Video surfaces (lfi_upload_images_yuv, lfi_download_views_yuv): what device-resident NV12 frames save, and what NV12 and pitches cost.
Per case, in ONE process on one context (its grid a torch tensor attached with lfi_attach_grid, so that the result can be read back), medians
of `runs` timed repetitions after `warm` warm-ups, host clock, host sides from page-locked memory (lfi_alloc_pinned):
  (a) one time step: lfi_upload_images_yuv + lfi_upload_wait from host I420 surfaces (frames that cross PCIe, the yardstick;
      lfi_upload_images_yuv420 is this call on a packed descriptor) against the same from NV12 device surfaces read in place;
  (b) host NV12 against host I420 through lfi_upload_images_yuv / lfi_download_views_yuv, both directions, and lfi_download_views_yuv into
      NV12 device surfaces written in place;
  (c) the kernels alone come from a SECOND run of this tool under
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/yuv_surfaces_time.py 3 1
      and  python tools/yuv_surfaces_time.py --kernels DIR/…_kernel_trace.csv
      which prints, per kernel and grid of launches, the number of launches and the median of End_Timestamp − Start_Timestamp (device clock).
Before anything is timed the grid's first and last image after the device call are held against the numpy restatement of the definition, and
the downloaded NV12 frames against the I420 ones.  Reads nothing but the package and tests/.
usage: python tools/yuv_surfaces_time.py [runs=20] [warm=3] [case ...]   cases: 1080p, 4k (default: both)"""
import csv
import json
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np

CASES = {
    # name: cols, rows, W, H
    "1080p": (8, 8, 1920, 1080),
    "4k": (15, 15, 3840, 2160),
}
VIEWS = 8   # views of the download side

if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
    with open(sys.argv[2], newline="") as f:
        trace = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    groups = {}
    for r in trace:
        name = r["Kernel_Name"].split("(")[0]
        if "yuvs_" not in name:
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


def timed(fn):
    """median host wall ms of fn, which ends with a host wait"""
    for _ in range(warm):
        fn()
    wall = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(wall)), 4)


for name in names:
    cols, rows, W, H = CASES[name]
    n = cols * rows
    fb = ref.sizes(W, H)[2]
    nv12 = sref.tight(sref.NV12, W, H)
    with L.Context(0) as ctx:
        ctx.set_grid(cols, rows, W, H)
        grid = torch.zeros((n, H, W, 4), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ctx.attach_grid(grid.data_ptr(), grid.numel())
        some = np.random.default_rng(7).integers(0, 256, (4, fb), dtype=np.uint8)
        some_nv12 = sref.scatter(some, nv12, 0)
        i420_host, nv12_host = ctx.pinned_empty((n, fb)), ctx.pinned_empty((n, fb))
        for g in range(n):
            i420_host[g], nv12_host[g] = some[g % 4], some_nv12[g % 4]
        nv12_dev = torch.from_numpy(nv12_host).to("cuda:0")
        torch.cuda.synchronize()
        s_i420_host = ctx.yuv_surfaces_packed("i420", "host", i420_host.ctypes.data, keep=i420_host)
        s_nv12_host = ctx.yuv_surfaces_packed("nv12", "host", nv12_host.ctypes.data, keep=nv12_host)
        s_nv12_dev = ctx.yuv_surfaces_packed("nv12", "device", nv12_dev.data_ptr(), keep=nv12_dev)
        assert nv12_dev.data_ptr() % 16 == 0 and W % 16 == 0 and (W * H) % 16 == 0 and fb % 16 == 0   # read in place
        row = {"case": name, "grid": f"{cols}x{rows}", "res": f"{W}x{H}", "images": n, "runs": runs, "warm": warm, "yuv_bytes": n * fb}

        def wait(fn):
            def call():
                fn()
                ctx.upload_wait()
            return call

        up = {
            "up_device_nv12_in_place_ms": wait(lambda: ctx.upload_images_yuv(s_nv12_dev, n)),
            "up_host_i420_surfaces_ms": wait(lambda: ctx.upload_images_yuv(s_i420_host, n)),          # the yardstick
            "up_host_nv12_surfaces_ms": wait(lambda: ctx.upload_images_yuv(s_nv12_host, n)),
        }
        before = ctx.memory_info().workspace_bytes
        up["up_device_nv12_in_place_ms"]()
        assert ctx.memory_info().workspace_bytes == before   # no staging buffer
        torch.cuda.synchronize()
        for g in (0, n - 1):
            assert (grid[g].cpu().numpy() == ref.rgba(i420_host[g], W, H, ref.BT709, ref.LIMITED, ref.BILINEAR)).all(), (name, g)
        for key, fn in up.items():
            row[key] = timed(fn)
        row["device_over_host"] = round(row["up_device_nv12_in_place_ms"] / row["up_host_i420_surfaces_ms"], 4)
        row["condition_device_below_host"] = bool(row["up_device_nv12_in_place_ms"] < row["up_host_i420_surfaces_ms"])
        row["host_GBps"] = round(n * fb / row["up_host_i420_surfaces_ms"] / 1e6, 1)
        row["device_read_write_GBps"] = round(n * W * H * 5.5 / row["up_device_nv12_in_place_ms"] / 1e6, 1)
        print(json.dumps(row), flush=True)

        # the download side: VIEWS views of one render
        ctx.set_params(L.build_params(cols, rows, W, H, "0,0.5,1,0.5", 0.1, 0.0, 3.0, 1.0, VIEWS))
        ctx.render("TEN_WM")
        ctx.sync()
        out_i420, out_nv12 = ctx.pinned_empty((VIEWS, fb)), ctx.pinned_empty((VIEWS, fb))
        out_dev = torch.zeros((VIEWS, fb), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        d_i420_host = ctx.yuv_surfaces_packed("i420", "host", out_i420.ctypes.data, keep=out_i420)
        d_nv12_host = ctx.yuv_surfaces_packed("nv12", "host", out_nv12.ctypes.data, keep=out_nv12)
        d_nv12_dev = ctx.yuv_surfaces_packed("nv12", "device", out_dev.data_ptr(), keep=out_dev)
        down = {
            "down_host_i420_surfaces_ms": lambda: ctx.download_views_yuv(d_i420_host),
            "down_host_nv12_surfaces_ms": lambda: ctx.download_views_yuv(d_nv12_host),
            "down_device_nv12_in_place_ms": lambda: ctx.download_views_yuv(d_nv12_dev),
        }
        for fn in down.values():
            fn()
        torch.cuda.synchronize()
        assert (sref.gather(out_nv12[:1], nv12) == out_i420[:1]).all() and (out_dev.cpu().numpy() == np.asarray(out_nv12)).all()
        row = {"case": name, "views": VIEWS, "yuv_bytes": VIEWS * fb}
        for key, fn in down.items():
            row[key] = timed(fn)
        print(json.dumps(row), flush=True)
    del grid, nv12_dev, out_dev
