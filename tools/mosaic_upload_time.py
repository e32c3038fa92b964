"""Mosaic input (lfi_upload_mosaic_yuv, csrc/hip/yuv_mosaic.hpp): what splitting ONE frame on the device costs against the two ways the same
bytes could go in before it existed.  Per case and source, in ONE process on one context, the three are ALTERNATED run by run and the medians
of `runs` timed repetitions after `warm` warm-ups are reported, from device events (lfi_timer_start … lfi_timer_stop around the call(s) and
their lfi_upload_wait: the events lie on the compute stream, which the copy stream's work is ordered into; the region holds one host
synchronise, the same for all three) and from the host clock:
  mosaic  one lfi_upload_mosaic_yuv of the frame;
  (a)     N lfi_upload_images_yuv calls of n = 1 over per-tile descriptors into the same frame (base at the tile's Y origin, the frame's pitch,
          c_offset the distance to the tile's chroma origin) — in place only where the tile's origin is a multiple of 16;
  (b)     one lfi_upload_images_yuv of the N tiles as N separate frames: the same bytes, the same arithmetic — the yardstick.
Sources: a device NV12 frame read in place (pitches rounded up to 16), and a page-locked host I420 frame (tight).
Cases: 8 x 8 cameras of 1920 x 1080 in a 15360 x 8640 frame (the aligned path) and a 5 x 9 quilt of 1638 x 910 tiles (the unaligned path).
Before anything is timed the three grids are held against each other, byte for byte.  (b)'s spread is its own max − min over the runs.
usage: python tools/mosaic_upload_time.py [runs=20] [warm=3] [case ...]   cases: 8x8_1080p, 45_1638x910 (default: both)"""
import json
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

import lfinterpolator_amd as L

CASES = {
    # name: tiles_x, tiles_y, W, H, order
    "8x8_1080p": (8, 8, 1920, 1080, "grid"),
    "45_1638x910": (5, 9, 1638, 910, "rows"),
}

args = sys.argv[1:]
runs = int(args[0]) if args else 20
warm = int(args[1]) if len(args) > 1 else 3
names = args[2:] or list(CASES)


def up16(v):
    return (v + 15) // 16 * 16


def alternate(ctx, fns):
    """{name: (device ms per run, host ms per run)} of the functions, taken in turn; each ends with lfi_upload_wait"""
    out = {k: ([], []) for k in fns}
    for i in range(warm + runs):
        for k, fn in fns.items():
            ctx.sync()
            t0 = time.perf_counter()
            ctx.timer_start()
            fn()
            dev = ctx.timer_stop()
            host = (time.perf_counter() - t0) * 1e3
            if i >= warm:
                out[k][0].append(dev)
                out[k][1].append(host)
    return out


for name in names:
    tiles_x, tiles_y, W, H, order = CASES[name]
    n = tiles_x * tiles_y
    MW, MH = tiles_x * W, tiles_y * H
    cols, rows = (tiles_x, tiles_y) if order == "grid" else (n, 1)
    mosaic = L.Mosaic.make(tiles_x, tiles_y, order)
    tiles = [tuple(int(v) for v in t) for t in L.abi.mosaic_map(mosaic, cols, rows)]   # per tile: tx, ty, g
    rng = np.random.default_rng(7)
    y = rng.integers(0, 256, (MH, MW), dtype=np.uint8)
    cb = rng.integers(0, 256, (MH // 2, MW // 2), dtype=np.uint8)
    cr = rng.integers(0, 256, (MH // 2, MW // 2), dtype=np.uint8)
    with L.Context(0) as ctx:
        ctx.set_grid(cols, rows, W, H)
        grid = torch.zeros((n, H, W, 4), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ctx.attach_grid(grid.data_ptr(), grid.numel())

        def result():
            ctx.upload_wait()
            ctx.sync()
            torch.cuda.synchronize()
            out = grid.clone()
            grid.zero_()
            torch.cuda.synchronize()
            return out

        for source in ("device_nv12_in_place", "host_i420_pinned"):
            keep = []
            if source == "device_nv12_in_place":
                # the frame: NV12, pitch a multiple of 16; (b)'s frames: NV12 of W x H each, pitch and stride multiples of 16
                P, p = up16(MW), up16(W)
                # (one row more than the frame: (a)'s descriptors start tx·W bytes into a row, and their last chroma row must end inside the allocation)
                frame = np.zeros((MH * 3 // 2 + 1, P), np.uint8)
                frame[:MH, :MW] = y
                frame[MH:MH * 3 // 2, 0:MW:2], frame[MH:MH * 3 // 2, 1:MW:2] = cb, cr
                own = np.zeros((n, H * 3 // 2, p), np.uint8)
                for tx, ty, g in tiles:
                    own[g, :H, :W] = frame[ty * H:(ty + 1) * H, tx * W:(tx + 1) * W]
                    own[g, H:, :W] = frame[MH + ty * H // 2:MH + (ty + 1) * H // 2, tx * W:(tx + 1) * W]
                d_frame, d_own = torch.from_numpy(frame).to("cuda:0"), torch.from_numpy(own).to("cuda:0")
                torch.cuda.synchronize()
                keep += [d_frame, d_own]
                base, own_base, memory, fmt = d_frame.data_ptr(), d_own.data_ptr(), "device", "nv12"
                whole = L.YuvSurfaces.make(fmt, memory, base, frame.size, P, MH * P, P)   # (the stride of one frame is not used)
                separate = L.YuvSurfaces.make(fmt, memory, own_base, own[0].size, p, H * p, p)
                per_tile = [(int(g), L.YuvSurfaces.make(fmt, memory, base + ty * H * P + tx * W, 0, P, MH * P - ty * H * P + ty * (H // 2) * P, P))
                            for tx, ty, g in tiles]
            else:
                # the frame: tight I420; (b)'s frames: tight I420 of W x H each
                fb, tb = MW * MH * 3 // 2, W * H * 3 // 2
                frame = ctx.pinned_empty((fb,))
                frame[:MW * MH] = y.reshape(-1)
                frame[MW * MH:MW * MH * 5 // 4] = cb.reshape(-1)
                frame[MW * MH * 5 // 4:] = cr.reshape(-1)
                own = ctx.pinned_empty((n, tb))
                for tx, ty, g in tiles:
                    own[g, :W * H] = y[ty * H:(ty + 1) * H, tx * W:(tx + 1) * W].reshape(-1)
                    own[g, W * H:W * H * 5 // 4] = cb[ty * H // 2:(ty + 1) * H // 2, tx * W // 2:(tx + 1) * W // 2].reshape(-1)
                    own[g, W * H * 5 // 4:] = cr[ty * H // 2:(ty + 1) * H // 2, tx * W // 2:(tx + 1) * W // 2].reshape(-1)
                base, memory, fmt = frame.ctypes.data, "host", "i420"
                c_off, cr_off = MW * MH, MW * MH * 5 // 4
                whole = L.YuvSurfaces.make(fmt, memory, base, fb, MW, c_off, MW // 2, cr_off)
                separate = L.YuvSurfaces.make(fmt, memory, own.ctypes.data, tb, W, W * H, W // 2, W * H * 5 // 4)
                per_tile = []
                for tx, ty, g in tiles:
                    y0, c0 = ty * H * MW + tx * W, ty * (H // 2) * (MW // 2) + tx * W // 2
                    per_tile.append((int(g), L.YuvSurfaces.make(fmt, memory, base + y0, 0, MW, c_off + c0 - y0, MW // 2, cr_off + c0 - y0)))

            def one_mosaic():
                ctx.upload_mosaic_yuv(mosaic, whole)
                ctx.upload_wait()

            def n_calls():
                for g, d in per_tile:
                    ctx.upload_images_yuv(d, 1, g0=g)
                ctx.upload_wait()

            def one_call():
                ctx.upload_images_yuv(separate, n)
                ctx.upload_wait()

            fns = {"mosaic": one_mosaic, "a_n_calls": n_calls, "b_one_call": one_call}
            grids = {}
            for k, fn in fns.items():
                fn()
                grids[k] = result()
            assert int(grids["b_one_call"].max()) > 0
            assert torch.equal(grids["mosaic"], grids["b_one_call"]) and torch.equal(grids["a_n_calls"], grids["b_one_call"]), (name, source)
            del grids
            times = alternate(ctx, fns)
            row = {"case": name, "source": source, "tiles": f"{tiles_x}x{tiles_y}", "tile": f"{W}x{H}", "frame": f"{MW}x{MH}", "unaligned": W % 8 != 0,
                   "runs": runs, "warm": warm, "yuv_bytes": MW * MH * 3 // 2, "rgba_bytes": n * W * H * 4}
            for k, (dev, host) in times.items():
                row[f"{k}_device_ms"] = round(float(np.median(dev)), 4)
                row[f"{k}_device_min_max_ms"] = [round(min(dev), 4), round(max(dev), 4)]
                row[f"{k}_host_ms"] = round(float(np.median(host)), 4)
            spread = row["b_one_call_device_min_max_ms"][1] - row["b_one_call_device_min_max_ms"][0]
            row["b_spread_ms"] = round(spread, 4)
            row["mosaic_over_b"] = round(row["mosaic_device_ms"] / row["b_one_call_device_ms"], 4)
            row["mosaic_over_a"] = round(row["mosaic_device_ms"] / row["a_n_calls_device_ms"], 4)
            row["mosaic_exceeds_b_by_more_than_its_spread"] = bool(row["mosaic_device_ms"] > row["b_one_call_device_ms"] + spread)
            row["mosaic_GBps_moved"] = round((row["yuv_bytes"] + row["rgba_bytes"]) / row["mosaic_device_ms"] / 1e6, 1)
            row["workspace_bytes"] = int(ctx.memory_info().workspace_bytes)
            print(json.dumps(row), flush=True)
            del keep
        del grid
