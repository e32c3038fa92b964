"""Lean mosaic input (lfi_upload_mosaic_yuv_derived, csrc/hip/yuv_mosaic_derived.hpp): what a time step of a one-stream camera array costs on
the input side when the mosaic goes straight into the planar copy, against what the same bytes cost the other ways.  Per case and source, in
ONE process, on the same frame, two contexts with the same parameters — `full` holds its RGBA planes, `lean` released them — and four sides
ALTERNATED run by run:
  mosaic     lean: one lfi_upload_mosaic_yuv_derived of the frame                                              — the new call
  yardstick  lean: one lfi_upload_images_yuv_derived of the same tiles as n separate frames: the same bytes, the same arithmetic
  two_pass   full: lfi_upload_mosaic_yuv plus the rebuild of the copy inside the next render (lfi_prepare brings the copy up to date exactly as
             that render would, and renders nothing), as tools/yuv_derived_time.py measures its two-pass side  — the step the call replaces
  per_tile   lean: n lfi_upload_images_yuv_derived calls of one tile each over descriptors into the frame — what a lean context had before:
             in place where the tile's origin is a multiple of 16 in every plane, staged otherwise
each followed by lfi_prepare, which orders the compute stream after the copy stream.  The contexts compute on a torch stream (lfi_set_stream)
and torch events on that stream bracket a step: device time from the moment the stream reaches the step to the moment the copy is ready for a
render.  `rounds` rounds of `runs` timed steps per side after `warm` warm-ups each; a side's figure is the median of a round, reported per
round, and the median of those; the yardstick's run-to-run spread is the range of its round medians.  Before anything is timed the four
copies are held against each other, byte for byte, and both layouts against each other.
Sources: a device NV12 frame read in place (pitch rounded up to 16) and a page-locked host I420 frame (tight).
Cases: 8 x 8 cameras of 1920 x 1080 in a 15360 x 8640 frame (the aligned kernel) and a 5 x 9 quilt of 1638 x 910 tiles (the unaligned one).
The process ends itself after `limit` seconds (SIGALRM), whatever it is doing.  Reads nothing but the package.
usage: python tools/mosaic_derived_time.py [runs=20] [warm=3] [rounds=5] [limit=420] [case[:source] ...]
       cases: 8x8_1080p, 45_1638x910; sources: device_nv12, host_i420 (default: both cases from the device, 8x8_1080p from the host)"""
import json
import signal
import sys

sys.path.insert(0, ".")
import numpy as np
import torch

import lfinterpolator_amd as L

CASES = {
    # name: tiles_x, tiles_y, W, H, order
    "8x8_1080p": (8, 8, 1920, 1080, "grid"),
    "45_1638x910": (5, 9, 1638, 910, "rows"),
}
VIEWS = 8

args = sys.argv[1:]
runs = int(args[0]) if args else 20
warm = int(args[1]) if len(args) > 1 else 3
rounds = int(args[2]) if len(args) > 2 else 5
limit = int(args[3]) if len(args) > 3 else 420
wanted = args[4:] or ["8x8_1080p:device_nv12", "45_1638x910:device_nv12", "8x8_1080p:host_i420"]
signal.alarm(limit)


def up16(v):
    return (v + 15) // 16 * 16


for item in wanted:
    name, _, source = item.partition(":")
    source = source or "device_nv12"
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
    hp = L.build_params(cols, rows, W, H, "0,0.5,1,0.5", 0.1, 0.0, 3.0, 1.0, VIEWS)
    stream = torch.cuda.Stream(device="cuda:0")
    with L.Context(0) as full, L.Context(0) as lean:
        keep = []
        if source == "device_nv12":
            P, p = up16(MW), up16(W)
            # (one row more than the frame: per_tile's descriptors start tx·W bytes into a row, and their last chroma row must end inside the allocation)
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
            base, memory, fmt = d_frame.data_ptr(), "device", "nv12"
            whole = L.YuvSurfaces.make(fmt, memory, base, frame.size, P, MH * P, P)   # (the stride of one frame is not used)
            separate = L.YuvSurfaces.make(fmt, memory, d_own.data_ptr(), own[0].size, p, H * p, p)
            per_tile = [(g, L.YuvSurfaces.make(fmt, memory, base + ty * H * P + tx * W, 0, P, MH * P - ty * H * P + ty * (H // 2) * P, P)) for tx, ty, g in tiles]
            in_place_tiles = sum((tx * W) % 16 == 0 for tx, ty, g in tiles)
        else:
            fb, tb = MW * MH * 3 // 2, W * H * 3 // 2
            frame = full.pinned_empty((fb,))
            frame[:MW * MH] = y.reshape(-1)
            frame[MW * MH:MW * MH * 5 // 4] = cb.reshape(-1)
            frame[MW * MH * 5 // 4:] = cr.reshape(-1)
            own = full.pinned_empty((n, tb))
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
                per_tile.append((g, L.YuvSurfaces.make(fmt, memory, base + y0, 0, MW, c_off + c0 - y0, MW // 2, cr_off + c0 - y0)))
            in_place_tiles = 0
        for ctx in (full, lean):
            ctx.set_grid(cols, rows, W, H)
            ctx.set_stream(stream.cuda_stream)
            ctx.fill_synthetic(7)
            ctx.set_params(hp)
            ctx.prepare("TEN_WM")
            ctx.sync()
        row = {"case": name, "source": source, "tiles": f"{tiles_x}x{tiles_y}", "tile": f"{W}x{H}", "frame": f"{MW}x{MH}", "unaligned": W % 8 != 0,
               "runs": runs, "warm": warm, "rounds": rounds, "per_tile_calls_in_place": int(in_place_tiles), "yuv_bytes": MW * MH * 3 // 2}
        info = full.memory_info()
        row["full_input_bytes"], row["full_derived_bytes"] = info.grid_bytes, info.derived_bytes
        lean.release_inputs()
        info = lean.memory_info()
        row["lean_input_bytes"], row["lean_derived_bytes"] = info.grid_bytes, info.derived_bytes
        assert full.derived_layout() == lean.derived_layout()
        row["planar_bytes_written"] = int(lean.derived_layout().pitch_bytes) * H * 3 * n

        def side_mosaic():
            lean.upload_mosaic_yuv_derived(mosaic, whole)
            lean.prepare("TEN_WM")

        def side_yardstick():
            lean.upload_images_yuv_derived(separate, n)
            lean.prepare("TEN_WM")

        def side_two_pass():
            full.upload_mosaic_yuv(mosaic, whole)
            full.prepare("TEN_WM")   # joins the upload and rebuilds the changed images' planes, as the next render would

        def side_per_tile():
            for g, d in per_tile:
                lean.upload_images_yuv_derived(d, 1, g0=g)
            lean.prepare("TEN_WM")

        sides = {"mosaic": side_mosaic, "yardstick": side_yardstick, "two_pass": side_two_pass, "per_tile": side_per_tile}
        # the four copies, byte for byte: the first and the last image
        copies = {}
        for k, fn in sides.items():
            fn()
            ctx = full if k == "two_pass" else lean
            ctx.sync()
            copies[k] = [ctx.download_derived(g, 1) for g in (0, n - 1)]
        for k in sides:
            assert all((a == b).all() for a, b in zip(copies[k], copies["yardstick"])), (name, source, k)
        assert int(copies["mosaic"][0].max()) > 0
        del copies
        medians = {k: [] for k in sides}
        for r in range(rounds):
            ms = {k: [] for k in sides}
            for i in range(warm + runs):
                for k, fn in sides.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    e1.synchronize()
                    if i >= warm:
                        ms[k].append(e0.elapsed_time(e1))
            for k in sides:
                medians[k].append(round(float(np.median(ms[k])), 4))
        for k in sides:
            row[f"{k}_round_medians_ms"] = medians[k]
            row[f"{k}_ms"] = round(float(np.median(medians[k])), 4)
        row["yardstick_spread_ms"] = round(max(medians["yardstick"]) - min(medians["yardstick"]), 4)
        row["mosaic_over_yardstick"] = round(row["mosaic_ms"] / row["yardstick_ms"], 4)
        row["mosaic_minus_yardstick_ms"] = round(row["mosaic_ms"] - row["yardstick_ms"], 4)
        row["mosaic_over_two_pass"] = round(row["mosaic_ms"] / row["two_pass_ms"], 4)
        row["mosaic_over_per_tile"] = round(row["mosaic_ms"] / row["per_tile_ms"], 4)
        row["model_mosaic_over_two_pass"] = round(4.5 / 12.5, 4)
        row["mosaic_GBps_moved"] = round((row["yuv_bytes"] + row["planar_bytes_written"]) / row["mosaic_ms"] / 1e6, 1)
        row["lean_workspace_bytes"] = int(lean.memory_info().workspace_bytes)
        print(json.dumps(row), flush=True)
        del keep
signal.alarm(0)
