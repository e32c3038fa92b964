"""10-bit video surfaces (LFI_YUV_I010, LFI_YUV_P010): what the 10-bit kernels cost beside the 8-bit ones.  Per case, in ONE process on one
context, the two depths ALTERNATING call by call (8, 10, 8, 10, …: whatever drifts, drifts for both), medians of `runs` device-event times
after `warm` warm-ups: the context computes on a torch stream (lfi_set_stream) and torch events on that stream bracket a call.
  convert   lfi_download_views_yuv of 64 views into device surfaces written in place (no copy, ONE launch): RGBA and planar views, the
            semi-planar pair NV12 / P010 and the planar pair I420 / I010, centre- and left-sited.  The views are attached device memory holding
            random bytes.  The yardstick is the 8-bit time times the ratio of bytes moved: (4 + 3)/(4 + 1.5) from RGBA views,
            (3 + 3)/(3 + 1.5) from planar views.
  expand    lfi_upload_images_yuv of 16 frames from device surfaces read in place (no copy, ONE launch) + lfi_upload_wait, bilinear, both
            pairs, both sitings; the yardstick is the 8-bit time times (3 + 4)/(1.5 + 4).  The event pair brackets the host wait too: a few
            microseconds, the same for both depths.
Each row carries both medians, both spreads (min, max), the ratio and the yardstick.  Before anything is timed the first and last frame
(image) of each 10-bit call are held against the numpy restatement (tests/yuv10_ref.py).  Reads nothing but the package and tests/.
usage: python tools/yuv10_time.py [runs=20] [warm=3] [case ...]   cases: 1080p, 4k (default: both)"""
import json
import sys

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np
import torch

import lfinterpolator_amd as L
import yuv10_ref as ref

CASES = {"1080p": (1920, 1080), "4k": (3840, 2160)}
VIEWS, FRAMES = 64, 16
PAIRS = {"semi_planar": ("nv12", "p010"), "planar": ("i420", "i010")}
SITINGS = ("centre", "left")
REF_FMT = {"p010": ref.P010, "i010": ref.I010}

args = sys.argv[1:]
runs = int(args[0]) if args else 20
warm = int(args[1]) if len(args) > 1 else 3
names = args[2:] or list(CASES)


def alternate(stream, calls):
    """{key: [ms]}: the calls in turn, warm + runs rounds, each bracketed by events on the stream"""
    ms = {k: [] for k in calls}
    for r in range(warm + runs):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if r >= warm:
                ms[k].append(e0.elapsed_time(e1))
    return ms


def report(row, ms, model):
    for k in ("8", "10"):
        row[f"ms_{k}"] = round(float(np.median(ms[k])), 4)
        row[f"min_{k}"], row[f"max_{k}"] = round(min(ms[k]), 4), round(max(ms[k]), 4)
    row["ratio"] = round(row["ms_10"] / row["ms_8"], 4)
    row["yardstick_ratio"] = round(model, 4)
    row["yardstick_ms"] = round(row["ms_8"] * model, 4)
    row["spread_8_ms"] = round(row["max_8"] - row["min_8"], 4)
    row["above_yardstick_by_more_than_spread"] = bool(row["ms_10"] > row["yardstick_ms"] + row["spread_8_ms"])
    print(json.dumps(row), flush=True)


for name in names:
    W, H = CASES[name]
    stream = torch.cuda.Stream(device="cuda:0")
    samples = ref.sizes(W, H)[2]
    # ---- convert: 64 attached views -> device surfaces in place
    for layout in ("rgba", "planar"):
        with L.Context(0) as ctx:
            ctx.set_grid(2, 2, W, H)
            ctx.set_params(L.build_params(2, 2, W, H, "0,0,1,1", 0.2, 0.0, 3.0, 1.0, VIEWS))
            ctx.set_output_layout(layout)
            ctx.set_stream(stream.cuda_stream)
            vl = ctx.view_layout()
            gen = torch.Generator(device="cuda:0").manual_seed(7)
            views = torch.randint(0, 256, (VIEWS * vl.view_stride_bytes,), dtype=torch.uint8, device="cuda:0", generator=gen)
            out8 = torch.zeros((VIEWS, samples), dtype=torch.uint8, device="cuda:0")
            out10 = torch.zeros((VIEWS, 2 * samples), dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            ctx.attach_views(views.data_ptr(), views.numel())
            assert out8.data_ptr() % 16 == 0 and out10.data_ptr() % 16 == 0 and W % 16 == 0 and samples % 16 == 0   # written in place
            before = ctx.memory_info().workspace_bytes
            for pair, (f8, f10) in PAIRS.items():
                s8 = ctx.yuv_surfaces_packed(f8, "device", out8.data_ptr(), keep=out8)
                s10 = ctx.yuv_surfaces_packed(f10, "device", out10.data_ptr(), keep=out10)
                for siting in SITINGS:
                    ctx.set_yuv_siting("centre", siting)
                    ctx.download_views_yuv(s10, VIEWS)
                    torch.cuda.synchronize()
                    lay = ref.tight(REF_FMT[f10], W, H)
                    for v in (0, VIEWS - 1):
                        raw = views[v * vl.view_stride_bytes:(v + 1) * vl.view_stride_bytes].cpu().numpy()
                        if layout == "planar":
                            rgb = raw.reshape(3, H, vl.row_pitch_bytes)[:, :, :W].transpose(1, 2, 0)
                        else:
                            rgb = raw.reshape(H, W, 4)
                        want = ref.codes(rgb, ref.BT709, ref.LIMITED, ref.LEFT if siting == "left" else ref.CENTRE)
                        assert (ref.gather(out10[v:v + 1].cpu().numpy(), lay)[0] == ref.words(want, lay.fmt)).all(), (name, layout, f10, siting, v)
                    ms = alternate(stream, {"8": lambda: ctx.download_views_yuv(s8, VIEWS), "10": lambda: ctx.download_views_yuv(s10, VIEWS)})
                    report({"what": "convert", "case": name, "views": VIEWS, "layout": layout, "formats": f"{f8}/{f10}", "siting": siting, "runs": runs, "warm": warm},
                           ms, 7 / 5.5 if layout == "rgba" else 6 / 4.5)
            assert ctx.memory_info().workspace_bytes == before   # no device frames of the context's own
        del views, out8, out10
    # ---- expand: 16 frames read in place -> the RGBA grid
    with L.Context(0) as ctx:
        ctx.set_grid(4, 4, W, H)
        ctx.set_stream(stream.cuda_stream)
        grid = torch.zeros((FRAMES, H, W, 4), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ctx.attach_grid(grid.data_ptr(), grid.numel())
        rng = np.random.default_rng(7)
        codes = rng.integers(0, 1024, (2, samples), dtype=np.uint16)
        bytes8 = rng.integers(0, 256, (FRAMES, samples), dtype=np.uint8)
        in8 = torch.from_numpy(bytes8).to("cuda:0")
        before = ctx.memory_info().workspace_bytes
        for pair, (f8, f10) in PAIRS.items():
            lay = ref.tight(REF_FMT[f10], W, H)
            two = ref.scatter(codes, lay, 0)
            in10 = torch.from_numpy(np.concatenate([two] * (FRAMES // 2))).to("cuda:0")
            torch.cuda.synchronize()
            assert in8.data_ptr() % 16 == 0 and in10.data_ptr() % 16 == 0
            s8 = ctx.yuv_surfaces_packed(f8, "device", in8.data_ptr(), keep=in8)
            s10 = ctx.yuv_surfaces_packed(f10, "device", in10.data_ptr(), keep=in10)

            def up(s):
                ctx.upload_images_yuv(s, FRAMES)
                ctx.upload_wait()

            for siting in SITINGS:
                ctx.set_yuv_siting(siting, "centre")
                up(s10)
                torch.cuda.synchronize()
                for g in (0, FRAMES - 1):
                    want = ref.rgba(codes[g % 2], W, H, ref.BT709, ref.LIMITED, ref.BILINEAR, ref.LEFT if siting == "left" else ref.CENTRE)
                    assert (grid[g].cpu().numpy() == want).all(), (name, f10, siting, g)
                ms = alternate(stream, {"8": lambda: up(s8), "10": lambda: up(s10)})
                report({"what": "expand", "case": name, "frames": FRAMES, "formats": f"{f8}/{f10}", "siting": siting, "filter": "bilinear", "runs": runs, "warm": warm},
                       ms, 7 / 5.5)
            del in10
        assert ctx.memory_info().workspace_bytes == before   # no staging buffer
    del grid, in8
