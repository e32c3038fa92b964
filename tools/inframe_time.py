"""In-frame blending (LFI_FLAG_IN_FRAME): what leaving out the out-of-frame samples costs, against the launches it stands beside.
In ONE process, contexts over the same synthetic grid — in-frame, flag-free, deep views, and in-frame at focus 0 — are timed alternately, launch
by launch: per side the median of `runs` device-event times (lfi_timer_start / lfi_timer_stop around one launch) after `warm` warm-up rounds of
all sides.  Planar view layout on every side, every copy prepared (lfi_prepare): a timed render is only a launch.  Per case and method:
  plain      the flag-free launch of the same build (TEN_WM: blend_p3; STD: the default band method)
  in-frame   blend_inframe at the case's focus; `interior_tiles` is the share of its 128-pixel tiles that take the unmasked path, counted
             here from the offsets' bounds as the kernel counts them
  deep       deep_blend, the sibling whose skeleton the kernel keeps, which writes 3x the bytes per view
  focus 0    blend_inframe with every offset zero — all tiles interior: what the classification and the second code path cost — against the
             flag-free launch at focus 0
Writes one JSON line per row to stdout and, with out=PATH, the same rows as a markdown table to PATH.  Reads nothing but the package.
usage: python tools/inframe_time.py [runs=20] [warm=3] [out=PATH] [case ...]   cases: 1080p, 4k (default: both)"""
import json
import sys

sys.path.insert(0, ".")
import numpy as np

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


def interior_share(hp, W, H):
    """the share of 128-pixel tiles every image covers, from the bounds of the integer offsets (blend_inframe.hpp border_tile)"""
    o = np.asarray(hp.focused_offsets)
    lo_x, hi_x, lo_y, hi_y = int(o[:, 0].min()), int(o[:, 0].max()), int(o[:, 1].min()), int(o[:, 1].max())
    x0 = np.arange(0, W, 128)
    x1 = np.minimum(x0 + 128, W) - 1
    cols_in = int(((x0 + lo_x >= 0) & (x1 + hi_x < W)).sum())
    y = np.arange(H)
    rows_in = int(((y + lo_y >= 0) & (y + hi_y < H)).sum())
    return cols_in * rows_in / (len(x0) * H), (lo_x, hi_x, lo_y, hi_y)


def report(case, method, label, kernel, t, base=None, **more):
    row = {"case": case, "method": method, "side": label, "kernel": kernel, "median_ms": round(t[0], 4), "min_ms": round(t[1], 4), "max_ms": round(t[2], 4)}
    if base is not None:
        row["ratio_to_plain"] = round(t[0] / base[0], 3)
    row.update(more)
    rows_out.append(row)
    print(json.dumps(row), flush=True)


def context(cols, rows, W, H, hp, flags, method):
    ctx = L.Context(0)
    ctx.set_grid(cols, rows, W, H)
    ctx.fill_synthetic(0x1F1F)
    ctx.set_output_layout("planar")
    ctx.set_params(hp, flags=flags)
    ctx.prepare(method)
    return ctx


for name in names:
    cols, rows, W, H, traj, f, aspect, V = CASES[name]
    hp = L.build_params(cols, rows, W, H, traj, f, 0.0, 3.0, aspect, V)
    hp0 = L.host.HostParams(hp.focused_offsets * 0, hp.offsets, hp.weights, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)
    share, bounds = interior_share(hp, W, H)
    for method in ("TEN_WM", "STD"):
        ctxs = {"plain": context(cols, rows, W, H, hp, 0, method), "in-frame": context(cols, rows, W, H, hp, L.LFI_FLAG_IN_FRAME, method),
                "deep": context(cols, rows, W, H, hp, L.LFI_FLAG_DEEP_VIEWS, method), "plain, focus 0": context(cols, rows, W, H, hp0, 0, method),
                "in-frame, focus 0": context(cols, rows, W, H, hp0, L.LFI_FLAG_IN_FRAME, method)}
        t = alternate([(label, c, (lambda c=c: c.render(method))) for label, c in ctxs.items()])
        # all tiles interior: the flag-free bytes (STD: byte for byte; TEN_WM: the same kernel arithmetic on the same operands)
        assert (ctxs["in-frame, focus 0"].download_view(V // 2) == ctxs["plain, focus 0"].download_view(V // 2)).all()
        kernels = {label: c.last_kernel_name() for label, c in ctxs.items()}
        report(name, method, "plain", kernels["plain"], t["plain"])
        report(name, method, "in-frame", kernels["in-frame"], t["in-frame"], t["plain"], interior_tiles=round(share, 4), offset_bounds=bounds,
               ratio_to_deep=round(t["in-frame"][0] / t["deep"][0], 3))
        report(name, method, "deep", kernels["deep"], t["deep"], t["plain"])
        report(name, method, "plain, focus 0", kernels["plain, focus 0"], t["plain, focus 0"])
        report(name, method, "in-frame, focus 0", kernels["in-frame, focus 0"], t["in-frame, focus 0"], t["plain, focus 0"], interior_tiles=1.0)
        for c in ctxs.values():
            c.close()

if out_path:
    with open(out_path, "w") as fh:
        fh.write("| case | method | side | kernel | median ms | min | max | ratio to its flag-free launch | ratio to deep | interior tiles |\n|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows_out:
            fh.write(f"| {r['case']} | {r['method']} | {r['side']} | `{r['kernel']}` | {r['median_ms']} | {r['min_ms']} | {r['max_ms']} | "
                     f"{r.get('ratio_to_plain', '')} | {r.get('ratio_to_deep', '')} | {r.get('interior_tiles', '')} |\n")
        fh.write(f"\nmedians of {runs} device-event times per side, the sides alternating launch by launch in one process, {warm} warm-up rounds\n")
