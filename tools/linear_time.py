"""Linear-light blending (LFI_FLAG_LINEAR_LIGHT): what the decode lookups and the encoding epilogue cost, against the launches they stand beside.
In ONE process, contexts over the same synthetic grid are timed alternately, launch by launch: per side and round the median of `runs` device-event
times (lfi_timer_start / lfi_timer_stop around one launch) after `warm` warm-up rounds of all sides; `rounds` such rounds, and the spread of their
medians.  Planar view layout on every side, every copy prepared (lfi_prepare): a timed render is only a launch.  Per case:
  linear TEN_WM, linear STD   blend_linear
  deep TEN_WM, deep STD       deep_blend, the sibling on the same skeleton without the tables (it writes 3x the bytes per view): the ratio of
                              blend_linear to the deep_blend of the same method is the price of the lookups and of E
  p3                          the flag-free TEN_WM launch (blend_p3)
Writes one JSON line per row to stdout and, with out=PATH, the same rows as a markdown table to PATH.  Reads nothing but the package.
usage: python tools/linear_time.py [runs=20] [warm=3] [rounds=5] [out=PATH] [case ...]   cases: 1080p, 4k (default: both)"""
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
runs, warm, rounds, out_path, names = 20, 3, 5, None, []
for arg in sys.argv[1:]:
    if arg.startswith("runs="):
        runs = int(arg[5:])
    elif arg.startswith("warm="):
        warm = int(arg[5:])
    elif arg.startswith("rounds="):
        rounds = int(arg[7:])
    elif arg.startswith("out="):
        out_path = arg[4:]
    else:
        names.append(arg)
names = names or list(CASES)
rows_out = []


def alternate(sides):
    """sides: [(label, ctx, fn)]; one launch of each in turn, `warm` rounds untimed, `runs` timed: {label: median ms}"""
    times = {label: [] for label, _, _ in sides}
    for r in range(warm + runs):
        for label, ctx, fn in sides:
            ctx.timer_start()
            fn()
            ms = ctx.timer_stop()
            if r >= warm:
                times[label].append(ms)
    return {k: float(np.median(v)) for k, v in times.items()}


def context(cols, rows, W, H, hp, flags, method):
    ctx = L.Context(0)
    ctx.set_grid(cols, rows, W, H)
    ctx.fill_synthetic(0x1F1F)
    ctx.set_output_layout("planar")
    ctx.set_params(hp, flags=flags)
    ctx.prepare(method)
    return ctx


SIDES = [("linear TEN_WM", L.LFI_FLAG_LINEAR_LIGHT, "TEN_WM"), ("linear STD", L.LFI_FLAG_LINEAR_LIGHT, "STD"), ("p3", 0, "TEN_WM"),
         ("deep TEN_WM", L.LFI_FLAG_DEEP_VIEWS, "TEN_WM"), ("deep STD", L.LFI_FLAG_DEEP_VIEWS, "STD")]

for name in names:
    cols, rows, W, H, traj, f, aspect, V = CASES[name]
    hp = L.build_params(cols, rows, W, H, traj, f, 0.0, 3.0, aspect, V)
    ctxs = {label: (context(cols, rows, W, H, hp, flags, method), method) for label, flags, method in SIDES}
    medians = {label: [] for label in ctxs}
    for _ in range(rounds):
        t = alternate([(label, c, (lambda c=c, m=m: c.render(m))) for label, (c, m) in ctxs.items()])
        for label, ms in t.items():
            medians[label].append(ms)
    mid = {label: float(np.median(v)) for label, v in medians.items()}
    for label, (c, method) in ctxs.items():
        row = {"case": name, "side": label, "kernel": c.last_kernel_name(), "median_ms": round(mid[label], 4), "round_medians_ms": [round(x, 4) for x in medians[label]],
               "spread": round((max(medians[label]) - min(medians[label])) / mid[label], 4), "ratio_to_p3": round(mid[label] / mid["p3"], 3)}
        if label.startswith("linear"):
            row["ratio_to_deep"] = round(mid[label] / mid["deep " + method], 3)
        rows_out.append(row)
        print(json.dumps(row), flush=True)
    for c, _ in ctxs.values():
        c.close()

if out_path:
    with open(out_path, "w") as fh:
        fh.write("| case | side | kernel | median ms | medians of the rounds | spread | ratio to deep_blend of its method | ratio to blend_p3 |\n|---|---|---|---|---|---|---|---|\n")
        for r in rows_out:
            fh.write(f"| {r['case']} | {r['side']} | `{r['kernel']}` | {r['median_ms']} | {r['round_medians_ms']} | {r['spread']} | {r.get('ratio_to_deep', '')} | {r['ratio_to_p3']} |\n")
        fh.write(f"\nper side and round the median of {runs} device-event times, the sides alternating launch by launch in one process, {warm} warm-up rounds; "
                 f"{rounds} rounds; spread = (largest - smallest round median) / their median\n")
