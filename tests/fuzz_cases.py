"""Randomised parity cases shared by tests/test_gpu_fuzz.py (fixed seeds, a bounded number of cases) and the soak tools under
tools/ (fuzz_parity.py, fuzz_focus.py, fuzz_allfocus.py, fuzz_view_rows.py: any number of cases, any seed).

Every function renders random small shapes through the HIP library (the C-ABI) and checks them against the CPU oracle — STD and
focus maps bit-exact, TEN_WM within one LSB of the fp16-accumulate model M16 and inside the interval of the exact sum
(tests/ten_interval.py) — and returns the list of mismatches (empty = pass).
`L` is the lfinterpolator_amd package, `oc` the oracle binding (oracle/lfi_oracle_c.py): the checker, never the thing measured.
"""
import numpy as np

import poison
import ten_interval
import view_rows

TEN_TOL_LSB = 1


def fuzz_blend(L, oc, n_cases: int, seed: int, log=None) -> list:
    """Fixed-focus renders: random grids (1–225 images), widths around the 128-pixel tile, 1–129 views, every main variant, view
    ranges, and both view layouts."""
    rng = np.random.default_rng(seed)
    ten_variants = ["auto", "persist_m2_nt", "wave_m2_nt"]
    std_variants = ["auto", "persist_m2_nt"]
    bad = []
    for i in range(n_cases):
        cols, rows = int(rng.integers(1, 16)), int(rng.integers(1, 16))
        if cols * rows < 2 or cols * rows > 225:
            cols, rows = 3, 4
        W = int(rng.choice([1, 4, 31, 33, 64, 100, 127, 128, 129, 191, 256, 300, 513, 700]))
        H = int(rng.integers(1, 10))
        V = int(rng.choice([1, 3, 31, 32, 33, 64, 65, 100, 129, 200, 300]))
        focus = float(rng.choice([0.0, 0.03, 0.23, 0.5, 1.1, -0.4]))
        traj = str(rng.choice(["0,0,1,1", "0.071,0.071,0.93,0.93", "1,0,0,1", "0.5,0.5,0.5,0.5", "0.2,0.9,0.8,0.1"]))
        effect = float(rng.choice([1.0, 3.0, 7.0]))
        hp = L.build_params(cols, rows, W, H, traj, focus, 0.0, effect, 1.783, V)
        lf = oc.synthetic_lf(cols * rows, W, H, int(rng.integers(1, 1 << 30)))
        case = dict(kind="blend", cols=cols, rows=rows, W=W, H=H, V=V, focus=focus, traj=traj, effect=effect)
        want_std = oc.blend_std(lf, hp.focused_offsets, hp.offsets, hp.weights, threads=8)
        want_ten = oc.blend_ten(lf, hp.focused_offsets, hp.offsets, hp.weights, model=oc.TEN_M16, threads=8)
        lo, hi = ten_interval.bounds(oc, lf, hp, threads=8)
        ctx = L.Context(0)
        ctx.set_grid(cols, rows, W, H)
        ctx.upload_grid(lf)
        ctx.set_params(hp)
        v0 = int(rng.integers(0, V))
        v1 = int(rng.integers(v0 + 1, V + 1))
        for var in std_variants:
            ctx.set_variant("STD", var)
            poison.render(ctx, "STD")
            if not (ctx.download_views() == want_std).all():
                bad.append(dict(case, what="STD", variant=var))
        for var in ten_variants:
            ctx.set_variant("TEN_WM", var)
            poison.render(ctx, "TEN_WM")
            full = ctx.download_views()
            d = int(np.abs(full.astype(int) - want_ten.astype(int)).max())
            out = ten_interval.outside(full, lo, hi)
            b = poison.render(ctx, "TEN_WM", v0=v0, v1=v1)
            if d > TEN_TOL_LSB or out or poison.written_outside(ctx, v0, v1, b) or not (ctx.download_views(v0, v1) == full[v0:v1]).all():
                bad.append(dict(case, what="TEN_WM", variant=var, lsb=d, outside_interval=out, v0=v0, v1=v1))
        # the planar view layout: TEN_WM within one LSB of the oracle and byte-identical to the RGBA layout's default kernel, view ranges
        # included; STD bit-exact (round 4: blend_stdx writes the byte planes itself, one to four chunks of images), a view range over it too
        ctx.set_variant("TEN_WM", "auto")
        ctx.set_variant("STD", "auto")
        poison.render(ctx, "TEN_WM")
        want_rgba = ctx.download_views()
        ctx.set_output_layout("planar")
        poison.render(ctx, "TEN_WM")
        got = ctx.download_views()
        kernel = ctx.last_kernel_name()
        b = poison.render(ctx, "TEN_WM", v0=v0, v1=v1)
        part_ok = not poison.written_outside(ctx, v0, v1, b) and (ctx.download_views(v0, v1) == got[v0:v1]).all()
        poison.render(ctx, "STD")
        std_ok = (ctx.download_views() == want_std).all()
        b = poison.render(ctx, "STD", v0=v0, v1=v1)
        std_ok = std_ok and not poison.written_outside(ctx, v0, v1, b) and (ctx.download_views(v0, v1) == want_std[v0:v1]).all()
        d = int(np.abs(got.astype(int) - want_ten.astype(int)).max())
        out = ten_interval.outside(got, lo, hi)
        if d > TEN_TOL_LSB or out or not (got == want_rgba).all() or not part_ok or not std_ok:
            bad.append(dict(case, what="planar layout", kernel=kernel, lsb=d, outside_interval=out, v0=v0, v1=v1))
        # round 4: the quilt of a random tiling (assembled on the device, filled in two parts) is the montage of the views; and after
        # lfi_release_inputs — the planar copy is the only copy of the inputs — STD stays the oracle's and TEN_WM the same bytes
        poison.render(ctx, "TEN_WM")
        tx = int(rng.integers(1, 5))
        ty = int(rng.integers(1, max(2, min(4, V // tx) + 1)))
        if tx * ty <= V:
            quilt = poison.sentinel((ty * H, tx * W, 4))
            cut = int(rng.integers(0, tx * ty + 1))
            if cut > 0:
                ctx.download_quilt_tiles(quilt, tx, ty, 0, cut)
            if cut < tx * ty:
                ctx.download_quilt_tiles(quilt, tx, ty, cut, tx * ty - cut, v0=cut)
            montage = got[:tx * ty].reshape(ty, tx, H, W, 4).transpose(0, 2, 1, 3, 4).reshape(ty * H, tx * W, 4)
            if not (quilt == montage).all():
                bad.append(dict(case, what="quilt", tiles=(tx, ty), cut=cut))
        try:
            ctx.release_inputs()
            poison.render(ctx, "TEN_WM")
            same = bool((ctx.download_views() == got).all())
            poison.render(ctx, "STD")
            if not same or not (ctx.download_views() == want_std).all():
                bad.append(dict(case, what="released inputs", ten_same=same))
        except L.LfiError as e:
            if "cannot be built" not in str(e):          # (absurd offsets: the planar copy is refused, and so is the release)
                bad.append(dict(case, what="released inputs", error=str(e)))
        ctx.close()
        if log and (i + 1) % 20 == 0:
            log(f"{i + 1} cases, {len(bad)} mismatches")
    return bad


def fuzz_focus(L, oc, n_cases: int, seed: int, log=None) -> list:
    """Focus maps: the factored estimate, the LDS-staged one and the reference-shaped plain kernel on random shapes, radii, focus
    ranges and contents (quantised and partly black inputs produce ties and FLT_MIN taps) — all against the oracle."""
    rng = np.random.default_rng(seed)
    bad = []
    for i in range(n_cases):
        cols, rows = int(rng.integers(2, 10)), int(rng.integers(2, 10))
        W = int(rng.choice([8, 33, 64, 100, 130, 257, 300, 640]))
        H = int(rng.integers(2, 48))
        focus = float(rng.choice([0.0, 0.05, 0.22, -0.2, 0.6]))
        frange = float(rng.choice([0.01, 0.1, 0.17, 0.5, 1.0]))
        traj = str(rng.choice(["0,0,1,1", "0.071,0.071,0.93,0.93", "0.5,0.5,0.5,0.5"]))
        hp = L.build_params(cols, rows, W, H, traj, focus, frange, 3.0, 1.783, 4)
        if rng.random() < 0.5:
            hp.block_radius = np.array([int(rng.integers(1, 12)), int(rng.integers(1, 6))], np.int32)
        lf = oc.synthetic_lf(cols * rows, W, H, int(rng.integers(1, 1 << 30)))
        q = int(rng.choice([1, 32, 64, 255]))
        lf = (lf // q * q).astype(np.uint8)
        if rng.random() < 0.3:
            lf[:, : H // 2, : W // 3, :3] = 0
        lf[..., 3] = 255
        case = dict(kind="focus", cols=cols, rows=rows, W=W, H=H, focus=focus, range=frange, traj=traj, radius=[int(x) for x in hp.block_radius], q=q)
        want0 = oc.focus_estimate(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, threads=8)
        want1 = oc.focus_filter(want0, hp.block_radius)
        ctx = L.Context(0)
        ctx.set_grid(cols, rows, W, H)
        ctx.upload_grid(lf)
        ctx.set_params(hp)
        for var in ("factored", "factored_direct", "plain", "lds"):
            ctx.set_variant("FOCUS", var)
            poison.focus_map(ctx)
            m0, m1 = ctx.download_map(0), ctx.download_map(1)
            if not ((m0 == want0).all() and (m1 == want1).all()):
                bad.append(dict(case, what="focus map", variant=var, wrong=int((m0 != want0).any(-1).sum())))
        ctx.close()
        if log and (i + 1) % 20 == 0:
            log(f"{i + 1} cases, {len(bad)} mismatches")
    return bad


def fuzz_allfocus(L, oc, n_cases: int, seed: int, log=None) -> list:
    """All-focus renders from random focus maps (noise, constant rows, blocks) on random small shapes, both view layouts."""
    rng = np.random.default_rng(seed)
    bad = []
    for i in range(n_cases):
        cols, rows = int(rng.integers(2, 16)), int(rng.integers(2, 16))
        W = int(rng.choice([17, 64, 100, 128, 129, 200, 257, 300, 520]))
        H = int(rng.integers(2, 12))
        V = int(rng.choice([1, 5, 33, 64, 70]))
        focus = float(rng.choice([0.0, 0.05, 0.3, -0.2]))
        frange = float(rng.choice([0.1, 0.5, 1.2, -0.4]))
        traj = str(rng.choice(["0,0,1,1", "0.071,0.071,0.93,0.93", "0.5,0.5,0.5,0.5"]))
        effect = float(rng.choice([1.0, 3.0, 7.0]))
        hp = L.build_params(cols, rows, W, H, traj, focus, frange, effect, 1.783, V)
        lf = oc.synthetic_lf(cols * rows, W, H, int(rng.integers(1, 1 << 30)))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            lv = rng.integers(0, 256, size=(H, W))
        elif kind == 1:
            lv = np.repeat(rng.integers(0, 256, size=(H, 1)), W, axis=1)
        else:
            lv = np.repeat(np.repeat(rng.integers(0, 256, size=((H + 3) // 4, (W + 89) // 90)), 4, axis=0), 90, axis=1)[:H, :W]
        m = np.repeat(lv[..., None].astype(np.uint8), 4, axis=-1)
        m[..., 3] = 255
        case = dict(kind="allfocus", cols=cols, rows=rows, W=W, H=H, V=V, focus=focus, range=frange, traj=traj, effect=effect, map=kind)
        want_std = oc.blend_std(lf, hp.focused_offsets, hp.offsets, hp.weights, all_focus=True, map_plane=m, focus=hp.focus, rng=hp.range, threads=8)
        want_ten = oc.blend_ten(lf, hp.focused_offsets, hp.offsets, hp.weights, all_focus=True, map_plane=m, focus=hp.focus, rng=hp.range, threads=8)
        lo, hi = ten_interval.bounds(oc, lf, hp, all_focus=True, map_plane=m, focus=hp.focus, rng=hp.range, threads=8)
        ctx = L.Context(0)
        ctx.set_grid(cols, rows, W, H)
        ctx.upload_grid(lf)
        ctx.set_params(hp)
        ctx.upload_map(0, m)
        ctx.upload_map(1, m)
        for layout in ("rgba", "planar"):
            ctx.set_output_layout(layout)
            poison.render(ctx, "STD", all_focus=True)
            ok_std = bool((ctx.download_views() == want_std).all())
            poison.render(ctx, "TEN_WM", all_focus=True)
            got = ctx.download_views()
            d = int(np.abs(got.astype(int) - want_ten.astype(int)).max())
            out = ten_interval.outside(got, lo, hi)
            if not ok_std or d > TEN_TOL_LSB or out:
                bad.append(dict(case, what="all-focus", layout=layout, std_exact=ok_std, lsb=d, outside_interval=out, kernel=ctx.last_kernel_name()))
            if cols * rows > 128 and layout == "rgba":
                # three or four chunks of images: blend_afs (every sample gathered once; round 4) must give the same bytes
                ctx.set_variant("STD", "filtered_gather_once")
                poison.render(ctx, "STD", all_focus=True)
                if ctx.last_kernel_name() != "blend_afs<STD,allfocus>" or not (ctx.download_views() == want_std).all():
                    bad.append(dict(case, what="all-focus", layout=layout, std_exact=False, kernel=ctx.last_kernel_name()))
                ctx.set_variant("STD", "auto")
        ctx.close()
        if log and (i + 1) % 20 == 0:
            log(f"{i + 1} cases, {len(bad)} mismatches")
    return bad


def fuzz_view_rows(L, oc, n_cases: int, seed: int, log=None) -> list:
    """Per-view rows (launch_view_rows: blend_vfocus, blend_vfocus_af): random grids (2–225 images), widths around the 256-pixel tile and
    the 4-pixel quad, 1–9 rows, view counts around the chunk of 8 with a random sub-range, integer rows from either source, float rows
    with the context's maps or a map pair per view, both view layouts, focus ramps of either sign.  Both methods: views outside the range
    keep the poison, the kernel is the one expected, STD byte for byte, TEN_WM within one LSB of M16 and inside the interval of the exact sum."""
    rng = np.random.default_rng(seed)
    bad = []
    for i in range(n_cases):
        cols, rows = int(rng.integers(1, 16)), int(rng.integers(1, 16))
        if cols * rows < 2:
            cols, rows = 3, 4
        n = cols * rows
        W = int(rng.choice([1, 4, 33, 255, 256, 257, 259, 300, 513]))
        H = int(rng.integers(1, 10))
        V = int(rng.choice([1, 7, 8, 9, 64, 65]))
        v0 = int(rng.integers(0, V))
        v1 = int(rng.integers(v0 + 1, V + 1))
        kind = str(rng.choice(view_rows.KINDS))
        source = str(rng.choice(["planar", "rgba"])) if kind == "int" else ""
        layout = str(rng.choice(["rgba", "planar"]))
        f0, f1 = (float(x) for x in rng.choice([0.0, 0.03, 0.23, 0.6, 1.1, -0.4, -0.9], 2))
        traj = str(rng.choice(["0,0,1,1", "0.071,0.071,0.93,0.93", "1,0,0,1", "0.2,0.9,0.8,0.1"]))
        effect = float(rng.choice([1.0, 3.0, 7.0]))
        lf = oc.synthetic_lf(n, W, H, int(rng.integers(1, 1 << 30)))
        case = dict(kind=kind, source=source, layout=layout, cols=cols, rows=rows, W=W, H=H, V=V, v0=v0, v1=v1, f0=f0, f1=f1, traj=traj, effect=effect)
        ctx = L.Context(0)
        ctx.set_grid(cols, rows, W, H)
        ctx.upload_grid(lf)
        ctx.set_output_layout(layout)
        if kind == "int":
            hp = L.build_params(cols, rows, W, H, traj, f0, 0.0, effect, 1.783, V)
            off = L.build_view_offsets(cols, rows, W, H, traj, 1.783, L.focus_ramp(f0, f1, V))
            ctx.set_params(hp)
            if source == "rgba":
                ctx.grid_device_ptr()
            ctx.set_view_offsets(off)
            maps = None
        else:
            frange = f1 - f0 if f1 != f0 else 0.5      # (the per-view maps' estimate takes a range > 0)
            if kind == "view_maps":
                frange = abs(frange)
            hp = L.build_params(cols, rows, W, H, traj, f0, frange, effect, 1.783, V)
            off, _ = L.build_view_centred_offsets(cols, rows, W, H, traj, 1.783, np.full(V, f0, np.float32))
            ctx.set_params(hp)
            ctx.set_view_float_offsets(off)
            map_seed = int(rng.integers(1, 1 << 30))
            if kind == "float":
                maps = view_rows.random_maps(H, W, map_seed)
                for k in (0, 1):
                    ctx.upload_map(k, maps[k])
            else:
                ctx.view_focus_maps(L.build_view_focus_ids(cols, rows, traj, V))
                maps = {v: view_rows.random_maps(H, W, map_seed + v) for v in range(v0, v1)}
                for v, pair in maps.items():
                    for k in (0, 1):
                        ctx.upload_view_map(v, k, pair[k])
        for method in view_rows.METHODS:
            want, S = [], []
            for v in range(v0, v1):
                w = hp.weights[v:v + 1]
                if kind == "int":
                    d = off[v].copy()
                    d[:, 0], d[:, 1] = np.clip(d[:, 0], -W, W), np.clip(d[:, 1], -H, H)
                    args, kw = (lf, d, hp.offsets, w), {}
                else:
                    pair = maps[v] if kind == "view_maps" else maps
                    args = (lf, hp.focused_offsets, off[v], w)
                    kw = dict(all_focus=True, map_plane=pair[1 if method == "STD" else 0], focus=hp.focus, rng=hp.range)
                if method == "STD":
                    want.append(oc.blend_std(*args, **kw)[0])
                else:
                    want.append(oc.blend_ten(*args, model=oc.TEN_M16, **kw)[0])
                    S.append(oc.blend_f64(*args, **kw)[0])
            want = np.stack(want)
            b = poison.render(ctx, method, all_focus=kind != "int", v0=v0, v1=v1)
            kernel = ctx.last_kernel_name()
            stray = poison.written_outside(ctx, v0, v1, b)
            got = ctx.download_views(v0, v1)
            found = dict(case, what=method, kernel=kernel, written_outside=stray)
            ok = kernel == view_rows.KERNEL[kind, source].format(method) and not stray
            if method == "STD":
                found["wrong"] = poison.mismatch(got, want)
                ok = ok and found["wrong"] == 0
            else:
                lo, hi = ten_interval.interval(np.stack(S), ten_interval.epsilon(hp.weights[v0:v1], n))
                found["lsb"] = int(np.abs(got.astype(int) - want.astype(int)).max())
                found["outside_interval"] = ten_interval.outside(got, lo, hi)
                ok = ok and found["lsb"] <= TEN_TOL_LSB and found["outside_interval"] == 0
            if not ok:
                bad.append(found)
        ctx.close()
        if log and (i + 1) % 20 == 0:
            log(f"{i + 1} cases, {len(bad)} mismatches")
    return bad
