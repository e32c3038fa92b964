"""Randomised parity cases shared by tests/test_gpu_fuzz.py (fixed seeds, a bounded number of cases) and the soak tools under
tools/ (fuzz_parity.py, fuzz_focus.py, fuzz_allfocus.py, fuzz_view_rows.py, fuzz_flagged.py: any number of cases, any seed).

Every function renders random small shapes through the HIP library (the C-ABI) and checks them against the CPU oracle — STD and
focus maps bit-exact, TEN_WM within one LSB of the fp16-accumulate model M16 and inside the interval of the exact sum
(tests/ten_interval.py) — and returns the list of mismatches (empty = pass).
`L` is the lfinterpolator_amd package, `oc` the oracle binding (oracle/lfi_oracle_c.py): the checker, never the thing measured.
"""
import numpy as np

import deep_ref
import focus_routes
import inframe_ref
import linear_ref
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


def focus_draws(L, oc, n_cases: int, seed: int):
    """fuzz_focus' cases, (case, hp, lf) each: the draw alone, on the CPU (tests/test_focus_routes_table.py states the leaves a seed reaches)"""
    rng = np.random.default_rng(seed)
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
        yield case, hp, lf


def focus_leaves(L, oc, case, hp, plan=None):
    """the leaves of tests/focus_routes.py a fuzz_focus case reaches, by the restatement"""
    c = dict(case, steps=32, more=())
    plan = plan or focus_routes.Plan(oc, case["W"], case["H"], hp.block_radius, hp.offsets[hp.focus_map_ids], hp.focus, hp.range)
    return focus_routes.leaves_of(c, hp, plan)


def fuzz_focus(L, oc, n_cases: int, seed: int, log=None) -> list:
    """Focus maps: the factored estimate, the LDS-staged one and the reference-shaped plain kernel on random shapes, radii, focus
    ranges and contents (quantised and partly black inputs produce ties and FLT_MIN taps) — all against the oracle; and the route each call
    took (lfi_focus_route_info) against the restatement of tests/focus_routes.py, the device's per-pass counts included.  Logs the leaves of
    that table the cases reached."""
    bad = []
    reached = set()
    for i, (case, hp, lf) in enumerate(focus_draws(L, oc, n_cases, seed)):
        cols, rows, W, H = case["cols"], case["rows"], case["W"], case["H"]
        want0 = oc.focus_estimate(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, threads=8)
        want1 = oc.focus_filter(want0, hp.block_radius)
        plan = focus_routes.Plan(oc, W, H, hp.block_radius, hp.offsets[hp.focus_map_ids], hp.focus, hp.range)
        reached |= focus_leaves(L, oc, case, hp, plan)
        ctx = L.Context(0)
        ctx.set_grid(cols, rows, W, H)
        ctx.upload_grid(lf)
        ctx.set_params(hp)
        state = focus_routes.PadState()
        for var in ("factored", "factored_direct", "plain", "lds"):
            ctx.set_variant("FOCUS", var)
            poison.focus_map(ctx)
            state.valid = False     # (the poison took the padded planes with the workspace: every call pads all of them)
            m0, m1 = ctx.download_map(0), ctx.download_map(1)
            if not ((m0 == want0).all() and (m1 == want1).all()):
                bad.append(dict(case, what="focus map", variant=var, wrong=int((m0 != want0).any(-1).sum())))
            got = ctx.focus_route()
            if var.startswith("factored"):
                want = focus_routes.expected_route(W, H, hp.block_radius, hp.offsets[hp.focus_map_ids], hp.focus_map_ids, hp.focus, hp.range, 32, var,
                                                   state=state, plan=plan)
                if want["declined"]:
                    want = dict(declined=want["declined"], estimate="lds" if var == "factored" else "packed_p2", passes=0)
            else:
                lds_fits = 128 + 2 * int(hp.block_radius[0]) + 8 <= 256   # the LDS-staged kernel's window in its 256-pixel row, else packed_p2
                want = dict(estimate="packed_p2" if var == "lds" and not lds_fits else var, declined="", passes=0)
            wrong = focus_routes.route_matches(got, want)
            if wrong:
                bad.append(dict(case, what="focus route", variant=var, fields={n: (got[n], want[n]) for n in wrong}))
        ctx.close()
        if log and (i + 1) % 20 == 0:
            log(f"{i + 1} cases, {len(bad)} mismatches")
    if log:
        log("leaves reached: " + "; ".join(sorted(reached)))
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


# ---- the flagged fixed-focus renders: deep_blend, blend_inframe, blend_linear (csrc/hip/blend_tile16.hpp) -------------------------------------------
# The draw is stratified, not free: case i takes entry i (cyclically, after one seeded shuffle per list) of each list, so that 24 cases show every
# value.  Images: one k-step of 16 (2, 3, 9: the lane-to-image clamp), of 32 (17, 32), a second k-step half unfetched (33, 48), one chunk (64), a
# second chunk of 16 (65, 80), a third chunk of 16 (129), a last chunk of 48 (225).  Widths: the ragged 8-byte store and the pitch padding it
# relies on (1, 4, 7, 9, 31, 100, 127, 129, 191, 257, 300), whole pieces (8, 64, 128).  Views: the wave boundaries (1, 15, 16, 17), one pass
# (64), a second (65), a third (129, 150).
FLAGGED_GRIDS = [(2, 1), (3, 1), (3, 3), (17, 1), (8, 4), (11, 3), (8, 6), (8, 8), (13, 5), (10, 8), (43, 3), (15, 15)]
FLAGGED_WIDTHS = [1, 4, 7, 8, 9, 31, 64, 100, 127, 128, 129, 191, 257, 300]
FLAGGED_VIEWS = [1, 3, 15, 16, 17, 64, 65, 129, 150]
FLAGGED_BUDGET = 120_000      # V·W·H of a stratified case: its CPU reference stays cheap.  (A third of it bought no time — the tests' cost is per view — and lost W = 300 beside V = 150: DESIGN.md §7)
# more tiles than the grid's 2 x CUs workgroups (512): every workgroup walks on to a second tile
FLAGGED_TILE_WALK = [dict(cols=17, rows=1, W=300, H=200, V=2), dict(cols=11, rows=3, W=64, H=1100, V=3)]
FLAGGED_KERNEL = {deep_ref.FLAG_DEEP_VIEWS: "deep_blend<{}>", inframe_ref.FLAG_IN_FRAME: "blend_inframe<{}>", linear_ref.FLAG_LINEAR_LIGHT: "blend_linear<{}>"}
# the offset sets a flag renders, in order; lfi_release_inputs follows the last
FLAGGED_SETS = {deep_ref.FLAG_DEEP_VIEWS: ("wide",), inframe_ref.FLAG_IN_FRAME: ("wide", "near"), linear_ref.FLAG_LINEAR_LIGHT: ("wide",)}
PLANAR_REFUSAL = "the planar copy of the inputs cannot serve these offsets"
# what tests/test_gpu_fuzz.py runs and tests/test_fuzz_flagged_table.py holds to the draw's conditions on the CPU
FLAGGED_CASES = 24
FLAGGED_SEED = {deep_ref.FLAG_DEEP_VIEWS: 7, inframe_ref.FLAG_IN_FRAME: 8, linear_ref.FLAG_LINEAR_LIGHT: 9}


def flagged_wide(i, W, H):
    """(ax, ay) of case i's `wide` offsets: none; one pixel; inside a lane's 8 pixels and beyond; the whole frame but one pixel; beyond the frame
    (the clamp is served by the planar copy's padding, in-frame masks everything out)"""
    return [(0, 0), (1, 1), (9, 2), (W - 1, H - 1), (W + 5, H + 2)][i % 5]


def flagged_near(n, W, H):
    """(ax, ay) of a case's `near` offsets: a quarter of the frame.  Narrowed for grids of fewer than 9 images to a sixteenth of the width: there
    a view may rest on one image whose weight is tiny, r = wall / den reaches 64 wherever the other is out of frame and scales the TEN_WM bound
    with it — at W // 4 the two-valued share of such a case (2 images, 300 x 6) was 2.8 %, over the cap of 2 %"""
    return (max(1, W // (4 if n >= 9 else 16)), H // 4)


def flagged_cases(n_cases, seed):
    """the draw: n_cases stratified cases and the two tile-walk cases, as dicts of plain values and small arrays; numpy alone"""
    rng = np.random.default_rng(seed)
    grids, widths, views = ([lst[int(k)] for k in rng.permutation(len(lst))] for lst in (FLAGGED_GRIDS, FLAGGED_WIDTHS, FLAGGED_VIEWS))
    flat = {int(k) for k in rng.choice(n_cases, min(2, n_cases), replace=False)}     # H = 1 forced
    out, over64, crossing = [], 0, 0
    for i in range(n_cases + len(FLAGGED_TILE_WALK)):
        if i < n_cases:
            (cols, rows), W, V = grids[i % len(grids)], widths[i % len(widths)], views[i % len(views)]
            H = 1 if i in flat else int(rng.integers(1, 7))
            tries = 0
            while V * W * H > FLAGGED_BUDGET:     # redraw H (a forced H = 1 stays), then V: the lists of n and W never shrink
                if tries < 8 and i not in flat:
                    H = int(rng.integers(1, 7))
                else:
                    V = int(rng.choice(FLAGGED_VIEWS))
                tries += 1
        else:
            t = FLAGGED_TILE_WALK[i - n_cases]
            cols, rows, W, H, V = t["cols"], t["rows"], t["W"], t["H"], t["V"]
        n = cols * rows
        traj = str(rng.choice(["0,0,1,1", "0.071,0.071,0.93,0.93", "1,0,0,1", "0.5,0.5,0.5,0.5", "0.2,0.9,0.8,0.1"]))
        effect = float(rng.choice([1.0, 3.0, 7.0]))
        case = dict(kind="flagged", i=i, cols=cols, rows=rows, W=W, H=H, V=V, traj=traj, effect=effect, lf_seed=int(rng.integers(1, 1 << 30)))
        case["reach"] = dict(wide=flagged_wide(i, W, H), near=flagged_near(n, W, H))
        case["offsets"] = {k: np.stack([rng.integers(-ax, ax + 1, n), rng.integers(-ay, ay + 1, n)], axis=1).astype(np.int32) for k, (ax, ay) in case["reach"].items()}
        # the exact rows (linear_ref.exact_rows): one-hot on a drawn image, one-hot on image n − 1, two halves on two drawn images
        k = min(V, 3)
        case["exact_views"] = [int(v) for v in rng.choice(V, k, replace=False)]
        pair = [int(g) for g in rng.choice(n, 2, replace=False)]
        case["exact_images"] = [(int(rng.integers(0, n)),), (n - 1,), tuple(pair)][:k]
        # the view range; half of the cases with V > 64 cross a 64-view pass from an unaligned start, where there is room for one
        v0 = int(rng.integers(0, V))
        v1 = int(rng.integers(v0 + 1, V + 1))
        if V > 64:
            over64 += 1
            if V >= 82 and 2 * crossing < over64:
                crossing += 1
                v0 = int(rng.integers(1, 16))
                v1 = int(rng.integers(v0 + 65, V + 1))
        case["v0"], case["v1"] = v0, v1
        out.append(case)
    return out


def flagged_label(case, **more):
    """a case as the plain values a mismatch reports"""
    return dict({k: v for k, v in case.items() if k != "offsets"}, **more)


def flagged_params(L, case, which):
    """the host parameters of a case under its `wide` or `near` offsets: build_params' weights with the exact rows in place"""
    hp = L.build_params(case["cols"], case["rows"], case["W"], case["H"], case["traj"], 0.0, 0.0, case["effect"], 1.783, case["V"])
    w = hp.weights.copy()
    one, half = np.float16(1.0).view(np.uint16), np.float16(0.5).view(np.uint16)
    for v, images in zip(case["exact_views"], case["exact_images"]):
        w[v, :] = 0
        w[v, list(images)] = one if len(images) == 1 else half
    return L.host.HostParams(np.ascontiguousarray(case["offsets"][which], np.int32), hp.offsets, w, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)


class FlaggedWant:
    """what a flag's renders of a case must be.  hp, lf; std [V][H][W][3] uint8: the STD bytes; lo, hi: the TEN_WM bytes' interval; exact
    [rows][H][W][3]: the TEN_WM bytes of the exact rows.  Deep views also: codes (STD), lo10, hi10, exact10 (TEN_WM), and lo, hi are
    ten_interval.bounds.  res: the restatement (in-frame, linear light)"""


def flagged_reference(L, oc, case, flag, which):
    want = FlaggedWant()
    hp = want.hp = flagged_params(L, case, which)
    n = case["cols"] * case["rows"]
    lf = want.lf = oc.synthetic_lf(n, case["W"], case["H"], case["lf_seed"])
    rows = case["exact_views"]
    want.res = None
    if flag == deep_ref.FLAG_DEEP_VIEWS:
        std, pre = oc.blend_std(lf, hp.focused_offsets, hp.offsets, hp.weights, return_prequant=True, threads=8)
        S, eps = ten_interval.exact_sums(oc, lf, hp, threads=8)
        want.std, want.codes = std[..., :3], deep_ref.q10_std(pre)
        want.lo10, want.hi10 = deep_ref.interval10(S, eps)
        want.lo, want.hi = ten_interval.interval(S, eps)
        want.exact10 = deep_ref.q10_ten(S[rows])
        want.exact = (want.exact10 >> 2).astype(np.uint8)
    elif flag == inframe_ref.FLAG_IN_FRAME:
        res = want.res = inframe_ref.restate(lf, hp)
        want.std = res.bytes
        want.lo, want.hi = inframe_ref.ten_interval_of(res, hp, n)
        want.exact = inframe_ref.ten_exact(res)[rows]
    else:
        res = want.res = linear_ref.restate(lf, hp)
        want.std = res.bytes
        want.lo, want.hi = linear_ref.ten_interval_of(res, hp, n)
        want.exact = res.bytes[rows]
    return want


def _flagged_compare(method, views, codes, want, a, b, rows):
    """the nonzero counts of what is wrong with views [a, b) as downloaded (codes: the deep views', or None)"""
    c = views[..., :3]
    found = dict(alpha_not_255=int((views[..., 3] != 255).sum()))
    if method == "STD":
        found["wrong_bytes"] = int((c != want.std[a:b]).sum())
        if codes is not None:
            found["wrong_codes"] = int((codes != want.codes[a:b]).sum())
    else:
        found["outside_interval"] = int(((c < want.lo[a:b]) | (c > want.hi[a:b])).sum())
        inside = [(k, v) for k, v in enumerate(rows) if a <= v < b]
        found["exact_rows_wrong"] = sum(int((c[v - a] != want.exact[k]).sum()) for k, v in inside)
        if codes is not None:
            found["codes_outside_interval"] = int(((codes < want.lo10[a:b]) | (codes > want.hi10[a:b])).sum())
            found["code_is_not_the_byte"] = int((codes >> 2 != c).sum())
            found["exact_rows_wrong"] += sum(int((codes[v - a] != want.exact10[k]).sum()) for k, v in inside)
    return {k: v for k, v in found.items() if v}


def fuzz_flagged(L, oc, flag, n_cases: int, seed: int, log=None) -> list:
    """The flagged fixed-focus renders (launch_flagged_views: deep_blend under LFI_FLAG_DEEP_VIEWS, blend_inframe under LFI_FLAG_IN_FRAME,
    blend_linear under LFI_FLAG_LINEAR_LIGHT): n_cases stratified cases (flagged_cases) and the two tile-walk cases, one context each, the inputs
    uploaded, the planar layout, explicit integer offsets (`wide`; in-frame: `wide`, then `near`).  Every render under poison.  STD bytes (and
    deep codes) `==` the reference; TEN_WM bytes (and codes) inside the flag's own interval, the exact rows `==`, alpha 255; a view range writes
    its views only and the same bytes; the kernel is the flag's; after lfi_release_inputs the same bytes.  A release or a render refused
    because the planar copy cannot serve the offsets is the case's outcome (log), not a mismatch."""
    deep = flag == deep_ref.FLAG_DEEP_VIEWS
    bad = []

    def render(ctx, method, a=0, b=None):
        if not deep:
            return poison.render(ctx, method, v0=a, v1=b)
        ctx.prepare(method, v0=a, v1=b)      # allocates the deep planes: they are poisoned with the views
        byte = poison._byte(None)
        ctx.poison(poison.RENDER | L.LFI_POISON_DEEP, byte)
        ctx.render(method, v0=a, v1=b)
        ctx.sync()
        return byte

    for case in flagged_cases(n_cases, seed):
        V, v0, v1, rows = case["V"], case["v0"], case["v1"], case["exact_views"]
        ctx = L.Context(0)
        ctx.set_grid(case["cols"], case["rows"], case["W"], case["H"])
        ctx.set_output_layout("planar")
        outcome = "served"
        for which in FLAGGED_SETS[flag]:
            want = flagged_reference(L, oc, case, flag, which)
            if which == FLAGGED_SETS[flag][0]:
                ctx.upload_grid(want.lf)
            ctx.set_params(want.hp, flags=flag)
            last = which == FLAGGED_SETS[flag][-1]
            before = codes_before = None     # the TEN_WM bytes (and codes) before the release; None where that render was refused
            for released in ((False, True) if last else (False,)):
                try:
                    if released:
                        ctx.release_inputs()
                    for method in ("STD", "TEN_WM"):
                        render(ctx, method)
                        found = {} if ctx.last_kernel_name() == FLAGGED_KERNEL[flag].format(method) else dict(kernel=ctx.last_kernel_name())
                        full, codes = ctx.download_views(), ctx.download_deep_views() if deep else None
                        found.update(_flagged_compare(method, full, codes, want, 0, V, rows))
                        if released:
                            if method == "TEN_WM" and before is not None and (not (full == before).all() or (deep and not (codes == codes_before).all())):
                                found["not_the_bytes_before_the_release"] = True
                        else:
                            if method == "TEN_WM":
                                before, codes_before = full, codes
                            byte = render(ctx, method, v0, v1)
                            stray = poison.written_outside(ctx, v0, v1, byte)
                            part, pcodes = ctx.download_views(v0, v1), ctx.download_deep_views(v0, v1 - v0) if deep else None
                            ranged = _flagged_compare(method, part, pcodes, want, v0, v1, rows)
                            if stray:
                                ranged["written_outside"] = stray[:8]
                            if method == "TEN_WM" and (not (part == full[v0:v1]).all() or (deep and not (pcodes == codes[v0:v1]).all())):
                                ranged["not_the_full_renders_bytes"] = True
                            if ranged:
                                found["range"] = ranged
                        if found:
                            bad.append(flagged_label(case, what=method, offsets=which, released=released, **found))
                except L.LfiError as e:
                    if released and PLANAR_REFUSAL in str(e):
                        outcome = "refused after the release: " + str(e)
                    else:
                        bad.append(flagged_label(case, what="refused", offsets=which, released=released, error=str(e)))
        ctx.close()
        if log:
            log(f"case {case['i']}: {case['cols']}x{case['rows']} images, {case['W']}x{case['H']}, {V} views, range [{v0}, {v1}): {outcome}; {len(bad)} mismatches")
    return bad
