"""GPU (-m gpu): a reused context against a fresh one across every state change — the table of tests/context_reuse.py.

Per change, one context: it is brought to the before-state and WORKED (every probe of that state once, checked: every buffer of the
Lifetimes table of DESIGN.md §3 that the state can allocate then exists and every cached value is set); the views, the scratch buffers, the
maps, the per-view maps and the deep planes are poisoned (never LFI_POISON_DERIVED or LFI_POISON_FOCUS_WORKSPACE: they reset grid_version and
pad_version, the bookkeeping under test); the change is applied with the calls a caller must repeat after it; every probe of the
after-state runs.  A second, fresh context is brought straight to the after-state and runs the same probes.  Both are held to the oracle or
restatement (STD, maps and every integer output `==`; TEN_WM within one LSB of M16 and inside the interval of the exact sum; the compare
records as tests/test_gpu_compare_views.py holds them; a call include/lfi.h refuses in the state by its message and an unchanged
lfi_memory_info), and the reused context's results equal the fresh one's byte for byte, TEN_WM included.

Memory after the probes (lfi_memory_info), every figure asserted.  After a change that calls lfi_set_grid all five equal the fresh
context's: the call releases every buffer and the geometry it was built with.  After any other change grid_bytes is the fresh context's;
views_bytes is the fresh context's plus, exactly, the deep planes of a before-state under LFI_FLAG_DEEP_VIEWS where the change kept the
views (they go with the views only); maps_bytes is the larger of the fresh context's and the worked before-state's (the per-view maps grow
only and go with lfi_set_grid); derived_bytes and workspace_bytes are at least the fresh context's and at most the larger of the fresh
context's and the worked before-state's plus the padding for growth that ensure_planar and launch_focus_factored_keys document (a quarter
of the reach or shift, rounded to 8: _growth restates both geometries) — a small fraction of either buffer, far from a second allocation.

test_one_long_lived_context walks one context through 40 seeded changes (context_reuse.walk: every family, both directions of every size),
three drawn probes after every step and all of them after every tenth, then destroys it and holds a fresh context to the oracle.

These tests hold the bookkeeping, not the races: at these shapes a missing stream wait may go unobserved (tests/stream_order.py)."""
import numpy as np
import pytest

import context_reuse as cr

pytestmark = pytest.mark.gpu


def _open(gpu):
    return cr.Run(gpu.Context(0))


def _close(run):
    run.ctx.close()
    run.keep.clear()     # the caller's buffers and stream outlive the context


def _same_bytes(reused, fresh, where):
    assert reused.keys() == fresh.keys()
    for name in reused:
        a, b = reused[name], fresh[name]
        assert (a is None) == (b is None), (where, name)
        if a is None:
            continue
        assert len(a) == len(b), (where, name)
        for i, (x, y) in enumerate(zip(a, b)):
            assert x.shape == y.shape and x.dtype == y.dtype and (x == y).all(), \
                (where, name, "the reused context answers otherwise than a fresh one", i, int((x != y).sum()))


def _round(v, unit):
    return (v + unit - 1) // unit * unit


def _growth(oc, st):
    """(derived, workspace): by how many bytes the two buffers that pad for growth may exceed what a context that allocated them at once has.
    ensure_planar (lfi_dispatch.hpp) builds a copy that has to grow for reach + reach / 4 + 8 instead of reach; launch_focus_factored_keys
    (lfi_focus_sched.hpp) pads planes that have to grow for need + need / 4 instead of need, both rounded up to 8.  The figures restate the two
    geometries for the largest reach and shift any probe of the state asks for, once as asked for and once grown."""
    s = cr.shadow(oc, st)
    hp = s.params(cr.L)
    D, O = cr.iw._view_offsets(cr.L, s)
    W, H = st.W, st.H
    i0, i1 = cr.held(oc, st) if st.windowed else (0, H)
    reach = max(int(np.abs(hp.focused_offsets[:, 0]).max()), int(np.clip(np.abs(D[..., 0]), 0, W).max()))

    def pitch(built):
        return _round(_round(built, 4) + 127 + _round(W, 128) + built, 128)
    derived = st.n * 3 * (i1 - i0) * (pitch(reach + reach // 4 + 8) - pitch(reach))
    fmax = max(abs(st.focus), abs(st.focus + st.rng)) * (1 + 1e-6)
    rx, ry = (int(v) for v in hp.block_radius)
    ids = max(len(hp.focus_map_ids), s.view_ids(cr.L).shape[1])
    need = [int(np.ceil(fmax * max(float(np.abs(hp.offsets[:, d]).max()), float(np.abs(O[..., d]).max())))) + 1 for d in (0, 1)]

    def planes(sx, sy):
        wp = _round(sx + rx + max(W + sx + rx, _round(W + 2 * rx, 256) - rx + sx), 4)
        hp_ = sy + ry + max(H + sy + ry, _round(H + 2 * ry, 4) - ry + sy)
        return 4 * (ids * hp_ + 128) * wp
    workspace = planes(*(_round(n + n // 4, 8) for n in need)) - planes(*(_round(n, 8) for n in need)) + 256
    return derived, workspace


def _deep_bytes(st):
    return st.V * 3 * st.H * _round(2 * st.W, 128)


def _check_memory(oc, change, worked, reused, fresh, grid_call):
    """lfi_memory_info of the reused context against the fresh one's (and the worked before-state's), every figure asserted"""
    b, a = change.before, change.after
    if grid_call:
        # lfi_set_grid releases every buffer and the geometry they were built with: the reused context IS a fresh one
        assert reused == fresh, ("after lfi_set_grid a reused context allocates otherwise than a fresh one", reused, fresh, "worked before-state", worked)
        return
    assert reused["grid_bytes"] == fresh["grid_bytes"], (reused, fresh)
    # the views are exact.  The deep planes (counted with them) are released with the views only: after a change that keeps the views
    # (no window, the same view count and layout) those of a before-state under LFI_FLAG_DEEP_VIEWS are still there, exactly
    views_kept = b.window == a.window and b.V == a.V and b.layout == a.layout
    stays = _deep_bytes(b) if b.flags & cr.DEEP and not a.flags & cr.DEEP and views_kept else 0
    assert reused["views_bytes"] == fresh["views_bytes"] + stays, ("views_bytes", reused, fresh, "deep planes that stay", stays)
    # the two map planes are exact and the per-view maps (counted with them) grow only, to 2 planes per view, and go with lfi_set_grid
    assert reused["maps_bytes"] == max(fresh["maps_bytes"], worked["maps_bytes"]), ("maps_bytes", reused, fresh, worked)
    for k, growth in zip(("derived_bytes", "workspace_bytes"), _growth(oc, a)):
        r, f, w = reused[k], fresh[k], worked[k]
        assert f <= r <= max(f, w) + growth, (k, "reused", r, "fresh", f, "worked before-state", w, "growth padding allowed", growth)


@pytest.mark.parametrize("change", cr.CHANGES, ids=lambda c: c.name)
def test_a_reused_context_answers_like_a_fresh_one(change, gpu, oracle_c):
    oc, b, a = oracle_c, change.before, change.after
    run, fresh = _open(gpu), _open(gpu)
    try:
        cr.move(oc, run, b)
        cr.run_probes(oc, run, b, f"{change.name}: the before-state")
        worked = cr.memory(run.ctx)
        run.ctx.poison(cr.poison_bits(b, a, change.again), cr.poison.POISON[len(change.name) & 1])
        bare = {}
        grid_call = change.again == "grid" or b.dims != a.dims
        cr.move(oc, run, a, again=change.again, on_grid=lambda: bare.update(reused=cr.bare_refusals(run.ctx)))
        cr.move(oc, fresh, a, on_grid=lambda: bare.update(fresh=cr.bare_refusals(fresh.ctx)))
        if grid_call:
            # after lfi_set_grid every reading call is refused until lfi_set_params, as on a fresh context, and in the same words
            assert bare["reused"] == bare["fresh"], {k: (v, bare["fresh"][k]) for k, v in bare["reused"].items() if v != bare["fresh"][k]}
        got_reused = cr.run_probes(oc, run, a, f"{change.name}: the reused context")
        got_fresh = cr.run_probes(oc, fresh, a, f"{change.name}: the fresh context")
        ran = [n for n, g in got_fresh.items() if g is not None]
        print(f"{change.name}: {len(ran)} probes ran, {len(got_fresh) - len(ran)} refused or skipped; calls: {run.log}")
        assert ran
        _same_bytes(got_reused, got_fresh, change.name)
        _check_memory(oc, change, worked, cr.memory(run.ctx), cr.memory(fresh.ctx), grid_call)
    finally:
        _close(run)
        _close(fresh)


def test_one_long_lived_context(gpu, oracle_c):
    oc = oracle_c
    steps = cr.walk()
    rng = np.random.default_rng(20272)
    run = _open(gpu)
    log = []
    try:
        cr.move(oc, run, cr.SMALL)
        cr.run_probes(oc, run, cr.SMALL, "the start")
        for i, (family, name, after, again) in enumerate(steps):
            log.append(f"{i}: {family}.{name} -> {after}")
            run.ctx.poison(cr.poison_bits(run.state, after, again), cr.poison.POISON[i & 1])
            cr.move(oc, run, after, again=again)
            active = [p.name for p, kind, _ in cr.probes_of(after) if kind != "skip"]
            only = None if i % 10 == 9 else {active[int(k)] for k in rng.choice(len(active), min(3, len(active)), replace=False)}
            log.append(f"    probes: {'all' if only is None else sorted(only)}")
            cr.run_probes(oc, run, after, f"step {i} ({family}.{name})", only)
        cr.run_probes(oc, run, run.state, "the end")
    except Exception:
        print("\n".join(log))
        raise
    finally:
        _close(run)          # lfi_destroy
    fresh = _open(gpu)
    try:
        cr.move(oc, fresh, cr.LARGE)
        cr.run_probes(oc, fresh, cr.LARGE, "a fresh context after lfi_destroy")
    finally:
        _close(fresh)
