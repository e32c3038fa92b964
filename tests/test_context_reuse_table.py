"""CPU: the table of tests/context_reuse.py held to the header and to being a check, before tests/test_gpu_context_reuse.py leans on it.

Completeness: every `int lfi_*` function of include/lfi.h is a change (CHANGE_CALLS), is called by a probe, is a writer of inputs that
tests/input_writers.py owns, or is in EXCLUDED with its reason — the next function added to the ABI fails here until it is classified.
Reach: N, W, H, V and the held rows each grow alone and shrink alone in some change, and the long-lived walk takes every family and both
directions of every size.  Discrimination, on the oracle and the restatements alone: for every change, every probe that runs in both states
either has expected outputs of another shape, or outputs that differ — colour bytes in at least half of the compared bytes, maps and curves
in some element — or is declared independent of what changes (Probe.fields), and then its two expected outputs ARE equal and the pair is
recorded, with the reason, in context_reuse.DROPPED; a probe that merely flips between served and refused does not count as telling; a
change after which no probe's output tells the states apart is named in NO_OUTPUT_CHANGES with the reason."""
import os
import re

import pytest

import context_reuse as cr
import input_writers as iw
from conftest import ROOT


def _declared():
    with open(os.path.join(ROOT, "include", "lfi.h")) as f:
        text = f.read()
    return re.findall(r"^(?:int|const char \*)\s*(lfi_\w+)\(", text, flags=re.M)


def test_every_function_of_the_header_is_classified():
    declared = _declared()
    assert len(declared) > 80 and "lfi_set_grid" in declared and "lfi_last_error" in declared, "the header is no longer parsed"
    kinds = {f: cr.classify(f) for f in declared}
    missing = sorted(f for f, k in kinds.items() if k is None)
    assert not missing, f"declared in include/lfi.h and neither a change, a probe's call, a writer of input_writers.WRITERS nor in EXCLUDED: {missing}"
    probe_calls = {f for p in cr.PROBES for f in p.calls}
    writers = {f for w in iw.WRITERS for f in w.abi}
    named = cr.CHANGE_CALLS | probe_calls | set(cr.EXCLUDED)
    assert not sorted(named - set(declared)), "the table names functions the header does not declare"
    # exactly one class each, but for the per-view rows, which are a change and what two probes set for themselves
    assert cr.CHANGE_CALLS & probe_calls == cr.CHANGE_AND_PROBE, sorted(cr.CHANGE_CALLS & probe_calls)
    assert not set(cr.EXCLUDED) & (cr.CHANGE_CALLS | probe_calls | writers), sorted(set(cr.EXCLUDED) & (cr.CHANGE_CALLS | probe_calls | writers))
    # a writer of inputs that a probe also calls: the input-side pair, on purpose
    assert probe_calls & writers == {"lfi_upload_images_yuv"}, sorted(probe_calls & writers)
    assert all(len(reason) > 10 for reason in cr.EXCLUDED.values())
    # every state-changing call has a row
    assert {c.family for c in cr.CHANGES} == set(cr.FAMILIES)
    for f in ("lfi_set_grid", "lfi_set_row_window", "lfi_set_params", "lfi_set_output_layout", "lfi_attach_views", "lfi_attach_grid",
              "lfi_release_inputs", "lfi_set_focus_steps", "lfi_set_yuv_siting", "lfi_set_stream", "lfi_set_view_offsets", "lfi_set_variant"):
        assert kinds[f] == "change", (f, kinds[f])
    print({k: sum(1 for v in kinds.values() if v == k) for k in ("change", "probe", "writer", "excluded")})


def test_every_size_grows_alone_and_shrinks_alone(oracle_c, native):
    seen = {s for c in cr.CHANGES for s in c.sizes}
    assert seen == {(size, way) for size in ("N", "W", "H", "V", "held") for way in ("grows", "shrinks")}, sorted(seen)
    for c in cr.CHANGES:
        a, b = c.before, c.after
        sizes = {"N": (a.n, b.n), "W": (a.W, b.W), "H": (a.H, b.H), "V": (a.V, b.V),
                 "held": tuple(y1 - y0 for y0, y1 in (cr.held(oracle_c, s) for s in (a, b))) if a.window or b.window else (0, 0)}
        changed = {k for k, (x, y) in sizes.items() if x != y}
        for size, way in c.sizes:
            assert changed == {size}, (c.name, "not alone", changed)
            x, y = sizes[size]
            assert (y > x) == (way == "grows"), (c.name, size, x, y)


def test_the_windows_are_interior_and_the_moved_band_keeps_its_size(oracle_c, native):
    bands = [cr.held(oracle_c, s) for s in (cr.BAND, cr.BAND_LARGER, cr.BAND_ELSEWHERE)]
    for s, (i0, i1) in zip((cr.BAND, cr.BAND_LARGER, cr.BAND_ELSEWHERE), bands):
        o0, o1 = s.window
        assert 0 < i0 < o0 and o1 < i1 < s.H, (s.window, i0, i1)     # five different numbers
    (a0, a1), (b0, b1), (c0, c1) = bands
    assert a1 - a0 == c1 - c0 and (a0, a1) != (c0, c1) and c0 >= a1, "the moved band: the same size, no row in common"
    assert b1 - b0 > a1 - a0


def test_the_shapes_are_the_smallest_at_which_the_machinery_is_live():
    s, l = cr.SMALL, cr.LARGE
    assert s.W % 8 == 0 and s.W % 128 != 0 and (s.W + 127) // 128 == 2
    assert l.n > 64 and (l.n + 15) // 16 * 16 == 80 and l.V > 64 and l.W % 8 != 0
    assert all(v % 2 == 0 for v in (s.W, s.H, l.W, l.H, cr.TALL.H))
    assert (5 + 63) // 64 == (7 + 63) // 64, "5 and 7 views share v_pad: an equal parameter blob, another view count"
    assert cr.tile_size(s) != cr.tile_size(l)


@pytest.mark.parametrize("change", cr.CHANGES, ids=lambda c: c.name)
def test_no_change_could_pass_on_the_previous_answer(change, oracle_c, native):
    table = cr.discrimination(oracle_c, change)
    for name, verdict, figure in table:
        print(f"{change.name}: {name}: {verdict} {figure:.3f}")
    probe = {p.name: p for p in cr.PROBES}
    for name, verdict, figure in table:
        if verdict == "differs":
            assert figure >= 0.5 if probe[name.split(" against ")[0]].colour else figure > 0, (change.name, name, "a stale answer could pass", figure)
    # the pairs dropped from this change are the table's own record (cr.DROPPED), each with its reason
    assert sorted(n for n, v, _ in table if v == "independent") == sorted(n for (c, n) in cr.DROPPED if c == change.name)
    assert all(len(cr.DROPPED[change.name, n]) > 20 for n, v, _ in table if v == "independent")
    telling = [name for name, verdict, _ in table if verdict in ("differs", "shape")]
    flips = [name for name, verdict, _ in table if verdict == "flips"]
    if change.name in cr.NO_OUTPUT_CHANGES:
        assert not telling, (change.name, "tells the states apart after all")
        assert flips or change.family in ("set_stream", "set_variant"), (change.name, "neither an output nor a refusal changes")
    else:
        assert telling, (change.name, "no probe's expected output tells the two states apart: a flip alone does not count")


def test_the_walk_takes_every_family_and_both_directions_of_every_size():
    steps = cr.walk()
    assert len(steps) == 40 and steps == cr.walk(), "not reproducible"
    assert {f for f, _, _, _ in steps} == set(cr.FAMILIES), sorted(set(cr.FAMILIES) - {f for f, _, _, _ in steps})
    st, ways = cr.SMALL, set()
    for _, _, after, _ in steps:
        for size, x, y in (("N", st.n, after.n), ("W", st.W, after.W), ("H", st.H, after.H), ("V", st.V, after.V),
                           ("held", st.band[1] - st.band[0] if st.H == after.H else None, after.band[1] - after.band[0])):
            if x is not None and x != y:
                ways.add((size, "grows" if y > x else "shrinks"))
        st = after
    assert ways == {(size, way) for size in ("N", "W", "H", "V", "held") for way in ("grows", "shrinks")}, sorted(ways)
    # a linear-light state and a deep one are on the way
    assert any(after.flags & cr.LINEAR for _, _, after, _ in steps) and any(after.flags & cr.DEEP for _, _, after, _ in steps)


def test_the_linear_light_flag_is_a_view_flag_in_every_predicate():
    """a linear-light state is a flagged state to every probe: none treats it as flag-free"""
    assert cr.VIEW_FLAGS == cr.DEEP | cr.IN_FRAME | cr.LINEAR
    plain, linear = cr.FAR_P, cr.LINEAR_P
    modes = {p.name: (p.mode(plain), p.mode(linear)) for p in cr.PROBES}
    assert modes["linear_std"] == (cr.SKIP("LFI_FLAG_LINEAR_LIGHT is not set, or std holds its refusal of the RGBA layout"), cr.RUN) and modes["linear_ten_wm"][1] == cr.RUN
    assert modes["std"] == (cr.RUN, cr.RUN) and modes["std_view_range"] == (cr.RUN, cr.RUN)       # against linear_ref under the flag
    for name in ("ten_wm", "std_variant_persist", "keep_and_compare_views", "download_quilt_scaled", "download_views_yuv420", "upload_images_yuv_then_std"):
        assert modes[name] == (cr.RUN, cr.SKIP(cr.FLAGGED)), (name, modes[name])
    for name in ("view_rows_planar_source", "all_focus_std_uploaded_map", "all_focus_ten_wm_uploaded_map", "render_stream"):
        assert modes[name][1][0] == "refused", (name, modes[name])
    assert cr.Std().mode(cr.replace(linear, layout="rgba")) == cr.REFUSED(cr.NEEDS_PLANAR)
    assert {"params_flag_linear_up", "params_flag_linear_down", "params_flag_linear_deep_up", "params_flag_linear_deep_down", "params_flag_linear_in_frame_up",
            "params_flag_linear_in_frame_down", "linear_then_more_views", "linear_then_set_grid"} <= {c.name for c in cr.CHANGES}
    assert not any(c.name in cr.NO_OUTPUT_CHANGES for c in cr.CHANGES if "linear" in c.name)
