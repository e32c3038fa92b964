"""CPU: the focus routes' table (tests/focus_routes.py) held to its claims before tests/test_gpu_focus_routes.py leans on it.

Every leaf of LEAVES is reached by a case, and every case reaches the leaves it names — by the exact restatement of the plan and of the routing,
with the constants parsed from the headers, so a constant that moves a route fails here.  The restatement's own keys give the oracle's map 0
on every case.  For every class of flagged pairs a case claims (CLASS_SHOWS), the map a kernel gives that skipped the class — the uniform-shift
key at the class's pairs — differs from the oracle's map 0, and only at pixels of that class: none of the classes could vanish unnoticed.  The
oracle's maps are not degenerate.  lfi_focus_route's fields are the header's.  The leaves the fuzz's fixed seed reaches are stated."""
import functools
import os
import re

import numpy as np
import pytest

import focus_routes as fr
import focus_steps_ref
import fuzz_cases
import lfinterpolator_amd as L

NAMES = [c["name"] for c in fr.CASES]


@functools.lru_cache(maxsize=None)
def _built(name):
    from oracle import lfi_oracle_c as oc
    oc.build()
    c = next(c for c in fr.CASES if c["name"] == name)
    hp, lf = fr.build(L, oc, c)
    plan = fr.plan_of(L, oc, c, hp)
    return c, hp, lf, plan


@functools.lru_cache(maxsize=None)
def _maps(name):
    """(the oracle's map 0 byte plane, the restatement's exact keys, its uniform-shift keys)"""
    from oracle import lfi_oracle_c as oc
    c, hp, lf, plan = _built(name)
    if c["steps"] == 32:
        want0 = oc.focus_estimate(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)
    else:
        want0 = focus_steps_ref.map0(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, c["steps"])
    assert (want0[..., :3] == want0[..., :1]).all() and (want0[..., 3] == 255).all()
    exact, unif = fr.key_planes(plan, lf, hp.focus_map_ids)
    return want0[..., 0], exact, unif


def test_the_constants_are_the_headers():
    k = fr.constants()
    assert (k["FRT_MAX_DX"], k["FRT_MAX_DY"], k["FRT_TW"], k["FRT_TH"], k["FOCUS_STEPS"], k["FOCUS_MAX_PASSES"]) == (32, 18, 64, 32, 32, 8)
    assert (k["R_CAP_FACTOR"], k["C_CAP_FACTOR"], k["PLANES_LIMIT"], k["TYPED_LIMIT"], k["PICK_SEP_MAX_RX"]) == (4, 4, 16 << 30, 1 << 32, 64)
    # the LDS patch of focus_range_t holds a group's span: the rule group_size restates is the one the patch is sized by
    text = open(os.path.join(fr.HIP, "focus_factored.hpp")).read()
    assert "constexpr int FRT_PW = FRT_TW + FRT_MAX_DX;" in text
    assert "return hi[0] - lo[0] <= FRT_MAX_DX && hi[1] - lo[1] <= FRT_MAX_DY;" in text


def test_fma32_rounds_once():
    # (1 + 2^-23)^2 + 2^-24 = 1 + 2^-22 + 2^-24 + 2^-46: 2^-46 above the midpoint of two floats — up; without the product's last bit — a tie, to even
    a, c = np.float32(1 + 2.0 ** -23), np.float32(2.0 ** -24)
    assert fr.fma32(a, a, c) == np.float32(1 + 2.0 ** -22 + 2.0 ** -23)
    assert fr.fma32(np.float32(1 + 2.0 ** -22), np.float32(1), c) == np.float32(1 + 2.0 ** -22)
    assert fr.fma32(np.float32(1 + 2.0 ** -23), np.float32(1), c) == np.float32(1 + 2.0 ** -22)
    for f, r, n in [(0.22, 0.17, 32), (-0.3, 0.6, 64), (0.1, 0.4, 256)]:
        assert (fr.candidates(f, r, n).view(np.uint32) == L.focus_candidates(f, r, n).view(np.uint32)).all()


def test_every_leaf_has_a_case_and_every_case_reaches_its_leaves():
    reached = set()
    for name in NAMES:
        c, hp, lf, plan = _built(name)
        got = fr.leaves_of(c, hp, plan)
        assert set(c["leaves"]) <= got, (name, sorted(set(c["leaves"]) - got))
        assert got <= set(fr.LEAVES), (name, sorted(got - set(fr.LEAVES)))
        reached |= got
    for what, hp, again, route, leaves in fr.pad_sequence_routes(L):
        reached |= leaves
    # slot-stable re-padding: the views of a per-view batch share slots, so a batch pads fewer planes than views x images
    c, hp, lf, plan = _built("both_overflows")
    O, ids = _view_batch(c)
    route, rows = fr.view_maps_route(c["W"], c["H"], hp.block_radius, O, ids, hp.focus, hp.range)
    assert route["jobs"] == len(ids) and len(ids[0]) <= route["planes_padded"] < len(ids) * len(ids[0]) and route["planes_kept"] > 0
    reached.add("slot-stable re-padding")
    assert reached == set(fr.LEAVES), sorted(set(fr.LEAVES) - reached)
    assert len(set(fr.LEAVES)) == len(fr.LEAVES) and len(set(NAMES)) == len(NAMES)


def _view_batch(c, V=3):
    O, _ = L.build_view_centred_offsets(c["cols"], c["rows"], c["W"], c["H"], fr.TRAJ, 1.783, np.full(V, c["focus"], np.float32))
    return O, L.build_view_focus_ids(c["cols"], c["rows"], fr.TRAJ, V)


def test_the_counts_at_the_caps():
    """the exact restatement's counts, as DESIGN.md §7 states them"""
    want = {"both_overflows": ([46], 32, [67], 32), "col_overflow": ([46], 96, [67], 32), "rows_above": ([70], 68, [88], 132),
            "rows_below": ([67], 68, [87], 132), "cols_below": ([34], 160, [47], 48), "cols_at_cap": ([34], 160, [48], 48),
            "cols_above": ([36], 160, [49], 48), "two_views": ([0], 20, [32], 28), "t4": ([74], 64, [205], 256),
            "sweep64_first": ([58, 42], 48, [87, 57], 64), "sweep64_later": ([32, 45], 32, [32, 71], 32),
            "sweep256_first": ([64, 64, 64, 40, 32, 32, 32, 38], 32, [97, 96, 86, 64, 64, 43, 32, 38], 32),
            "sweep256_later": ([32, 39, 32, 32, 32, 32, 53, 64], 32, [32, 39, 32, 32, 55, 64, 64, 64], 32)}
    for name, (rows, r_cap, cols, c_cap) in want.items():
        plan = _built(name)[3]
        assert (plan.row_entries, plan.R_cap, plan.col_entries, plan.C_cap) == (rows, r_cap, cols, c_cap), name


@pytest.mark.parametrize("name", NAMES)
def test_the_restatements_keys_give_the_oracles_map(name):
    c, hp, lf, plan = _built(name)
    want0, exact, unif = _maps(name)
    assert (fr.map0_of(plan, exact) == want0).all()
    assert len(np.unique(want0)) >= fr.DISTINCT_MIN.get(name, 5), (name, len(np.unique(want0)))
    # the shortcut is proven where it is used: an unflagged pair's uniform-shift key is the exact one
    assert (unif[plan.cls == 0] == exact[plan.cls == 0]).all()


@pytest.mark.parametrize("name,cls", [(n, k) for n, ks in fr.CLASS_SHOWS.items() for k in ks])
def test_skipping_a_class_changes_the_map(name, cls):
    c, hp, lf, plan = _built(name)
    want0, exact, unif = _maps(name)
    assert cls in plan.classes()
    wrong = fr.naive_map0(plan, exact, unif, cls) != want0
    of_class = (plan.cls == 1 + fr.CLASSES.index(cls)).any(axis=0)
    assert wrong.any() and not (wrong & ~of_class).any(), (name, cls, int(wrong.sum()))


def test_every_class_is_shown_and_every_class_leaf_is_a_shown_one():
    shown = {k for ks in fr.CLASS_SHOWS.values() for k in ks}
    assert shown == set(fr.CLASSES)
    for c in fr.CASES:
        for leaf in c["leaves"]:
            if leaf.startswith("class "):
                assert leaf[6:] in fr.CLASS_SHOWS.get(c["name"], []), (c["name"], leaf)


def test_the_record_is_the_headers():
    text = open(os.path.join(fr.ROOT, "include", "lfi.h")).read()
    body = re.search(r"typedef struct lfi_focus_route \{(.*?)\} lfi_focus_route;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []   # (name, type, array length or 0) in the header's order
    for kind, names in re.findall(r"(const char \*|int32_t |uint32_t )([^;]+);", body):
        for n in names.split(","):
            m = re.fullmatch(r"(\w+)(?:\[(\w+)\])?", n.strip())
            fields.append((m.group(1), kind.strip(), {None: 0, "2": 2, "LFI_FOCUS_ROUTE_PASSES": L.abi.LFI_FOCUS_ROUTE_PASSES}[m.group(2)]))
    ctype = {L.abi.C.c_char_p: "const char *", L.abi.C.c_int32: "int32_t", L.abi.C.c_uint32: "uint32_t"}
    bound = [(n, ctype[getattr(k, "_type_", k) if hasattr(k, "_length_") else k], getattr(k, "_length_", 0)) for n, k in L.abi.FocusRoute._fields_]
    assert fields == bound and len(fields) == 21
    assert int(re.search(r"#define LFI_FOCUS_ROUTE_PASSES (\d+)", text).group(1)) == L.abi.LFI_FOCUS_ROUTE_PASSES == fr.constants()["FOCUS_MAX_PASSES"]
    assert "lfi_focus_route_info" in L.ABI_SYMBOLS
    # the restatement speaks of every field but the two counters of calls and jobs
    c, hp, lf, plan = _built("t4")
    route = fr.expected_route(c["W"], c["H"], hp.block_radius, hp.offsets[hp.focus_map_ids], hp.focus_map_ids, hp.focus, hp.range, plan=plan)
    assert set(route) | {"calls", "jobs"} == {n for n, _ in L.abi.FocusRoute._fields_}


# the leaves tests/fuzz_cases.py::fuzz_focus reaches with the suite's seed and count (tests/test_gpu_fuzz.py), by the restatement
FUZZ_SEED_1 = {
    "focus_range_t<8>", "focus_range_t<4>", "focus_range<4> direct", "focus_range_t<8> striped", "focus_range_t<4> striped", "focus_range_t plain order",
    "focus_range<4> plain order", "focus_pick_sep", "focus_pick<2>", "focus_pick<1>", "pick striped", "pick plain order", "negative focus",
    "class row_line", "class col_line", "class corner", "class a_row_noslot", "class a_col_noslot", "class b", "class c",
    "column overflow beside flagged rows", "rows above R_cap by at most 4", "rows below R_cap by at most 4", "columns at C_cap exactly",
    "columns below C_cap by at most 4",
}   # 25 of the table's 51: no fall-back to focus_range, no sweep, neither decline, never both overflows in one pass


def test_the_fuzzs_fixed_seed_reaches_these_leaves():
    from oracle import lfi_oracle_c as oc
    oc.build()
    reached = set()
    for case, hp, lf in fuzz_cases.focus_draws(L, oc, 40, 1):
        reached |= fuzz_cases.focus_leaves(L, oc, case, hp)
    assert reached == FUZZ_SEED_1, sorted(reached)
