"""CPU: the oracle against the reference's own kernels.

tests/golden/ref_kernels.npz holds what the reference's src/kernels.cu computes when it is compiled for the CPU (oracle/ref_kernels.cpp over
the shim headers in oracle/ref_shim/, tests/golden/make_ref_kernel_golden.py).  Every GPU test compares the HIP kernels with the oracle, so
the oracle's own reading of that source is what these tests pin: STD, the focus estimate and the filter byte for byte, and TEN_WM's M16 model
in everything around the matrix instruction (fragment addressing, pixel packing, batch order, which map is read, the final truncation —
the accumulate rounding of the instruction itself stays a model, oracle/ref_shim/mma.h).

The first group needs neither the reference tree nor the library.  The second runs the library live and skips only where the reference
tree is absent.
"""
import numpy as np
import pytest

import ref_kernel_cases as rc
from oracle import ref_kernels as rk

FIX = rc.Fixture()
PAIRS = FIX.pairs()
IDS = ["%s-%s" % p for p in PAIRS]
# what lfi_oracle_np implements: everything the C oracle does
ORACLES = ["oracle_c", "oracle_np"]

_inputs = {}


def _lf(oracle_c, case):
    if case["name"] not in _inputs:
        _inputs[case["name"]] = rc.inputs(oracle_c, case)
        _inputs[case["name"]].setflags(write=False)
    return _inputs[case["name"]]


def _scalars(case):
    return float(np.float32(case["focus"])), float(np.float32(case["range"]))


def _oracle_output(o, case, kernel, lf):
    """What oracle module `o` computes for (case, kernel), from the fixture's parameter arrays."""
    focus, rng = _scalars(case)
    if kernel == "estimate":
        return o.focus_estimate(lf, FIX.array(case, "offsets"), FIX.array(case, "ids"), focus, rng, case["radius"])
    if kernel == "filter":
        return o.focus_filter(FIX.map_out(case, "estimate"), case["radius"])
    af = kernel.endswith("_af")
    # Standard::process<true> reads map 1, Tensors::process<true> map 0: the oracle takes the map its caller hands it, so the caller's
    # convention is part of what is checked — the fixture was made with both maps bound and they differ
    plane = (FIX.map_in(case, 1 if kernel == "std_af" else 0)) if af else None
    args = (lf, FIX.array(case, "focused"), FIX.array(case, "offsets"), FIX.array(case, "weights"))
    kw = dict(all_focus=af, map_plane=plane, focus=focus, rng=rng)
    if kernel.startswith("std"):
        return o.blend_std(*args, **kw)
    return o.blend_ten(*args, model=o.TEN_M16, **kw)


def _check(case, kernel, out, what):
    if kernel in ("estimate", "filter"):
        want = FIX.map_out(case, kernel)
        assert out.shape == want.shape
        diff = int((out != want).sum())
        assert diff == 0, (case["name"], kernel, what, "map differs from the reference's in %d bytes" % diff)
    else:
        FIX.check_views(case, kernel, out, what)


def test_fixture_file_covers_the_cases():
    """The file is the one the generator writes from CASES, within its size cap, and records where contraction is observable."""
    import os
    assert os.path.getsize(rc.FIXTURE) <= 300 * 1000
    assert [c["name"] for c in FIX.cases] == [c["name"] for c in rc.CASES]
    for got, want in zip(FIX.cases, rc.CASES):
        for k, v in want.items():
            assert got[k] == (list(v) if isinstance(v, tuple) else v), (want["name"], k)
    sensitive = [(c["name"], k) for c in FIX.cases for k in c["sensitive"]]
    assert any(k == "estimate" for _, k in sensitive) and any(k == "std_af" for _, k in sensitive)
    kernels = {k for _, k in PAIRS}
    assert kernels == {"std", "ten", "std_af", "ten_af", "estimate", "filter"}
    assert any(c["focus"] < 0 for c in FIX.cases) and any(c["range"] < 0 for c in FIX.cases)
    assert any(c["grid"][0] * c["grid"][1] == 256 for c in FIX.cases)
    for c in FIX.cases:
        if c["map_seeds"]:
            assert (FIX.array(c, "map0") != FIX.array(c, "map1")).mean() > 0.9
        for key in [k for k in FIX.arrays if k.startswith(c["name"] + ".") and (k.endswith(".map") or k[-5:-1] == ".map")]:
            assert len(np.unique(FIX.arrays[key])) >= 8, key


def test_fixture_parameters_are_the_host_functions(oracle_c, oracle_np):
    """The parameter arrays in the file are what both oracles' host functions give for the case's scalars (the host arithmetic is a
    restatement of src/interpolator.cu and stays one: DESIGN.md §6)."""
    for case in FIX.cases:
        (cols, rows), (W, H) = case["grid"], case["size"]
        for o in (oracle_c, oracle_np):
            se = o.interpret_trajectory(case["traj"], cols, rows)
            off, foc = o.offsets(se, cols, rows, W, H, case["aspect"], case["focus"])
            assert (off == FIX.array(case, "offsets")).all() and (foc == FIX.array(case, "focused")).all(), case["name"]
            assert (o.focus_map_ids(se, cols, rows) == FIX.array(case, "ids")).all(), case["name"]
        assert (oracle_c.weight_matrix_f16(se, cols, rows, 64, case["effect"]) == FIX.array(case, "weights")).all(), case["name"]
    e7 = FIX.case("g8x8_48x20_e7")
    w = FIX.array(e7, "weights")
    assert ((w & 0x7c00) == 0).any() and (w != 0).all(), "effect 7 is there for its subnormal fp16 weights"
    far = FIX.case("g8x8_48x20_e7_far")
    lf_w = far["size"][0]
    assert (np.abs(FIX.array(far, "focused")[:, 0]).max() > lf_w // 3), "focus 1.1 is there for samples beyond the image"


@pytest.mark.parametrize("which", ORACLES)
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_oracle_reproduces_the_reference_kernels(pair, which, request, oracle_c):
    """Every (case, kernel) of the file, by the C oracle and by its numpy twin: maps whole, views by SHA-256 plus views 0 and 63."""
    case, kernel = FIX.case(pair[0]), pair[1]
    o = request.getfixturevalue(which)
    _check(case, kernel, _oracle_output(o, case, kernel, _lf(oracle_c, case)), which)


def test_inputs_recipe_agrees_between_the_oracles(oracle_c, oracle_np):
    for case in FIX.cases[:1] + [FIX.case("g8x16_130x37_focus")]:
        assert (rc.inputs(oracle_np, case) == _lf(oracle_c, case)).all()
        if case["bands"]:
            lf = _lf(oracle_c, case)
            assert (lf[..., :3] % 16 == 0).all() and (lf[:, :, 60:100, :3] == 0).all() and (lf[:, :, :60, :3] == 64).all()


# ---- the live library -------------------------------------------------------------------------------------------------------

needs_tree = pytest.mark.skipif(not rk.tree_present(), reason="the reference tree is absent")


def _ref_output(case, kernel, lf, fused):
    cols, rows = case["grid"]
    focus, rng = _scalars(case)
    if kernel == "estimate":
        return rk.focus_estimate(lf, cols, rows, FIX.array(case, "offsets"), FIX.array(case, "ids"), focus, rng, case["radius"], fused=fused)
    if kernel == "filter":
        return rk.focus_filter(FIX.map_out(case, "estimate"), case["radius"], fused=fused)
    af = kernel.endswith("_af")
    fn = rk.blend_std if kernel.startswith("std") else rk.blend_ten
    maps = (FIX.map_in(case, 0), FIX.map_in(case, 1)) if af else (None, None)
    return fn(lf, cols, rows, FIX.array(case, "focused"), FIX.array(case, "offsets"), FIX.array(case, "weights"), af, maps[0], maps[1], focus, rng,
              fused=fused)


@needs_tree
def test_library_builds_where_the_tree_is():
    assert rk.available(build=True), "make -C oracle ref failed although the reference tree is present"


@needs_tree
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_live_library_reproduces_the_fixture(pair, oracle_c):
    """The library built now gives the recorded bytes; the non-contracting build differs exactly where the generator recorded it."""
    case, kernel = FIX.case(pair[0]), pair[1]
    lf = _lf(oracle_c, case)
    _check(case, kernel, _ref_output(case, kernel, lf, True), "live library")
    other = _ref_output(case, kernel, lf, False)
    want = FIX.map_out(case, kernel) if kernel in ("estimate", "filter") else None
    if want is not None:
        differs = bool((other != want).any())
    else:
        differs = bool((rc.view_hashes(other) != FIX.array(case, kernel + ".hashes")).any())
    assert differs == (kernel in case["sensitive"]), (pair, "the build without contraction", "differs" if differs else "agrees")


@needs_tree
def test_live_library_refuses_what_the_reference_cannot_do(oracle_c):
    case = FIX.case("g4x4_48x20")
    lf = _lf(oracle_c, case)
    args = (FIX.array(case, "focused"), FIX.array(case, "offsets"))
    w = FIX.array(case, "weights")
    with pytest.raises(rk.Refused, match="64 views"):
        rk.blend_std(lf, 4, 4, *args, w[:32])
    with pytest.raises(rk.Refused, match="32 focus-map images"):
        rk.focus_estimate(lf, 4, 4, args[1], FIX.array(case, "ids"), 0.0, 1.0, (10, 10))
    with pytest.raises(rk.Refused, match="under 10"):
        rk.focus_filter(np.zeros((20, 48, 4), np.uint8), (15, 9))
    with pytest.raises(rk.Refused, match="warps that are not whole"):
        rk.blend_ten(lf[:, :19], 4, 4, *args, w)
    with pytest.raises(rk.Refused, match="warps that are not whole"):
        rk.blend_ten(lf[:, :, :40], 4, 4, *args, w)
    with pytest.raises(rk.Refused, match="no multiple of 16"):
        rk.blend_ten(np.concatenate([lf, lf[:8]]), 4, 6, np.zeros((24, 2), np.int32), np.zeros((24, 2), np.float32), np.zeros((64, 24), np.uint16))
    with pytest.raises(rk.Refused, match="no multiple of 8"):
        rk.blend_std(lf[:12], 4, 3, args[0][:12], args[1][:12], np.ascontiguousarray(w[:, :12]))
    with pytest.raises(rk.Refused, match="at most 256"):
        n = 17 * 16
        rk.blend_std(np.zeros((n, 2, 16, 4), np.uint8), 17, 16, np.zeros((n, 2), np.int32), np.zeros((n, 2), np.float32), np.zeros((64, n), np.uint16))


@needs_tree
def test_selftest_binary_is_clean():
    """The driver with its own main under the host's address and undefined-behaviour sanitizers: one tiny case per kernel."""
    r = rk.selftest()
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ref-selftest: ok" in r.stdout
