"""CPU: the draw of tests/fuzz_cases.py::fuzz_flagged held to its conditions on the references alone, before tests/test_gpu_fuzz.py leans on it.

The fixed-seed cases show every listed image count, width and view count; the pixel budget and the two tile-walk cases hold; a range per
flag crosses a 64-view pass from an unaligned start.  No TEN_WM interval admits more than two values, and the share of two-valued bytes per
case — over the views the interval alone holds: the exact rows are demanded `==` (_rest) — stays under the project's caps (2 % up to 72
images, 6 % above: tests/inframe_ref.py, tests/linear_ref.py) for linear light, for in-frame on the `near` offsets and for the deep BYTES.  In-frame on the `wide` offsets (r = wall / den scales the bound: tens) and the deep CODES (two
more bits) are wider by their nature: their shares are printed, not capped — on those shapes STD `==`, the exact rows and the deep bytes
carry the check.  Each flag's reference differs from the flag-free oracle on the case, so a render that lost its flag cannot pass: linear
light in more than 90 % of the bytes at which a linear-light and an encoded mean of the same samples lie a code apart (_means_apart: every
byte from 9 images on, about four fifths with 2 or 3).  The exact
rows' float32 value does not depend on the order of the images."""
import functools

import numpy as np
import pytest

import lfinterpolator_amd as L
import deep_ref
import fuzz_cases as fz
import inframe_ref
import linear_ref

DEEP, IN_FRAME, LINEAR = deep_ref.FLAG_DEEP_VIEWS, inframe_ref.FLAG_IN_FRAME, linear_ref.FLAG_LINEAR_LIGHT
FLAGS = [DEEP, IN_FRAME, LINEAR]
IDS = ["deep", "in_frame", "linear"]


def _cases(flag):
    return fz.flagged_cases(fz.FLAGGED_CASES, fz.FLAGGED_SEED[flag])


@functools.lru_cache(maxsize=None)
def _want(flag, i, which):
    from oracle import lfi_oracle_c as oc
    return fz.flagged_reference(L, oc, _cases(flag)[i], flag, which)


def _cap(case):
    return 0.06 if case["cols"] * case["rows"] > 72 else 0.02


def test_the_flags_are_the_headers():
    assert (DEEP, IN_FRAME, LINEAR) == (L.LFI_FLAG_DEEP_VIEWS, L.LFI_FLAG_IN_FRAME, L.LFI_FLAG_LINEAR_LIGHT)
    assert set(fz.FLAGGED_KERNEL) == set(fz.FLAGGED_SETS) == set(fz.FLAGGED_SEED) == set(FLAGS)


@pytest.mark.parametrize("flag", FLAGS, ids=IDS)
def test_the_fixed_seed_cases_show_every_listed_value_within_the_budget(flag):
    cases = _cases(flag)
    assert cases[0]["offsets"]["wide"].tobytes() == _cases(flag)[0]["offsets"]["wide"].tobytes(), "not reproducible"
    drawn, walk = cases[:fz.FLAGGED_CASES], cases[fz.FLAGGED_CASES:]
    assert len(drawn) == 24 and len(walk) == 2
    assert {c["cols"] * c["rows"] for c in drawn} == {2, 3, 9, 17, 32, 33, 48, 64, 65, 80, 129, 225} == {a * b for a, b in fz.FLAGGED_GRIDS}
    assert {c["W"] for c in drawn} == {1, 4, 7, 8, 9, 31, 64, 100, 127, 128, 129, 191, 257, 300} == set(fz.FLAGGED_WIDTHS)
    assert {c["V"] for c in drawn} == {1, 3, 15, 16, 17, 64, 65, 129, 150} == set(fz.FLAGGED_VIEWS)
    assert all(1 <= c["H"] <= 6 and c["V"] * c["W"] * c["H"] <= fz.FLAGGED_BUDGET == 120_000 for c in drawn)
    assert sum(c["H"] == 1 for c in drawn) >= 2
    assert [(c["W"], c["H"], c["V"], c["cols"] * c["rows"]) for c in walk] == [(300, 200, 2, 17), (64, 1100, 3, 33)]
    assert all((c["W"] + 127) // 128 * c["H"] > 512 for c in walk)
    for i, c in enumerate(cases):
        n, W, H = c["cols"] * c["rows"], c["W"], c["H"]
        assert c["reach"]["wide"] == [(0, 0), (1, 1), (9, 2), (W - 1, H - 1), (W + 5, H + 2)][i % 5]
        assert c["reach"]["near"] == (max(1, W // 4 if n >= 9 else W // 16), H // 4)     # narrowed below 9 images: fuzz_cases.flagged_near
        for which, (ax, ay) in c["reach"].items():
            o = c["offsets"][which]
            assert o.shape == (n, 2) and np.abs(o[:, 0]).max() <= ax and np.abs(o[:, 1]).max() <= ay
        k = min(c["V"], 3)
        assert len(set(c["exact_views"])) == k == len(c["exact_images"]) and all(0 <= v < c["V"] for v in c["exact_views"])
        assert [len(g) for g in c["exact_images"]] == [1, 1, 2][:k] and (k < 2 or c["exact_images"][1] == (n - 1,))
        assert k < 3 or c["exact_images"][2][0] != c["exact_images"][2][1]
        assert 0 <= c["v0"] < c["v1"] <= c["V"]
    # offsets beyond the frame occur, and so does every kind of `wide`
    assert any(np.abs(c["offsets"]["wide"][:, 0]).max() >= c["W"] for c in cases)
    # a range that starts unaligned and needs a second 64-view pass, which then starts at v0 + 64; half of those that could
    # (65 views have no room for one: v0 >= 1 leaves 64)
    room = [c for c in drawn if c["V"] > 65]
    crossing = [c for c in room if c["v0"] % 16 != 0 and c["v1"] - c["v0"] > 64]
    assert len(crossing) >= 2 and 2 * len(crossing) >= len(room), (len(crossing), len(room))
    # three passes in one launch (one chunk of images) and three launches of several chunks
    assert any(c["V"] > 128 and c["cols"] * c["rows"] <= 64 for c in drawn) and any(c["V"] > 128 and c["cols"] * c["rows"] > 64 for c in drawn)


def _rest(case):
    """the views whose weights are the trajectory's: those the interval alone holds.  (The exact rows are demanded `==`; their sums are whole
    or half numbers, which sit on the steps of q, so up to every byte of theirs admits two values, and one-hot rows render the input itself
    whatever the flag.)  Cases of one or three views have none: the exact rows and STD `==` carry them"""
    return [v for v in range(case["V"]) if v not in case["exact_views"]]


def _means_apart(want, rest):
    """[rest][H][W][3] bool: the bytes at which a linear-light mean and an encoded mean of the same samples CAN differ — the share of differing
    bytes is measured on these.  With samples b_g of weighted mean m and weighted variance s² (weights normalised), the mean taken in linear
    light, encoded again, lies above m by (γ − 1)·s² / (2·m) codes to second order (γ = 2.4).  Where that is under one code — two or three
    samples that happen to lie close together, a row that rests on one image — both renders round to the same byte whatever the flag, and
    such a byte says nothing about it.  From 9 images on no byte is left out; with 2 or 3 images about a fifth are"""
    w = linear_ref.weights_f32(want.hp.weights).astype(np.float64)[rest]
    w /= w.sum(axis=1, keepdims=True)
    b = linear_ref.samples(want.lf, want.hp.focused_offsets).astype(np.float64)
    m = np.einsum("vn,nhwc->vhwc", w, b)
    var = np.einsum("vn,nhwc->vhwc", w, b * b) - m * m
    return 1.4 * var >= 2.0 * np.maximum(m, 1.0)


def _what(c, which):
    return f"case {c['i']} ({c['cols'] * c['rows']} images, {c['W']}x{c['H']}, {c['V']} views) {which}"


@pytest.mark.parametrize("flag", FLAGS, ids=IDS)
def test_no_interval_admits_more_than_two_values_and_the_share_on_the_interval_held_views_is_capped(flag, oracle_c, native):
    """the width on every byte of every case; the two-valued share over the views the interval alone holds (_rest): every case of more than
    three views has one, and every one of them is capped but in-frame on `wide`"""
    capped = 0
    for c in _cases(flag):
        rest = _rest(c)
        for which in fz.FLAGGED_SETS[flag]:
            want, what = _want(flag, c["i"], which), _what(c, which)
            lo, hi = want.lo.astype(int), want.hi.astype(int)
            assert (hi >= lo).all() and (hi - lo).max() <= 1, (what, int((hi - lo).max()))
            rows = c["exact_views"]
            assert ((want.exact >= want.lo[rows]) & (want.exact <= want.hi[rows])).all(), what     # the exact rows lie inside their own intervals
            if flag == DEEP:
                lo10, hi10 = want.lo10.astype(int), want.hi10.astype(int)
                assert (hi10 >= lo10).all() and (hi10 - lo10).max() <= 1, (what, int((hi10 - lo10).max()))
                assert ((want.exact10 >= want.lo10[rows]) & (want.exact10 <= want.hi10[rows])).all(), what
            if not rest:
                continue
            share = float((hi[rest] != lo[rest]).mean())
            if flag == DEEP:
                print(f"{what}: two-valued deep bytes {share:.4f}, codes {float((hi10[rest] != lo10[rest]).mean()):.4f} (the codes: not capped)")
            elif flag == IN_FRAME and which == "wide":
                print(f"{what}: two-valued in-frame bytes {share:.4f} (not capped), largest r {float(want.res.r[rest].max()):.1f}")
                continue
            else:
                print(f"{what}: two-valued bytes {share:.4f}")
            assert share <= _cap(c), (what, share, _cap(c))
            capped += 1
    # exactly the cases that have such views (the tile-walk cases and the drawn cases of one or three views have exact rows only)
    assert capped == sum(c["V"] > 3 for c in _cases(flag)) >= 17


@pytest.mark.parametrize("flag", FLAGS, ids=IDS)
def test_a_render_that_lost_its_flag_cannot_pass(flag, oracle_c, native):
    oc = oracle_c
    told = 0
    for c in _cases(flag):
        rest, n = _rest(c), c["cols"] * c["rows"]
        for which in fz.FLAGGED_SETS[flag]:
            want, what = _want(flag, c["i"], which), _what(c, which)
            hp = want.hp
            plain = oc.blend_std(want.lf, hp.focused_offsets, hp.offsets, hp.weights, threads=8)[..., :3]
            if flag == LINEAR:
                one_hot = [v for v, g in zip(c["exact_views"], c["exact_images"]) if len(g) == 1]
                assert (want.std[one_hot] == plain[one_hot]).all()     # E(D[b]) = b: a one-hot view is the input under either render
                if rest:
                    apart = _means_apart(want, rest)
                    differ, share = float((want.std[rest] != plain[rest])[apart].mean()), float(apart.mean())
                    print(f"{what}: linear-light bytes that differ from the encoded render's: {differ:.4f} of the {share:.4f} whose two means lie a code apart")
                    assert differ > 0.90, (what, differ)
                    # the measured bytes are all of them from 9 images on, and most of them with 2 or 3
                    assert share > (0.99 if n >= 9 else 0.50), (what, share)
                    told += 1
            elif flag == IN_FRAME:
                # the restatement with every mask full IS the flag-free render; where a weighted sample is out of frame, some byte differs
                assert (inframe_ref.restate(want.lf, hp, force_full=True).bytes == plain).all(), what
                out = ~inframe_ref.in_frame(hp.focused_offsets, c["W"], c["H"])                 # [N][H][W]
                weighted = inframe_ref.weights_f32(hp.weights) > 0                                # [V][N]
                if (weighted[:, :, None, None] & out[None]).any():
                    assert (want.std != plain).any(), (what, "weighted samples out of frame and the same bytes")
                    told += 1
                else:
                    assert (want.std == plain).all(), what
            else:
                assert (want.std == plain).all(), what                 # the 8-bit bytes are the flag-free bytes: the codes are what the flag adds
                assert (np.abs(want.codes.astype(int) - 4 * plain.astype(int)) <= 2).all(), what
                if rest:
                    assert (want.codes[rest] & 3 != 0).any(), (what, "every code is four times a byte")
                    told += 1
    assert told >= (30 if flag == IN_FRAME else 17), told


@pytest.mark.parametrize("flag", [IN_FRAME, LINEAR], ids=IDS[1:])
def test_the_exact_rows_do_not_depend_on_the_order_of_the_images(flag, oracle_c, native):
    """one-hot and half/half rows: every product and partial sum is exact in fp32, so the float32 restatement's chain — ascending images — gives
    the value any order gives.  Shown by permuting the images (with their offsets and weight columns)"""
    restate = inframe_ref.restate if flag == IN_FRAME else linear_ref.restate
    for c in _cases(flag):
        for which in fz.FLAGGED_SETS[flag]:
            want = _want(flag, c["i"], which)
            hp, rows = want.hp, c["exact_views"]
            perm = np.random.default_rng(c["lf_seed"]).permutation(want.lf.shape[0])
            shuffled = L.host.HostParams(np.ascontiguousarray(hp.focused_offsets[perm]), np.ascontiguousarray(hp.offsets[perm]),
                                         np.ascontiguousarray(hp.weights[rows][:, perm]), hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)
            again = restate(np.ascontiguousarray(want.lf[perm]), shuffled)
            assert (again.s == want.res.s[rows]).all() and (again.bytes == want.res.bytes[rows]).all(), (c["i"], which)
            assert (again.S == want.res.S[rows]).all()
