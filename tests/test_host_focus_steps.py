"""CPU: the numpy restatement of the fine focus map (tests/focus_steps_ref.py) anchored to the committed oracle at 32 steps, the planted scene
at 128 steps that the GPU test uploads, and the command line's checks of --map-steps (made before any device is opened)."""
import dataclasses

import numpy as np
import pytest

import focus_curve_ref as cref
import focus_steps_ref as ref
from conftest import SMALL_CASES
from view_rows import run_cli

GOLDEN = {c[0]: c for c in SMALL_CASES}


def golden_case(native, oracle_c, name, rng):
    """a conftest.SMALL_CASES light field with a focusing range: (hp, lf)"""
    _, cols, rows, W, H, V, traj, focus, aspect, effect = GOLDEN[name]
    hp = native.build_params(cols, rows, W, H, traj, focus, rng, effect, aspect, V)
    return hp, oracle_c.synthetic_lf(cols * rows, W, H, 0x1F1F)


# Eight fuzz cases (name, cols, rows, W, H, trajectory, focus, range, seed, block radius or None for build_params' own).  Between them: centred
# trajectories (images on either side of the camera: negative shifts, so flagged rows and columns on both axes), even and odd radius_x, and a
# radius_x above 64, where focus_pick_sep does not apply.  The sizes are those of tests/test_gpu_focus_steps.py: 33 x 17, 32 x 24, 96 x 64.
FUZZ = [
    ("f0_3x3_33x17", 3, 3, 33, 17, "0,0,1,1", 0.1, 0.3, 11, None),
    ("f1_8x8_32x24", 8, 8, 32, 24, "0.3,0.6,0.5,0.1", 0.0, 0.5, 5, (2, 2)),
    ("f2_8x8_32x24_r3x1", 8, 8, 32, 24, "0.3,0.6,0.5,0.1", -0.2, 0.5, 6, (3, 1)),
    ("f3_4x4_96x64_r4x2", 4, 4, 96, 64, "0.071,0.071,0.93,0.93", 0.22, 0.17, 99, (4, 2)),
    ("f4_4x4_32x24_r66x3", 4, 4, 32, 24, "0.5,0.5,0.5,0.5", -0.3, 0.9, 7, (66, 3)),
    ("f5_5x2_33x17_r1x3", 5, 2, 33, 17, "1,0,0,1", 0.05, 0.4, 8, (1, 3)),
    ("f6_2x7_32x24_r6x1", 2, 7, 32, 24, "0.5,0.5,0.5,0.5", 0.6, -0.0 + 0.35, 9, (6, 1)),
    ("f7_15x15_33x17", 15, 15, 33, 17, "0,0.5,1,0.5", 0.23, 0.31, 10, (2, 1)),
]


def fuzz_case(native, oracle_c, case):
    _, cols, rows, W, H, traj, focus, rng, seed, radius = case
    hp = native.build_params(cols, rows, W, H, traj, focus, rng, 3.0, 1.783, 3)
    if radius is not None:
        hp = dataclasses.replace(hp, block_radius=np.array(radius, np.int32))
    return hp, oracle_c.synthetic_lf(cols * rows, W, H, seed)


def has_negative_shifts(hp):
    f = cref.candidates(hp.focus, hp.range, 32)
    o = hp.offsets[hp.focus_map_ids]
    return bool((np.outer(f, o[:, 0]) < 0).any() and (np.outer(f, o[:, 1]) < 0).any())


def test_the_fuzz_cases_cover_what_they_claim(native, oracle_c):
    hps = [fuzz_case(native, oracle_c, c)[0] for c in FUZZ]
    assert sum(has_negative_shifts(hp) for hp in hps) >= 4
    rx = [int(hp.block_radius[0]) for hp in hps]
    assert any(r % 2 == 0 for r in rx) and any(r % 2 == 1 for r in rx) and any(r > 64 for r in rx)
    assert {(c[3], c[4]) for c in FUZZ} == {(33, 17), (32, 24), (96, 64)}


def black_scene(native, oracle_c):
    """g4x4_33x17 sampled at two images that both show one pattern of flat 6 x 6-pixel cells, black or grey: wherever both images' samples of
    a tap fall into cells of one colour the tap's range is 0, so many pixels have S = 0 at several candidates — and the number of all-zero
    taps (FLT_MIN taps: the black ones, never the grey ones) differs between those candidates, because their shifts reach other cells"""
    hp, _ = golden_case(native, oracle_c, "g4x4_33x17_v5", 0.25)
    hp = dataclasses.replace(hp, focus_map_ids=np.ascontiguousarray(hp.focus_map_ids[:2]))
    _, cols, rows, W, H = GOLDEN["g4x4_33x17_v5"][:5]
    cells = np.random.RandomState(4).randint(0, 2, size=(H // 6 + 1, W // 6 + 1)).astype(np.uint8) * 90
    lf = np.empty((cols * rows, H, W, 4), np.uint8)
    lf[..., :3] = np.kron(cells, np.ones((6, 6), np.uint8))[None, :H, :W, None]
    lf[..., 3] = 255
    return hp, lf


def _oracle(oracle_c, hp, lf):
    return oracle_c.focus_estimate(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)


@pytest.mark.parametrize("name,rng", [("g4x4_33x17_v5", 0.25), ("g15x15_16x16_v8", 0.4)])
def test_restatement_at_32_steps_is_the_oracle_on_the_golden_cases(native, oracle_c, name, rng):
    hp, lf = golden_case(native, oracle_c, name, rng)
    if name.startswith("g15x15"):
        assert len(hp.focus_map_ids) == 32          # 32 of 225 sampled
    got = ref.map0(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, 32)
    want = _oracle(oracle_c, hp, lf)
    assert (got == want).all(), int((got != want).sum())


@pytest.mark.parametrize("case", FUZZ, ids=[c[0] for c in FUZZ])
def test_restatement_at_32_steps_is_the_oracle_on_the_fuzz_cases(native, oracle_c, case):
    hp, lf = fuzz_case(native, oracle_c, case)
    got = ref.map0(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, 32)
    want = _oracle(oracle_c, hp, lf)
    assert (got == want).all(), int((got != want).sum())


def test_restatement_at_32_steps_is_the_oracle_where_the_zero_sum_rule_decides(native, oracle_c):
    hp, lf = black_scene(native, oracle_c)
    key, zero = ref.keys(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, 32)
    best = ref.winners(key)
    won_by_rule = np.take_along_axis(zero, best[None], axis=0)[0]          # the winner's key came from the S = 0 rule …
    several = zero.sum(axis=0) >= 2                                        # … and had another zero-sum candidate to beat
    differing = np.array([len(set(key[:, y, x][zero[:, y, x]])) > 1 for y, x in zip(*np.nonzero(several))])
    assert (won_by_rule & several).sum() >= 1 and differing.any(), (int(won_by_rule.sum()), int(several.sum()))
    got = ref.map0(lf, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, 32)
    want = _oracle(oracle_c, hp, lf)
    assert (got == want).all(), int((got != want).sum())


# ---- the planted scene at 128 steps ------------------------------------------------------------------------------------------------------
# focus_curve_ref.PLANTED with 128 candidates: the texture is planted at candidate k of 128.  Neighbouring fine candidates can give every image
# the same integer shifts, so the winner is the FIRST candidate equivalent to k, not necessarily k.
#
# PLANTED's texture has flat cells of 8 x 8 pixels.  A pixel whose nine taps stay inside one cell under an EARLIER candidate's (smaller)
# shifts has S = 0 there too, and that candidate wins it: a flat patch has no focus.  So on PLANTED the per-pixel statement "the winner's shifts
# are k's" holds for the pixels near a cell border only — checked below as: every winner is <= k with S = 0, every pixel NOT won by an
# equivalent candidate is such a flat patch (all nine taps of all images one colour at the winner), and the first equivalent candidate wins
# more pixels of every region than any other candidate.  The statement as it stands, for EVERY pixel, is checked on the same scene with a texel per pixel (`fine_planted`),
# where no patch is flat.

PLANTED_128 = dict(cref.PLANTED, steps=128)
# k = 37 and 93.  (Not 90: candidates 90 and 91 of 128 share all shifts and candidate 90's map byte, 181, is also candidate 22 of 32's — the two
# maps would not differ there.  93 is equivalent to 92, whose byte 185 no candidate of 32 has.)
PLANTED_KS = (37, 93)


def planted(native, k, steps=128):
    P = dict(cref.PLANTED, steps=steps)
    hp = native.build_params(P["cols"], P["rows"], P["W"], P["H"], P["traj"], P["focus"], P["rng"], 3.0, 1.0, 2)
    return hp, cref.planted_scene(hp.offsets, k, **P)


def fine_planted(native, k, steps=128):
    """planted_scene with one random texel per pixel instead of 8 x 8 cells: image g shows T(x - sx_g, y - sy_g), (sx_g, sy_g) the shift at f_k"""
    P = dict(cref.PLANTED, steps=steps)
    hp = native.build_params(P["cols"], P["rows"], P["W"], P["H"], P["traj"], P["focus"], P["rng"], 3.0, 1.0, 2)
    f_k = cref.candidates(P["focus"], P["rng"], steps)[k]
    reach = int(np.ceil(np.abs(hp.offsets).max() * max(abs(P["focus"]), abs(P["focus"] + P["rng"])))) + 8
    W, H = P["W"], P["H"]
    texels = np.random.RandomState(P["seed"] + k).randint(0, 256, size=(H + 2 * reach, W + 2 * reach, 3)).astype(np.uint8)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    lf = np.empty((P["cols"] * P["rows"], H, W, 4), np.uint8)
    lf[..., 3] = 255
    for g in range(len(lf)):
        sx, sy = ref.shifts(hp.offsets, [g], f_k)[0]
        lf[g, ..., :3] = texels[ys - sy + reach, xs - sx + reach]
    return hp, lf


def _equivalent(hp, f, k):
    at_k = ref.shifts(hp.offsets, hp.focus_map_ids, f[k])
    return np.array([(ref.shifts(hp.offsets, hp.focus_map_ids, fi) == at_k).all() for fi in f])


@pytest.mark.parametrize("k", PLANTED_KS)
def test_planted_scene_at_128_steps_is_won_by_a_candidate_equivalent_to_the_planted_one(native, k):
    P = PLANTED_128
    hp, lf = planted(native, k)
    key, zero = ref.keys(lf, hp.offsets, hp.focus_map_ids, P["focus"], P["rng"], hp.block_radius, 128)
    best = ref.winners(key)
    fine = ref.map0(lf, hp.offsets, hp.focus_map_ids, P["focus"], P["rng"], hp.block_radius, 128, key=key)
    coarse = ref.map0(lf, hp.offsets, hp.focus_map_ids, P["focus"], P["rng"], hp.block_radius, 32)
    f = cref.candidates(P["focus"], P["rng"], 128)
    equivalent = _equivalent(hp, f, k)
    assert equivalent[k] and equivalent.sum() < 128
    for x0, y0, x1, y1 in cref.PLANTED_REGIONS:
        won = best[y0:y1, x0:x1]
        assert (won <= k).all(), (k, np.unique(won))
        assert np.take_along_axis(zero, best[None], axis=0)[0, y0:y1, x0:x1].all()       # S = 0 at every winner, as at k
        by_equivalent = equivalent[won]
        assert np.bincount(won.ravel()).argmax() == np.argmax(equivalent), (k, np.bincount(won.ravel()))
        assert (won[by_equivalent] == np.argmax(equivalent)).all()                          # the FIRST equivalent candidate
        # the extra candidates carry information: where an equivalent candidate wins, the 32-step map cannot name this focus
        assert (coarse[y0:y1, x0:x1, 0][by_equivalent] != fine[y0:y1, x0:x1, 0][by_equivalent]).all(), k


@pytest.mark.parametrize("k", PLANTED_KS)
def test_planted_texels_at_128_steps_every_pixel_is_won_by_an_equivalent_candidate(native, k):
    P = PLANTED_128
    hp, lf = fine_planted(native, k)
    fine, best = ref.map0(lf, hp.offsets, hp.focus_map_ids, P["focus"], P["rng"], hp.block_radius, 128, with_index=True)
    coarse = ref.map0(lf, hp.offsets, hp.focus_map_ids, P["focus"], P["rng"], hp.block_radius, 32)
    f = cref.candidates(P["focus"], P["rng"], 128)
    at_k = ref.shifts(hp.offsets, hp.focus_map_ids, f[k])
    for x0, y0, x1, y1 in cref.PLANTED_REGIONS:
        won = np.unique(best[y0:y1, x0:x1])
        assert (won <= k).all(), (k, won)
        for i in won:
            assert (ref.shifts(hp.offsets, hp.focus_map_ids, f[i]) == at_k).all(), (k, int(i))
        assert (coarse[y0:y1, x0:x1, 0] != fine[y0:y1, x0:x1, 0]).all(), (k, np.unique(coarse[y0:y1, x0:x1, 0]), np.unique(fine[y0:y1, x0:x1, 0]))


# ---- the command line ---------------------------------------------------------------------------------------------------------------------

MAP_STEPS_ARGS = ["--synthetic", "4,4,32,16", "-t", "0,0,1,1", "-m", "STD", "-n", "4", "-b", "1", "-f", "0.0"]


@pytest.mark.parametrize("extra", [["-r", "0.5", "--map-steps", "100"], ["-r", "0.5", "--map-steps", "0"], ["-r", "0.5", "--map-steps", "288"],
                                   ["-r", "0.5", "-c", "--map-steps", "64", "--view-maps"], ["-r", "0.5", "--map-steps", "64", "--autofocus"],
                                   ["--map-steps", "64"]],
                         ids=["100", "0", "288", "--view-maps", "--autofocus", "no -r"])
def test_cli_refuses_map_steps_it_cannot_serve(native, tmp_path, extra):
    res = run_cli(native, *MAP_STEPS_ARGS, *extra, "-o", str(tmp_path / "out"))
    assert res.returncode != 0
    assert "--map-steps" in res.stderr
    assert not (tmp_path / "out").exists()
