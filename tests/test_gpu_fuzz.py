"""GPU (-m gpu): the randomised parity cases of tests/fuzz_cases.py with FIXED seeds and a bounded number of cases each — the soak
tools of round 2 (tools/fuzz_*.py) brought under pytest: STD and focus maps bit-exact against the oracle, TEN_WM within one LSB of
M16, on random shapes around the tile and chunk sizes, both view layouts, the main kernel variants; the flagged fixed-focus renders (deep
views, in-frame, linear light) on a stratified draw, each against its own reference.  One process, one context at a time."""
import pytest

import fuzz_cases

pytestmark = pytest.mark.gpu


def _oracle():
    from oracle import lfi_oracle_c as oc
    oc.build()
    return oc


def test_fuzz_fixed_focus_blend(gpu):
    bad = fuzz_cases.fuzz_blend(gpu, _oracle(), n_cases=40, seed=1)
    assert not bad, bad[:5]


def test_fuzz_focus_maps(gpu):
    bad = fuzz_cases.fuzz_focus(gpu, _oracle(), n_cases=40, seed=1, log=print)   # (the leaves of tests/focus_routes.py the seed reaches)
    assert not bad, bad[:5]


def test_fuzz_all_focus_renders(gpu):
    bad = fuzz_cases.fuzz_allfocus(gpu, _oracle(), n_cases=40, seed=3)
    assert not bad, bad[:5]


def test_fuzz_view_rows(gpu):
    bad = fuzz_cases.fuzz_view_rows(gpu, _oracle(), n_cases=24, seed=5)
    assert not bad, bad[:5]


# the flagged fixed-focus renders: 24 stratified cases and the two tile-walk cases each; tests/test_fuzz_flagged_table.py holds the same
# fixed-seed draws to their conditions on the CPU.  Measured beside test_fuzz_view_rows (0.21 s): linear light 0.5 s, deep views 0.8 s,
# in-frame 1.3–1.7 s, references included — over it, and no faster at a third of the pixel budget: what they cost is per view

def _fuzz_flagged(gpu, flag):
    bad = fuzz_cases.fuzz_flagged(gpu, _oracle(), flag, n_cases=fuzz_cases.FLAGGED_CASES, seed=fuzz_cases.FLAGGED_SEED[flag], log=print)
    assert not bad, (len(bad), bad[:5])


def test_fuzz_deep_views(gpu):
    _fuzz_flagged(gpu, gpu.LFI_FLAG_DEEP_VIEWS)


def test_fuzz_in_frame(gpu):
    _fuzz_flagged(gpu, gpu.LFI_FLAG_IN_FRAME)


def test_fuzz_linear_light(gpu):
    _fuzz_flagged(gpu, gpu.LFI_FLAG_LINEAR_LIGHT)
