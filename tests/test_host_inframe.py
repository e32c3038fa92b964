"""CPU: in-frame blending (LFI_FLAG_IN_FRAME) on the restatement (tests/inframe_ref.py) and the oracle alone — that the restatement is tied to the
pinned oracle, that the renders tests/test_gpu_inframe.py checks tell an in-frame render from a clamped one, that the TEN_WM interval is tight
enough to mean something, the constants, the program's usage errors, and the code object."""
import re

import numpy as np
import pytest

import code_object
import inframe_ref as ref
import ten_interval
from view_rows import run_cli


# ---- the restatement against the oracle -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [ref.CASES[0], ref.CASES[2], ref.CASES[3], ref.CASES[6]], ids=lambda c: c[0])
def test_masks_forced_full_give_the_oracles_chain(case, native, oracle_c):
    """every sample counted: den is wall bit for bit, r = 1, and bytes and pre-quantisation values are oracle_c.blend_std's"""
    hp, lf = ref.inputs(native, oracle_c, case)
    res = ref.restate(lf, hp, force_full=True)
    want, pre = oracle_c.blend_std(lf, hp.focused_offsets, hp.offsets, hp.weights, return_prequant=True)
    assert (res.den == res.wall[:, None, None]).all() and (res.r == 1.0).all()
    assert (res.s.view(np.uint32) == pre.view(np.uint32)).all()
    assert (res.bytes == want[..., :3]).all()


def test_offsets_zero_give_the_oracles_chain(native, oracle_c):
    case = ref.CASES[2]
    hp, lf = ref.inputs(native, oracle_c, case)
    hp0 = native.host.HostParams(hp.focused_offsets * 0, hp.offsets, hp.weights, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius)
    res = ref.restate(lf, hp0)
    want, pre = oracle_c.blend_std(lf, hp0.focused_offsets, hp0.offsets, hp0.weights, return_prequant=True)
    assert res.all_in.all() and (res.r == 1.0).all()
    assert (res.s.view(np.uint32) == pre.view(np.uint32)).all() and (res.bytes == want[..., :3]).all()


@pytest.mark.parametrize("case", ref.CASES, ids=ref.CASE_IDS)
def test_in_frame_bytes_differ_from_the_clamped_ones_at_the_border(case, native, oracle_c):
    """without this the GPU tests would pass on a library that ignores the flag: of the border bytes (at least one image out of frame) more than
    20 % differ from the clamped oracle's; where every image is in frame none does"""
    hp, lf = ref.inputs(native, oracle_c, case)
    res = ref.restated(native, oracle_c, case)
    clamped = oracle_c.blend_std(lf, hp.focused_offsets, hp.offsets, hp.weights)[..., :3]
    border = ~res.all_in
    assert border.any() and (res.bytes[:, res.all_in] == clamped[:, res.all_in]).all()
    share = float((res.bytes[:, border] != clamped[:, border]).mean())
    print(case[0], f"border bytes: {100 * border.mean():.1f} % of the frame; in-frame != clamped in {100 * share:.1f} % of them")
    assert share > 0.20, (case[0], share)
    assert (res.bytes[:, res.none_in] == 0).all()
    if case is ref.NONE_IN_FRAME:
        assert res.none_in[:, 4:20].all() and not res.none_in[:, :4].any() and not res.none_in[:, 20:].any()


@pytest.mark.parametrize("case", ref.CASES, ids=ref.CASE_IDS)
def test_no_border_byte_admits_more_than_two_values(case, native, oracle_c):
    hp, lf = ref.inputs(native, oracle_c, case)
    res = ref.restated(native, oracle_c, case)
    lo, hi = ref.ten_interval_of(res, hp, lf.shape[0])
    width = hi.astype(int) - lo.astype(int)
    border = ~res.all_in
    share = float((width[:, border] > 0).mean())
    print(case[0], f"border bytes with two admissible values: {100 * share:.2f} % (cap {100 * ref.TWO_VALUED_CAP[case[0]]:.0f} %), widest interval {int(width.max())}")
    assert width.min() >= 0 and width[:, border].max() <= 1, (case[0], int(width[:, border].max()))
    assert share <= ref.TWO_VALUED_CAP[case[0]], (case[0], share)
    # where every image is in frame the interval is the ordinary TEN_WM one
    plo, phi = ten_interval.bounds(oracle_c, lf, hp)
    assert (lo[:, res.all_in] == plo[:, res.all_in]).all() and (hi[:, res.all_in] == phi[:, res.all_in]).all()


def test_dyadic_weights_need_no_interval(native, oracle_c):
    hp, lf = ref.dyadic(native, oracle_c)
    res = ref.restate(lf, hp)
    lo, hi = ref.ten_interval_of(res, hp, lf.shape[0])
    exact = ref.ten_exact(res)
    assert ((exact >= lo) & (exact <= hi)).all()
    # every sum is a multiple of 2^-6 below 2^14: float32 holds it whatever the order
    assert (res.num.astype(np.float64) == res.S).all()


# ---- the constants ---------------------------------------------------------------------------------------------------------------------------

def test_the_flag_is_bit_128_in_the_header_the_binding_and_the_export(native):
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lfi.h")).read()
    assert re.search(r"\bLFI_FLAG_IN_FRAME = 128u\b", header)
    assert native.abi.LFI_FLAG_IN_FRAME == 128 and native.LFI_FLAG_IN_FRAME == 128 and ref.FLAG_IN_FRAME == 128
    assert "LFI_FLAG_IN_FRAME" in native.__all__


# ---- the command line ------------------------------------------------------------------------------------------------------------------------

ARGS = ["--synthetic", "3,3,16,8", "-t", "0,0,1,1", "-m", "TEN_WM", "-n", "4", "-b", "1", "-f", "0.2"]


def test_cli_help_names_the_option(native):
    res = run_cli(native, "-h")
    assert res.returncode == 0
    for word in ("--edges clamp|in-frame", "leaves the sample out"):
        assert word in res.stdout, word


@pytest.mark.parametrize("extra,word", [
    (["-r", "0.3"], "-r above 0"),
    (["-F", "0.4"], "-F"),
    (["-c"], "-c (view-centred"),
    (["-c", "-r", "0.3", "--view-maps"], "cannot be combined"),
    (["--deep"], "--deep"),
    (["-g", "2"], "-g above 1"),
])
def test_cli_usage_errors_come_back_without_a_gpu(native, tmp_path, extra, word):
    res = run_cli(native, *ARGS, "-o", str(tmp_path / "out"), "--edges", "in-frame", *extra)
    assert res.returncode != 0 and "--edges in-frame" in res.stderr and word in res.stderr, (res.stdout, res.stderr)
    assert not (tmp_path / "out").exists()


def test_cli_edges_takes_clamp_or_in_frame(native, tmp_path):
    res = run_cli(native, *ARGS, "-o", str(tmp_path / "out"), "--edges", "mirror")
    assert res.returncode != 0 and "--edges expects clamp or in-frame" in res.stderr
    assert not (tmp_path / "out").exists()


# ---- the code object -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not code_object.have_tools(), reason="ROCm LLVM tools not installed")
def test_inframe_kernels_exist_and_fit(native):
    """blend_inframe twice (STD, TEN_WM): no scratch, no spills; the TEN_WM one on the matrix cores, the STD one not; both divide (the
    correctly rounded sequence, not a bare reciprocal) and fetch by LDS-DMA"""
    kernels = code_object.kernels(native.build.HIP_LIB)
    bodies = code_object.bodies(native.build.HIP_LIB)
    found = code_object.named(kernels, "blend_inframe")
    assert len(found) == 2, sorted(found)
    for k, r in found.items():
        assert r[".private_segment_fixed_size"] == 0 and r[".vgpr_spill_count"] == 0 and r[".sgpr_spill_count"] == 0, (k, r)
        assert "scratch_" not in bodies[k], k
        assert "global_load_lds_dwordx4" in bodies[k] and "v_div_fixup_f32" in bodies[k], k
    blends = code_object.named(bodies, "blend_inframe")
    ten = [k for k in blends if "ILb0E" in k][0]
    std = [k for k in blends if "ILb1E" in k][0]
    assert "v_mfma_f32_16x16x32_f16" in blends[ten] and "v_mfma" not in blends[std]
    assert any(op in blends[std] for op in ("v_pk_fma_f32", "v_fma_f32", "v_fmac_f32"))
    assert len(code_object.named(kernels, "deep_blend")) == 2   # what an existing test counts
