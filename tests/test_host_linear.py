"""CPU: linear-light blending (LFI_FLAG_LINEAR_LIGHT) on the restatement (tests/linear_ref.py), the library's tables and epilogue (csrc/linear_light.h
through the host library) and the oracle alone — that the committed bit patterns are the formulas' values, that the restatement is tied to the pinned
oracle, that the renders tests/test_gpu_linear.py checks tell a linear-light render from an encoded one, that the TEN_WM interval is tight enough to
mean something, that the kernel's epilogue returns the definition's count for every fp32 input that matters, the constants, the program's usage
errors, and the code object."""
import os
import re

import numpy as np
import pytest

import code_object
import linear_ref as ref
import ten_interval
from view_rows import run_cli


# ---- the tables -------------------------------------------------------------------------------------------------------------------------------

def test_the_committed_bit_patterns_are_the_formulas_values(native):
    d, t = native.linear_tables()
    assert (d == ref.D16.view(np.uint16)).all(), np.flatnonzero(d != ref.D16.view(np.uint16))
    assert (t[1:] == ref.T32.view(np.uint32)).all(), np.flatnonzero(t[1:] != ref.T32.view(np.uint32)) + 1
    assert t[0] == 0
    assert ref.D16[0] == 0 and ref.D16[255] == 255


def test_the_tables_increase_and_the_round_trip_is_the_identity(native):
    D, T = ref.D16.astype(np.float64), ref.T32.astype(np.float64)
    assert (np.diff(D) > 0).all() and (np.diff(T) > 0).all()
    # T[b] <= D[b] < T[b + 1]
    assert (T <= D[1:]).all() and (D[:-1] < T).all()
    b = np.arange(256)
    assert (ref.encode(ref.D16.astype(np.float32)) == b).all()
    assert (native.linear_encode(ref.D16.astype(np.float32)) == b).all()
    # where D[b] stands in its bin [T[b], T[b + 1]): at least 0.46 of the bin's width from either edge (bins 1 ... 254: the two outer ones are open)
    pos = (D[1:255] - T[:-1]) / np.diff(T)
    print(f"D[b] in its bin: {pos.min():.4f} ... {pos.max():.4f}")
    assert pos.min() >= 0.46 and pos.max() <= 0.54
    # neighbouring thresholds are further apart than a sixteenth: what the epilogue's first guess rests on (csrc/linear_light.h)
    assert np.diff(T).min() > 1.0 / 16 and T[0] < 1.0 / 16


def _tie_margin(x, mant_bits, min_exp):
    """the distance of each x > 0 from the nearest rounding tie of a binary format with mant_bits explicit mantissa bits, relative to x"""
    e = np.maximum(np.floor(np.log2(x)), min_exp)
    ulp = np.ldexp(1.0, (e - mant_bits).astype(np.int64))
    frac = x / ulp - np.floor(x / ulp)
    return np.abs(frac - 0.5) * ulp / x


def test_the_rounding_margins_leave_pow_no_say():
    """no D[b] is nearer than 1.1e-6 (relative) to an fp16 tie and no T[b] nearer than 2.1e-10 to an fp32 tie: a pow that is off by a few ulps of a
    double (1e-16) gives the same bits"""
    d = _tie_margin(ref.decode_exact()[1:], 10, -14).min()
    t = _tie_margin(ref.threshold_exact()[1:], 23, -126).min()
    print(f"smallest margin: D {d:.3g}, T {t:.3g}")
    assert d > 1e-8 and t > 1e-11


# ---- the restatement against the oracle ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [ref.RAGGED, ref.TWO_CHUNKS_70], ids=lambda c: c[0])
def test_identity_tables_give_the_oracles_chain(case, native, oracle_c):
    """D[b] = b and E = rint & 0xff: bytes and pre-quantisation bits are oracle_c.blend_std's"""
    hp, lf = ref.inputs(native, oracle_c, case)
    res = ref.restate(lf, hp, identity=True)
    want, pre = oracle_c.blend_std(lf, hp.focused_offsets, hp.offsets, hp.weights, return_prequant=True)
    assert (res.s.view(np.uint32) == pre.view(np.uint32)).all()
    assert (res.bytes == want[..., :3]).all()


@pytest.mark.parametrize("case", ref.CASES, ids=ref.CASE_IDS)
def test_linear_bytes_differ_from_the_encoded_ones(case, native, oracle_c):
    """without this the GPU tests would pass on a library that ignores the flag: more than 90 % of the bytes differ from the flag-free oracle's"""
    hp, lf = ref.inputs(native, oracle_c, case)
    res = ref.restated(native, oracle_c, case)
    encoded = oracle_c.blend_std(lf, hp.focused_offsets, hp.offsets, hp.weights)[..., :3]
    diff = res.bytes.astype(int) - encoded.astype(int)
    share = float((diff != 0).mean())
    print(case[0], f"linear != encoded in {100 * share:.1f} % of the bytes; mean difference {np.abs(diff).mean():.1f} code values, linear brighter in "
          f"{100 * float((diff > 0).mean()):.1f} %")
    assert share > 0.90, (case[0], share)


@pytest.mark.parametrize("case", ref.CASES, ids=ref.CASE_IDS)
def test_no_byte_admits_more_than_two_values(case, native, oracle_c):
    hp, lf = ref.inputs(native, oracle_c, case)
    res = ref.restated(native, oracle_c, case)
    lo, hi = ref.ten_interval_of(res, hp, lf.shape[0])
    width = hi.astype(int) - lo.astype(int)
    share = float((width > 0).mean())
    print(case[0], f"bytes with two admissible values: {100 * share:.2f} % (cap {100 * ref.TWO_VALUED_CAP[case[0]]:.0f} %), widest interval {int(width.max())}")
    assert width.min() >= 0 and width.max() <= 1, (case[0], int(width.max()))
    assert share <= ref.TWO_VALUED_CAP[case[0]], (case[0], share)
    # the STD chain's own byte lies in the interval: its error is within the same bound
    assert ((res.bytes >= lo) & (res.bytes <= hi)).all()
    # the bound's premise: no partial sum reaches 512
    assert res.S.max() < 512.0


def test_exact_rows_need_no_interval_and_return_the_inputs_bytes(native, oracle_c):
    hp, lf = ref.exact_rows(native, oracle_c)
    res = ref.restate(lf, hp)
    px = ref.samples(lf, hp.focused_offsets)
    rows = [v for v, _ in ref.ONE_HOT] + [v for v, _, _ in ref.HALVES]
    assert (res.s[rows].astype(np.float64) == res.S[rows]).all()        # float32 holds these sums whatever the order
    for v, g in ref.ONE_HOT:
        assert (res.bytes[v] == px[g]).all()
    seen = np.unique(np.concatenate([res.bytes[v].ravel() for v, _ in ref.ONE_HOT]))
    assert len(seen) == 256                                             # the whole of D and E is exercised
    lo, hi = ref.ten_interval_of(res, hp, lf.shape[0])
    assert ((res.bytes >= lo) & (res.bytes <= hi)).all()


# ---- the epilogue -------------------------------------------------------------------------------------------------------------------------------

def test_the_kernels_epilogue_is_the_definitions_count(native):
    """csrc/linear_light.h's linear_encode — a first guess from the table of sixteenths, one comparison — against the count over T, for every fp32
    value in [0, 256] that is a T[b], its predecessor or its successor, the edges of the guess table's cells and their neighbours, and a random million"""
    t = ref.T32
    cells = np.arange(0, 4097, dtype=np.float32) / np.float32(16)
    special = np.concatenate([t, np.nextafter(t, np.float32(-1)), np.nextafter(t, np.float32(1e9)),
                              cells, np.nextafter(cells, np.float32(-1)).clip(0), np.nextafter(cells, np.float32(1e9)),
                              ref.D16.astype(np.float32), np.array([0.0, 255.0, 256.0, 300.0, 511.0, 1e-30], np.float32)]).astype(np.float32)
    rng = np.random.default_rng(0x1F1F)
    rand = np.concatenate([rng.uniform(0.0, 256.0, 700_000), rng.uniform(0.0, 8.0, 200_000), 256.0 * rng.uniform(0.0, 1.0, 100_000) ** 4]).astype(np.float32)
    for s in (special, rand):
        got, want = native.linear_encode(s), ref.encode(s)
        assert (got == want).all(), (s[got != want][:8], got[got != want][:8], want[got != want][:8])
    assert set(np.unique(native.linear_encode(special))) == set(range(256))


# ---- the constants ---------------------------------------------------------------------------------------------------------------------------

def test_the_flag_is_bit_256_in_the_header_the_binding_and_the_export(native):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lfi.h")).read()
    assert re.search(r"\bLFI_FLAG_LINEAR_LIGHT = 256u\b", header)
    assert native.abi.LFI_FLAG_LINEAR_LIGHT == 256 and native.LFI_FLAG_LINEAR_LIGHT == 256 and ref.FLAG_LINEAR_LIGHT == 256
    assert "LFI_FLAG_LINEAR_LIGHT" in native.__all__
    host = native.load_host_library()
    assert hasattr(host, "lfi_host_linear_tables") and hasattr(host, "lfi_host_linear_encode")


# ---- the command line ------------------------------------------------------------------------------------------------------------------------

ARGS = ["--synthetic", "3,3,16,8", "-t", "0,0,1,1", "-m", "TEN_WM", "-n", "4", "-b", "1", "-f", "0.2"]


def test_cli_help_names_the_option(native):
    res = run_cli(native, "-h")
    assert res.returncode == 0
    for word in ("--light encoded|linear", "decodes every sample from sRGB"):
        assert word in res.stdout, word


@pytest.mark.parametrize("extra,word", [
    (["-r", "0.3"], "-r above 0"),
    (["-F", "0.4"], "-F"),
    (["-c"], "-c (view-centred"),
    (["-c", "-r", "0.3", "--view-maps"], "cannot be combined"),
    (["--view-maps"], "--view-maps"),
    (["--deep"], "--deep"),
    (["--edges", "in-frame"], "--edges in-frame"),
    (["-g", "2"], "-g above 1"),
])
def test_cli_usage_errors_come_back_without_a_gpu(native, tmp_path, extra, word):
    res = run_cli(native, *ARGS, "-o", str(tmp_path / "out"), "--light", "linear", *extra)
    assert res.returncode != 0 and "--light linear" in res.stderr and word in res.stderr, (res.stdout, res.stderr)
    assert not (tmp_path / "out").exists()


def test_cli_light_takes_encoded_or_linear(native, tmp_path):
    res = run_cli(native, *ARGS, "-o", str(tmp_path / "out"), "--light", "gamma")
    assert res.returncode != 0 and "--light expects encoded or linear." in res.stderr
    assert not (tmp_path / "out").exists()


# ---- the code object -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not code_object.have_tools(), reason="ROCm LLVM tools not installed")
def test_linear_kernels_exist_and_fit(native):
    """blend_linear twice (STD, TEN_WM): no scratch, no spills, at most 256 VGPRs; the TEN_WM one on the matrix cores, the STD one not; both fetch by
    LDS-DMA and look their operands up in LDS"""
    kernels = code_object.kernels(native.build.HIP_LIB)
    bodies = code_object.bodies(native.build.HIP_LIB)
    found = code_object.named(kernels, "blend_linear")
    assert len(found) == 2, sorted(found)
    for k, r in found.items():
        assert r[".private_segment_fixed_size"] == 0 and r[".vgpr_spill_count"] == 0 and r[".sgpr_spill_count"] == 0, (k, r)
        assert r[".vgpr_count"] <= 256, (k, r[".vgpr_count"])
        assert "scratch_" not in bodies[k], k
        assert "global_load_lds_dwordx4" in bodies[k], k
    blends = code_object.named(bodies, "blend_linear")
    ten = [k for k in blends if "ILb0E" in k][0]
    std = [k for k in blends if "ILb1E" in k][0]
    assert "v_mfma_f32_16x16x32_f16" in blends[ten] and "v_mfma" not in blends[std]
    assert "ds_read_u16" in blends[ten]                                        # the fp16 decode table
    assert any(op in blends[std] for op in ("v_pk_fma_f32", "v_fma_f32", "v_fmac_f32"))
    assert "v_cvt_f32_ubyte" not in blends[std]                                # the fp32 decode table stands in for the conversion
    assert len(code_object.named(kernels, "deep_blend")) == 2 and len(code_object.named(kernels, "blend_inframe")) == 2
