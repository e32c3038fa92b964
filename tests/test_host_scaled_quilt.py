"""CPU: the host side of scaled quilts (lfi_download_quilt_scaled) — the span arithmetic the kernel runs, through lfi_host_area_span, against
overlaps computed by brute force; the numpy restatement (tests/scaled_quilt_ref.py) against the definition as written, the block mean, the
identity and the float64 area mean; the exported symbols; the CLI's checks of --quilt-tile; the new kernel's code object."""

import numpy as np
import pytest

import code_object
import scaled_quilt_ref as ref
from view_rows import run_cli

# (src, dst): dst = 1, dst = src, integer ratios, coprime pairs, the tile sizes of 4096² and 8192² quilts from 1080p and 4K views
PAIRS = [(1, 1), (7, 1), (7, 7), (2, 1), (12, 4), (13, 5), (50, 17), (22, 9), (50, 25), (22, 11), (97, 96), (100, 51), (1920, 819), (1080, 455),
         (3840, 1638), (2160, 910), (3840, 1920), (1920, 1919), (1920, 1)]


def _brute_overlap(src, dst, o):
    """[src] int64: the overlap of output o with every source pixel, on the grid of src·dst units"""
    s = np.arange(src, dtype=np.int64)
    return np.maximum(np.minimum((o + 1) * src, (s + 1) * dst) - np.maximum(o * src, s * dst), 0)


@pytest.mark.parametrize("src,dst", PAIRS)
def test_spans_agree_with_brute_force_overlaps(native, src, dst):
    covered = np.zeros(src, np.int64)   # per source pixel: the sum of its weights over all outputs
    prev_last = -1
    for o in range(dst):
        first, last, w_first, w_last = native.area_span(src, dst, o)
        ov = _brute_overlap(src, dst, o)
        nz = np.flatnonzero(ov)
        assert (first, last) == (nz[0], nz[-1]) and (np.diff(nz) == 1).all(), (o, first, last)
        assert w_first == ov[first] and w_last == ov[last], (o, w_first, w_last)
        assert (ov[first + 1:last] == dst).all(), o                       # every interior weight
        total = w_first if first == last else w_first + w_last + (last - first - 1) * dst
        assert total == src == ov.sum(), (o, total)
        assert first in (prev_last, prev_last + 1), (o, first, prev_last)  # no gap between neighbouring outputs' spans
        prev_last = last
        covered[first:last + 1] += ov[first:last + 1]
    assert native.area_span(src, dst, 0)[0] == 0 and prev_last == src - 1
    assert (covered == dst).all()                                          # the spans tile the source: every source pixel is used up exactly


def test_spans_at_the_largest_axis(native):
    """src = 65535: every product stays below 2^32 (csrc/area_span.h works in uint32_t)"""
    src = 65535
    for dst in (1, 2, 3, 32768, 65534, 65535):
        for o in sorted({0, 1 % dst, dst // 2, dst - 1}):
            first, last, w_first, w_last = native.area_span(src, dst, o)
            ov = _brute_overlap(src, dst, o)
            nz = np.flatnonzero(ov)
            assert (first, last, w_first, w_last) == (nz[0], nz[-1], ov[nz[0]], ov[nz[-1]]), (dst, o)


@pytest.mark.parametrize("args", [(8, 0, 0), (8, 9, 0), (8, 4, 4), (8, 4, -1), (0, 0, 0), (65536, 2, 0)])
def test_span_export_refuses_what_is_not_a_downscale(native, args):
    with pytest.raises(ValueError):
        native.area_span(*args)


# ---- the numpy restatement ------------------------------------------------------------------------------------------------------------

def _random_view(rng, W, H):
    view = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    view[..., 3] = 255
    return view


@pytest.mark.parametrize("W,H,tw,th", [(50, 22, 17, 9), (50, 22, 25, 11), (50, 22, 50, 11), (50, 22, 50, 22), (50, 22, 1, 1), (41, 12, 40, 5),
                                       (64, 48, 3, 47), (7, 5, 1, 5)])
def test_restatement_equals_the_definition_as_written(W, H, tw, th):
    view = _random_view(np.random.default_rng(W * 1000 + tw), W, H)
    assert (ref.resize(view, tw, th) == ref.resize_dense(view, tw, th)).all()


@pytest.mark.parametrize("W,H,k,l", [(48, 20, 2, 2), (48, 20, 3, 5), (48, 20, 48, 20), (48, 20, 1, 4), (60, 36, 5, 1), (1920, 1080, 2, 2)])
def test_integer_ratios_give_the_block_mean_rounded_half_up(W, H, k, l):
    view = _random_view(np.random.default_rng(k * 100 + l), W, H)
    got = ref.resize(view, W // k, H // l)
    blocks = view.astype(np.uint64).reshape(H // l, l, W // k, k, 4).sum(axis=(1, 3))
    want = (blocks + (k * l) // 2) // (k * l)
    assert (got[..., :3] == want[..., :3]).all() and (got[..., 3] == 255).all()


def test_half_up_rounding_is_exercised():
    """a 2 x 1 block of 0 and 1 has the mean 0.5: rounded UP"""
    view = np.zeros((1, 2, 4), np.uint8)
    view[0, 1, :3] = 1
    assert ref.resize(view, 1, 1)[0, 0].tolist() == [1, 1, 1, 255]


@pytest.mark.parametrize("W,H", [(50, 22), (1, 1), (131, 33)])
def test_identity_at_the_views_size(W, H):
    view = _random_view(np.random.default_rng(W), W, H)
    assert (ref.resize(view, W, H) == view).all()


@pytest.mark.parametrize("W,H,tw,th", [(50, 22, 17, 9), (96, 64, 41, 27), (131, 33, 130, 32), (64, 48, 1, 1), (100, 100, 51, 3)])
def test_within_half_of_the_float64_area_mean(W, H, tw, th):
    """every product and partial sum below is an integer under 2^53: the float64 sums are exact, and so is a quotient that ends in .5"""
    view = _random_view(np.random.default_rng(W + tw), W, H)
    wy, wx = ref.overlaps(H, th).astype(np.float64), ref.overlaps(W, tw).astype(np.float64)
    got = ref.resize(view, tw, th)
    for ch in range(3):
        mean = wy @ view[..., ch].astype(np.float64) @ wx.T / float(W * H)
        assert np.abs(got[..., ch].astype(np.float64) - mean).max() <= 0.5


# ---- the library and the command line -------------------------------------------------------------------------------------------------

def test_symbols_are_exported_and_bound(native):
    lib = native.load_hip_library()
    for name in ("lfi_download_quilt_scaled", "lfi_download_quilt_tiles_scaled"):
        assert name in native.ABI_SYMBOLS and hasattr(lib, name)
    assert hasattr(native.load_host_library(), "lfi_host_area_span")
    assert hasattr(native.Context, "download_quilt_scaled") and hasattr(native.Context, "download_quilt_tiles_scaled")


QUILT_ARGS = ["--synthetic", "4,4,32,16", "-t", "0,0,1,1", "-m", "STD", "-n", "6", "-b", "1", "-f", "0.0"]


def test_cli_refuses_a_tile_size_without_a_quilt(native, tmp_path):
    res = run_cli(native, *QUILT_ARGS, "-o", str(tmp_path / "out"), "--quilt-tile", "16x8")
    assert res.returncode != 0
    assert "--quilt-tile" in res.stderr and "-q" in res.stderr
    assert not (tmp_path / "out").exists()


def test_cli_help_names_the_flag(native):
    res = run_cli(native, "-h")
    assert res.returncode == 0 and "--quilt-tile WxH" in res.stdout


# ---- the code object ------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not code_object.have_tools(), reason="ROCm LLVM tools not installed")
def test_quilt_scale_uses_no_scratch_and_no_atomics(native):
    """From the code object: both instantiations of quilt_scale (csrc/hip/quilt_scaled.hpp) exist, use no scratch, spill nothing, stay at or
    below 96 registers per lane (five waves per SIMD at least), and contain no atomic instruction."""
    kernels = code_object.kernels(native.build.HIP_LIB)
    scale = code_object.named(kernels, "quilt_scale")
    assert len(scale) == 2, sorted(scale)
    for k, v in scale.items():
        assert v[".private_segment_fixed_size"] == 0 and v[".vgpr_spill_count"] == 0 and v[".sgpr_spill_count"] == 0, (k, v)
        assert v[".vgpr_count"] <= 96, (k, v)
    bodies = {k: v for k, v in code_object.bodies(native.build.HIP_LIB).items() if k in scale}
    assert set(bodies) == set(scale)
    for k, text in bodies.items():
        assert "atomic" not in text and "scratch_" not in text, k
        assert "global_load_dword" in text and "ds_write_b128" in text, k
