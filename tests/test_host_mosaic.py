"""CPU: mosaic input (include/lfi.h: lfi_mosaic, lfi_mosaic_map, lfi_upload_mosaic_yuv, lfi_upload_mosaic) — the mapping against its numpy
twin (tests/mosaic_ref.py) and every refusal, the staged route's chunk plan, the new kernels' resources, and the command line's usage
errors, which are raised from the file alone before any GPU is touched."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import code_object
import mosaic_ref as mref
from view_rows import run_cli


def _mosaic(native, tiles_x, tiles_y, first_tile, n, order, flags):
    return native.Mosaic(tiles_x, tiles_y, first_tile, n, order, flags)


def _map(lib, m, cols, rows, g0, k):
    tx, ty, g = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    rc = lib.lfi_mosaic_map(C.byref(m) if m is not None else None, cols, rows, g0, k, C.byref(tx), C.byref(ty), C.byref(g))
    return rc, (tx.value, ty.value, g.value)


# ---- the interface ------------------------------------------------------------------------------------------------------------------------------

def test_header_constants_equal_the_bindings(native):
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "lfi.h")).read()
    m = re.search(r"enum \{ LFI_MOSAIC_ROWS = (\d+), LFI_MOSAIC_GRID = (\d+) \};", text)
    assert m and (int(m.group(1)), int(m.group(2))) == (native.LFI_MOSAIC_ROWS, native.LFI_MOSAIC_GRID) == (mref.ROWS, mref.GRID)
    m = re.search(r"enum \{ LFI_MOSAIC_BOTTOM_UP = (\d+)u \};", text)
    assert m and int(m.group(1)) == native.LFI_MOSAIC_BOTTOM_UP == mref.BOTTOM_UP
    assert re.search(r"int lfi_mosaic_map\(const lfi_mosaic \*m, int cols, int rows, int g0, int k, int \*tx, int \*ty, int \*g\);", text)
    assert re.search(r"int lfi_upload_mosaic_yuv\(lfi_ctx \*ctx, const lfi_mosaic \*m, int g0, int matrix, int range, int chroma, const lfi_yuv_surfaces \*src\);", text)
    assert re.search(r"int lfi_upload_mosaic\(lfi_ctx \*ctx, const lfi_mosaic \*m, int g0, const uint8_t \*rgba, size_t pitch_bytes\);", text)
    fields = re.search(r"typedef struct lfi_mosaic \{(.*?)\} lfi_mosaic;", text, re.S).group(1)
    declared = [name for line in re.sub(r"/\*.*?\*/", "", fields, flags=re.S).split(";") for name in re.findall(r"(\w+)\s*(?:,|$)", line.strip())]
    assert declared == [f for f, _ in native.Mosaic._fields_] == ["tiles_x", "tiles_y", "first_tile", "n", "order", "flags"]
    assert C.sizeof(native.Mosaic) == 24
    lib = native.load_hip_library()
    for name in ("lfi_mosaic_map", "lfi_upload_mosaic_yuv", "lfi_upload_mosaic"):
        assert name in native.ABI_SYMBOLS and hasattr(lib, name)
    for name in ("upload_mosaic_yuv", "upload_mosaic"):
        assert hasattr(native.Context, name) and hasattr(native, name)
    # without a context the uploads refuse
    m = native.Mosaic.make(1, 1)
    assert lib.lfi_upload_mosaic_yuv(None, C.byref(m), 0, 0, 0, 0, None) == -1
    assert lib.lfi_upload_mosaic(None, C.byref(m), 0, None, 0) == -1


# ---- the mapping --------------------------------------------------------------------------------------------------------------------------------

def _grids(tiles_x, tiles_y, order):
    """the grids a mosaic of this shape is tried against: its own, its transpose, one row of all tiles, and one image more than that"""
    t = tiles_x * tiles_y
    return [(tiles_x, tiles_y), (tiles_y, tiles_x), (t, 1), (t + 1, 1)]


def test_map_equals_the_twin_over_all_small_mosaics(native):
    """(order, flags, tiles 1…4 x 1…3, first_tile, n, g0) against every grid of _grids: the same refusals, and for every k the same tile"""
    lib = native.load_hip_library()
    accepted = refused = 0
    for order, flags, tiles_x, tiles_y in itertools.product((mref.ROWS, mref.GRID), (0, mref.BOTTOM_UP), range(1, 5), range(1, 4)):
        t = tiles_x * tiles_y
        for first_tile, g0 in itertools.product(range(0, t), (0, 1)):
            for n in sorted({1, 2, t - first_tile, t - first_tile + 1}):
                for cols, rows in _grids(tiles_x, tiles_y, order):
                    want = mref.mosaic_map(tiles_x, tiles_y, first_tile, n, order, flags, cols, rows, g0)
                    m = _mosaic(native, tiles_x, tiles_y, first_tile, n, order, flags)
                    what = (order, flags, tiles_x, tiles_y, first_tile, n, g0, cols, rows)
                    if want is None:
                        assert _map(lib, m, cols, rows, g0, 0) == (-1, (-7, -7, -7)), what
                        refused += 1
                        continue
                    accepted += 1
                    for k in range(n):
                        assert _map(lib, m, cols, rows, g0, k) == (0, tuple(int(v) for v in want[k])), (what, k)
                    assert _map(lib, m, cols, rows, g0, n)[0] == -1 and _map(lib, m, cols, rows, g0, -1)[0] == -1, what
                    # no two tiles share a place or an image
                    assert len({(a, b) for a, b, _ in want}) == n == len({g for _, _, g in want}), what
                    assert (native.abi.mosaic_map(m, cols, rows, g0) == want).all(), what
    assert accepted > 300 and refused > 300, (accepted, refused)


def test_map_by_hand(native):
    """a 3 x 2 camera mosaic: tile (tx, ty) is the camera of file <ty>_<tx>, g = tx * rows + ty; bottom-up the cameras' rows run upwards.  A
    quilt of 6 views in a 3 x 2 frame: reading order, bottom-up from the bottom left"""
    assert native.mosaic_map(3, 2, 3, 2, "grid").tolist() == [[0, 0, 0], [1, 0, 2], [2, 0, 4], [0, 1, 1], [1, 1, 3], [2, 1, 5]]
    assert native.mosaic_map(3, 2, 3, 2, "grid", bottom_up=True).tolist() == [[0, 1, 0], [1, 1, 2], [2, 1, 4], [0, 0, 1], [1, 0, 3], [2, 0, 5]]
    assert native.mosaic_map(3, 2, 6, 1, "rows").tolist() == [[0, 0, 0], [1, 0, 1], [2, 0, 2], [0, 1, 3], [1, 1, 4], [2, 1, 5]]
    assert native.mosaic_map(3, 2, 6, 1, "rows", bottom_up=True).tolist() == [[0, 1, 0], [1, 1, 1], [2, 1, 2], [0, 0, 3], [1, 0, 4], [2, 0, 5]]
    assert native.mosaic_map(5, 1, 4, 1, "rows", first_tile=2, n=2, g0=1).tolist() == [[2, 0, 1], [3, 0, 2]]


def test_map_refusals(native):
    lib = native.load_hip_library()
    good = dict(tiles_x=3, tiles_y=2, first_tile=0, n=6, order=mref.GRID, flags=0)
    assert _map(lib, _mosaic(native, **good), 3, 2, 0, 0)[0] == 0
    cases = [
        ("GRID with a partial range", dict(good, n=5), (3, 2, 0)),
        ("GRID from tile 1", dict(good, first_tile=1, n=5), (3, 2, 0)),
        ("GRID with g0", dict(good), (3, 2, 1)),
        ("GRID on a transposed grid", dict(good), (2, 3, 0)),
        ("GRID on a row of images", dict(good), (6, 1, 0)),
        ("tiles past the last tile", dict(good, order=mref.ROWS, first_tile=4, n=3), (6, 1, 0)),
        ("images past the last image", dict(good, order=mref.ROWS, n=6), (3, 2, 1)),
        ("n = 0", dict(good, order=mref.ROWS, n=0), (3, 2, 0)),
        ("first_tile below 0", dict(good, order=mref.ROWS, first_tile=-1, n=2), (3, 2, 0)),
        ("g0 below 0", dict(good, order=mref.ROWS, n=2), (3, 2, -1)),
        ("tiles_x = 0", dict(good, tiles_x=0), (3, 2, 0)),
        ("tiles_y below 0", dict(good, tiles_y=-2), (3, 2, 0)),
        ("cols = 0", dict(good, order=mref.ROWS, n=1), (0, 2, 0)),
        ("rows = 0", dict(good, order=mref.ROWS, n=1), (3, 0, 0)),
        ("unknown order", dict(good, order=2), (3, 2, 0)),
        ("order below 0", dict(good, order=-1), (3, 2, 0)),
        ("unknown flag", dict(good, flags=2), (3, 2, 0)),
        ("unknown flag beside the known one", dict(good, flags=mref.BOTTOM_UP | 0x80000000), (3, 2, 0)),
    ]
    for what, fields, (cols, rows, g0) in cases:
        assert _map(lib, _mosaic(native, **fields), cols, rows, g0, 0) == (-1, (-7, -7, -7)), what
        with pytest.raises(native.LfiError):
            native.abi.mosaic_map(_mosaic(native, **fields), cols, rows, g0)
    assert _map(lib, None, 3, 2, 0, 0) == (-1, (-7, -7, -7))
    # tile counts that overflow 32 bits are counted in 64
    big = _mosaic(native, 1 << 20, 1 << 20, 0, 1, mref.ROWS, 0)
    assert _map(lib, big, 1, 1, 0, 0) == (0, (0, 0, 0))
    # the outputs may be NULL: the call then only judges the mosaic
    assert lib.lfi_mosaic_map(C.byref(_mosaic(native, **good)), 3, 2, 0, 5, None, None, None) == 0


# ---- the staged route's plan ----------------------------------------------------------------------------------------------------------------------

def _chunks(lib, m, w, h, cap):
    out = []
    for c in range(64):
        five = np.full(5, -7, np.int32)
        if lib.lfi_debug_mosaic_chunk(C.byref(m), w, h, cap, c, five.ctypes.data) != 0:
            assert (five == -7).all()
            break
        out.append(tuple(int(v) for v in five))
    return out


def test_chunks_are_whole_tile_rows_under_the_cap(native):
    """tiles of 16 x 4 in a frame 3 tiles wide: a staged tile row is 48 x 4 x 3/2 = 288 bytes.  Every tile of the call lies in exactly one
    chunk, a chunk's rows fit the cap (or it is one row), and bottom-up the copied rows are counted from the frame's other end"""
    lib = native.load_hip_library()
    w, h, row = 16, 4, 288
    for bottom_up, (first_tile, n), cap in itertools.product((False, True), [(0, 12), (2, 5), (4, 8), (5, 1)], (1, row, 2 * row - 1, 2 * row, 3 * row, 100 * row)):
        m = native.Mosaic.make(3, 4, "rows", bottom_up, first_tile, n)
        chunks = _chunks(lib, m, w, h, cap)
        per = max(1, cap // row)
        r_first, r_last = first_tile // 3, (first_tile + n - 1) // 3
        assert len(chunks) == -(-(r_last - r_first + 1) // per), (bottom_up, first_tile, n, cap, chunks)
        k_next, r_next = 0, r_first
        for r0, nr, ty0, k0, nk in chunks:
            assert (r0, k0) == (r_next, k_next) and 1 <= nr <= per and nk >= 1
            assert ty0 == (4 - (r0 + nr) if bottom_up else r0)
            rows = [(first_tile + k) // 3 for k in range(k0, k0 + nk)]
            assert min(rows) == r0 and max(rows) == r0 + nr - 1
            k_next, r_next = k0 + nk, r0 + nr
        assert k_next == n and r_next == r_last + 1
    # the call's own cap: 8 x 8 cameras of 1920 x 1080 — a tile row of 15360 x 1080 x 3/2 bytes, ten to a chunk of 256 MiB: one chunk
    assert _chunks(lib, native.Mosaic.make(8, 8, "grid"), 1920, 1080, 0) == [(0, 8, 0, 0, 64)]
    # … and 16 x 16 tiles of 3840 x 2160 in a frame of 61440 x 34560: a tile row is 199,065,600 bytes, one to a chunk
    assert [c[:2] for c in _chunks(lib, native.Mosaic.make(16, 16, "grid"), 3840, 2160, 0)] == [(r, 1) for r in range(16)]
    # refusals: an odd size, a bad mosaic, NULL
    five = np.zeros(5, np.int32)
    assert lib.lfi_debug_mosaic_chunk(C.byref(native.Mosaic.make(3, 4)), 15, 4, 0, 0, five.ctypes.data) == -1
    assert lib.lfi_debug_mosaic_chunk(C.byref(native.Mosaic.make(3, 4)), 16, 3, 0, 0, five.ctypes.data) == -1
    assert lib.lfi_debug_mosaic_chunk(C.byref(native.Mosaic.make(3, 4, n=13)), 16, 4, 0, 0, five.ctypes.data) == -1
    assert lib.lfi_debug_mosaic_chunk(None, 16, 4, 0, 0, five.ctypes.data) == -1
    assert lib.lfi_debug_mosaic_chunk(C.byref(native.Mosaic.make(3, 4)), 16, 4, 0, 0, None) == -1


# ---- the code object ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not code_object.have_tools(), reason="ROCm LLVM tools not installed")
def test_mosaic_kernels_exist_and_fit(native):
    """yuvs_mosaic_expand<FORMAT, NEAREST, UNALIGNED> eight times and yuvs_mosaic_expand_left<FORMAT, UNALIGNED> four times (a left-sited nearest
    upload is the nearest kernel), under stems of their own: the numbers of yuvs_expand and yuvs_expand_left bodies stay what they were.  No
    scratch, no spills, no LDS, no atomics, at most 128 registers.  The aligned kernels load what yuvs_expand loads; the unaligned ones load
    dwords only — no wider load could be aligned — and shift them with v_alignbyte_b32"""
    kernels = code_object.kernels(native.build.HIP_LIB)
    bodies = code_object.bodies(native.build.HIP_LIB)
    expect = {"yuvs_mosaic_expand": [f"ILi{f}ELb{n}ELb{u}E" for f in "01" for n in "01" for u in "01"],
              "yuvs_mosaic_expand_left": [f"ILi{f}ELb{u}E" for f in "01" for u in "01"]}
    for stem, variants in expect.items():
        found = code_object.named(kernels, stem)
        assert len(found) == len(variants), (stem, sorted(found))
        for v in variants:
            assert sum(f"{stem}{v}" in k for k in found) == 1, (stem, v, sorted(found))
        for k, r in found.items():
            assert r[".private_segment_fixed_size"] == 0 and r[".vgpr_spill_count"] == 0 and r[".sgpr_spill_count"] == 0, (k, r)
            assert r[".group_segment_fixed_size"] == 0 and r[".vgpr_count"] <= 128, (k, r)
            text = bodies[k]
            assert "scratch_" not in text and "atomic" not in text and "ds_read" not in text and "ds_write" not in text, k
            unaligned = k[:k.index("EEEv")].endswith("Lb1")
            wide = len(re.findall(r"global_load_dwordx[234]", text))
            if unaligned:
                assert wide == 0 and "v_alignbyte_b32" in text, (k, wide)
                assert not re.search(r"global_load_(u|s)(byte|short)", text), k
            else:
                assert wide > 0 and "v_alignbyte_b32" not in text, (k, wide)
    assert len(code_object.named(kernels, "yuvs_expand")) == 4 and len(code_object.named(kernels, "yuvs_expand_left")) == 2
    # the aligned kernels run yuvs_block_pixels as it is: the loads of their twins, instruction by instruction
    loads = lambda text: sorted(re.findall(r"global_load_\w+", text))
    twins = {k[len("_ZN3lfi11yuvs_expand"):k.index("EEEv")]: v for k, v in code_object.named(bodies, "yuvs_expand").items()}
    for k in code_object.named(kernels, "yuvs_mosaic_expand"):
        variant = k[len("_ZN3lfi18yuvs_mosaic_expand"):k.index("EEEv")]
        if variant.endswith("Lb0"):
            assert loads(bodies[k]) == loads(twins[variant[:-len("ELb0")]]), k
    left = {k[len("_ZN3lfi16yuvs_expand_left"):k.index("EEEv")]: v for k, v in code_object.named(bodies, "yuvs_expand_left").items()}
    for k in code_object.named(kernels, "yuvs_mosaic_expand_left"):
        variant = k[len("_ZN3lfi23yuvs_mosaic_expand_left"):k.index("EEEv")]
        if variant.endswith("Lb0"):
            assert loads(bodies[k]) == loads(left[variant[:-len("ELb0")]]), k


# ---- the command line -------------------------------------------------------------------------------------------------------------------------------

RENDER = ["-t", "0,0.5,1,0.5", "-m", "STD", "-f", "0.1", "-n", "4", "-b", "1"]


def _y4m(native, path, w, h, depth=8):
    bytes_ = (w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)) * (2 if depth == 10 else 1)
    native.write_y4m(str(path), np.full((2, bytes_), 64 if depth == 8 else 1, np.uint8), w, h, depth=depth)


def test_cli_help_and_usage_errors(native, tmp_path):
    """every refusal names what is wrong and comes from the file alone: no output directory, and no GPU needed"""
    res = run_cli(native, "-h")
    assert res.returncode == 0
    for flag in ("--mosaic CxR", "--mosaic-order grid|rows", "--mosaic-bottom-up"):
        assert flag in res.stdout
    out = tmp_path / "out"
    from PIL import Image
    Image.fromarray(np.zeros((8, 14, 3), np.uint8)).save(tmp_path / "quilt.png")
    _y4m(native, tmp_path / "even.y4m", 24, 8)
    _y4m(native, tmp_path / "deep.y4m", 24, 8, depth=10)
    for args, words in [
        (["-i", str(tmp_path / "quilt.png"), "--mosaic", "3x2"], ("14x8", "3x2", "remainder")),
        (["-i", str(tmp_path / "quilt.png"), "--mosaic", "2x3"], ("14x8", "2x3", "remainder")),
        (["-i", str(tmp_path / "even.y4m"), "--mosaic", "5x2"], ("24x8", "5x2", "remainder")),
        (["-i", str(tmp_path / "even.y4m"), "--mosaic", "4x2"], ("6x4",)),                                 # divides, even: only the missing GPU may stop it
        (["-i", str(tmp_path / "even.y4m"), "--mosaic", "8x2"], ("3x4", "even", "4:2:0")),
        (["-i", str(tmp_path / "even.y4m"), "--mosaic", "2x8"], ("12x1", "even", "4:2:0")),
        (["-i", str(tmp_path / "deep.y4m"), "--mosaic", "2x2"], ("10-bit", "C420p10", "not supported")),
        (["-i", str(tmp_path / "even.y4m"), "--mosaic", "2x2", "--lean-inputs"], ("--lean-inputs", "--mosaic", "planar copy")),
        (["-i", str(tmp_path / "even.y4m"), "--mosaic", "2"], ("--mosaic", "CxR")),
        (["-i", str(tmp_path / "even.y4m"), "--mosaic", "0x2"], ("--mosaic", "CxR")),
        (["-i", str(tmp_path / "even.y4m"), "--mosaic", "2x2", "--mosaic-order", "columns"], ("--mosaic-order", "grid", "rows")),
        (["-i", str(tmp_path / "even.y4m"), "--mosaic-order", "rows"], ("--mosaic-order", "--mosaic CxR")),
        (["-i", str(tmp_path / "even.y4m"), "--mosaic-bottom-up"], ("--mosaic-bottom-up", "--mosaic CxR")),
        (["--synthetic", "2,2,12,4", "--mosaic", "2x2"], ("--mosaic", "--synthetic")),
        (["-i", str(tmp_path / "missing.png"), "--mosaic", "2x2"], ("missing.png",)),
    ]:
        res = run_cli(native, *args, *RENDER, "-o", str(tmp_path / "good" if words == ("6x4",) else out))
        if words == ("6x4",):
            # a good mosaic: with a GPU it renders, without one the context is what fails — never the mosaic
            assert "remainder" not in res.stderr and "even" not in res.stderr, res.stderr
            assert res.returncode == 0 or "GPU" in res.stderr, res.stderr
            continue
        assert res.returncode != 0, args
        for word in words:
            assert word in res.stderr, (args, res.stderr)
        assert not out.exists(), args
