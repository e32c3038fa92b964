"""CPU: the table of tests/input_writers.py held to the header and to being a check, before tests/test_gpu_input_writers.py leans on it.

Every function of include/lfi.h that can change a context's inputs — or that decides which copy of them is read — is named by a row of
WRITERS or by EXCLUDED with its reason: the next writer added to the ABI fails here until it has a row.  And for every (writer, reader)
pair, on the oracle alone: the expected output after the writer differs from the one before it, and from the one with any single run of
a partial writer left unapplied — otherwise a stale plane would pass the GPU test.  Where a focus reader samples none of the images a
run changes, its output must NOT change, and the GPU test then holds it to the unchanged oracle."""
import os
import re

import numpy as np
import pytest

import lfinterpolator_amd as L
import input_writers as iw
from conftest import ROOT


def _declared():
    with open(os.path.join(ROOT, "include", "lfi.h")) as f:
        text = f.read()
    return re.findall(r"^(?:int|const char \*)\s*(lfi_\w+)\(", text, flags=re.M)


def test_every_input_writer_of_the_header_has_a_row():
    declared = _declared()
    assert len(declared) > 80 and "lfi_upload_image" in declared and "lfi_last_error" in declared, "the header is no longer parsed"
    family = sorted(f for f in declared if re.fullmatch(iw.WRITER_FAMILY, f))
    assert len(family) >= 18, family
    named = {f for w in iw.WRITERS for f in w.abi}
    missing = [f for f in family if f not in named and f not in iw.EXCLUDED]
    assert not missing, f"declared in include/lfi.h without a row in tests/input_writers.py WRITERS or a reason in EXCLUDED: {missing}"
    assert not sorted((named | set(iw.EXCLUDED)) - set(declared)), "rows name functions the header does not declare"
    assert not sorted(named & set(iw.EXCLUDED)), "both a row and an exclusion"
    assert all(len(reason) > 10 for reason in iw.EXCLUDED.values())
    assert len({w.name for w in iw.WRITERS}) == len(iw.WRITERS) and len({r.name for r in iw.READERS}) == len(iw.READERS)


def test_the_partial_writers_walk_the_run_loop_at_both_ends():
    """one writer changes a single image, one a run in the middle, one two disjoint runs in a single step; image 0 and image N − 1 each
    appear in a partial writer's set (ensure_planar's run loop starts and ends on a changed image)"""
    for shape in iw.SHAPES:
        n = shape.n
        partial = [w for w in iw.WRITERS if w.runs is not None and not w.released]
        runs = {w.name: w.image_runs(n) for w in partial}
        for name, rr in runs.items():
            assert all(0 <= a < b <= n for a, b in rr) and all(rr[i][1] < rr[i + 1][0] for i in range(len(rr) - 1)), (name, rr)
            assert sum(b - a for a, b in rr) < n, (name, "changes every image: not partial")
        assert any(len(rr) == 1 and rr[0][1] - rr[0][0] == 1 for rr in runs.values())
        assert any(len(rr) == 1 and rr[0][0] > 0 and rr[0][1] < n and rr[0][1] - rr[0][0] > 1 for rr in runs.values())
        assert any(len(rr) == 2 and rr[0][0] > 0 and rr[1][1] < n for rr in runs.values())
        assert any(rr[0][0] == 0 for rr in runs.values()) and any(rr[-1][1] == n for rr in runs.values())
        assert any(w.runs is not None for w in iw.WRITERS if w.released)


def test_the_scene_restatement_is_a_shifted_texture(native):
    """scene_lf against what the header promises of lfi_fill_synthetic_scene: sampling every image at pixel + floor(f*·offset) shows the same
    texel, f* candidate 3 of [focus, focus + range] (one 1024 x 1024 block here); alpha is 255; cells are 8 x 8"""
    shape = iw.Shape("scene", 4, 4, 320, 200, 0, (4, 2))
    hp = iw.Shadow(shape, None).params(L)
    lf = iw.scene_lf(hp.offsets, shape.n, shape.W, shape.H, 7, hp.focus, hp.range)
    assert (lf[..., 3] == 255).all() and len(np.unique(lf[0, ..., :3].reshape(-1, 3), axis=0)) > 20
    assert len(np.unique(lf[0, ..., :3].reshape(-1, 3), axis=0)) <= (shape.W // 8 + 2) * (shape.H // 8 + 2)   # 8 x 8 cells
    f = L.focus_candidates(hp.focus, hp.range, 32)
    hits = []
    for k in (3, 11, 20, 28):
        sx = np.floor(np.float32(f[k]) * hp.offsets[:, 0]).astype(int)
        sy = np.floor(np.float32(f[k]) * hp.offsets[:, 1]).astype(int)
        m = max(int(np.abs(sx).max()), int(np.abs(sy).max())) + 1
        ys, xs = np.meshgrid(np.arange(m, shape.H - m), np.arange(m, shape.W - m), indexing="ij")
        assert ys.size > 1000
        if all((lf[g, ys + sy[g], xs + sx[g], :3] == lf[0, ys + sy[0], xs + sx[0], :3]).all() for g in range(1, shape.n)):
            hits.append(k)
    assert len(hits) == 1, ("the images do not show one texture at exactly one of the four candidates", hits)


@pytest.mark.parametrize("shape", iw.SHAPES, ids=lambda s: s.name)
@pytest.mark.parametrize("writer", iw.WRITERS, ids=lambda w: w.name)
def test_no_pair_passes_on_a_stale_copy(writer, shape, oracle_c, native):
    table = iw.stale_copy_check(oracle_c, L, shape, writer)
    assert {name for name, _, _ in table} == {r.name for r in iw.readers_of(writer)}, "a reader was skipped"
    # every reader that samples all images changes under every writer
    assert all(must for name, _, must in table if name in ("std_rgba_layout", "ten_wm_planar_layout", "view_rows_planar_source", "all_focus_std_uploaded_map", "download_derived",
                                                           "deep_std", "inframe_std", "linear_std", "linear_ten"))
    # the flagged readers join every writer, released ones included
    assert {r.name for r in iw.FLAGGED_READERS} == {"deep_std", "inframe_std", "linear_std", "linear_ten"} <= {name for name, _, _ in table}


def test_some_pairs_must_not_change_and_most_must(native):
    """the 3 x 5 shape keeps 8 focus ids: some run of some partial writer lies outside them (the "must not change" pairs exist), and every
    writer still changes every focus reader through some image; the 4 x 4 shape samples every image"""
    a, b = iw.SHAPES
    assert len(iw.Shadow(a, None).params(L).focus_map_ids) == a.n
    ids = {int(g) for g in iw.Shadow(b, None).params(L).focus_map_ids}
    assert len(ids) == b.ids < b.n
    outside = [(w.name, run) for w in iw.WRITERS if not w.released for run in w.image_runs(b.n) if not set(range(*run)) & ids]
    assert outside, "no run outside the focus ids: the unchanged-oracle case is not exercised"
    assert all(set(w.images(b.n)) & ids for w in iw.WRITERS if not w.released), "a writer reaches no focus reader at all"
    assert len(iw.pairs()) == sum(len(iw.readers_of(w)) for w in iw.WRITERS)
