"""GPU (-m gpu): the HIP library against the reference's own kernels — directly, not through the oracle.

tests/golden/ref_kernels.npz holds what the reference's src/kernels.cu computes when compiled for the CPU (tests/ref_kernel_cases.py,
tests/test_ref_kernels.py); neither the reference tree nor oracle/_ref is read here.  Per case one small context gets the very parameter
arrays and inputs the reference's kernels were given, and every render goes through tests/poison.py:

  * STD, fixed focus and all-focus from the file's map: every view's SHA-256 and the stored views 0 and 63, in both view layouts, by the
    default route and by the `vfma` variant;
  * focus map, every FOCUS variant: map 0 is the reference's estimate, map 1 its filter (the reference filters at radii ≥ 10 only);
  * TEN_WM with LFI_FLAG_TEN_ROUND_PER_BATCH: the hashes (the reference's mma_sync is modelled as M16, oracle/ref_shim/mma.h);
  * TEN_WM by the default route: at most 1 LSB from the reference's bytes — the file holds two views whole, so the oracle's M16 views
    serve as the full copy once THEY hash equal — and the same bytes in both layouts.
"""
import numpy as np
import pytest

import poison
import ref_kernel_cases as rc

pytestmark = pytest.mark.gpu

FIX = rc.Fixture()
TEN_TOL_LSB = 1   # fp32 accumulation on the matrix pipe against the fp16 accumulator of M16 (tests/test_gpu_parity.py)
LAYOUTS = ("rgba", "planar")


def _upload_maps(ctx, case):
    if case["map_seeds"]:
        for k in (0, 1):
            ctx.upload_map(k, FIX.map_in(case, k))


@pytest.mark.parametrize("name", [c["name"] for c in FIX.cases])
def test_hip_library_reproduces_the_reference_kernels(name, gpu, oracle_c):
    case = FIX.case(name)
    (cols, rows), (W, H) = case["grid"], case["size"]
    kernels = case["kernels"]
    hp = FIX.params(case)
    lf = rc.inputs(oracle_c, case)
    ctx = gpu.Context(0)
    ctx.set_grid(cols, rows, W, H)
    ctx.upload_grid(lf)
    ctx.set_params(hp)
    checked = []

    if "estimate" in kernels:
        want0 = FIX.map_out(case, "estimate")
        filtered = "filter" in kernels and min(case["radius"]) >= 10
        for variant in ctx.list_variants("FOCUS"):
            ctx.set_variant("FOCUS", variant)
            poison.focus_map(ctx)
            got0 = ctx.download_map(0)
            assert (got0 == want0).all(), (name, variant, "map 0 differs from the reference's estimate in %d bytes" % int((got0 != want0).sum()))
            checked.append("estimate")
            if filtered:
                got1, want1 = ctx.download_map(1), FIX.map_out(case, "filter")
                assert (got1 == want1).all(), (name, variant, "map 1 differs from the reference's filter in %d bytes" % int((got1 != want1).sum()))
                checked.append("filter")
        ctx.set_variant("FOCUS", "auto")

    for kernel in [k for k in kernels if k.startswith("std")]:
        af = kernel.endswith("_af")
        for layout in LAYOUTS:
            ctx.set_output_layout(layout)
            _upload_maps(ctx, case)
            for variant in ("auto", "vfma"):
                ctx.set_variant("STD", variant)
                poison.render(ctx, "STD", all_focus=af)
                FIX.check_views(case, kernel, ctx.download_views(), (layout, variant, ctx.last_kernel_name()))
        ctx.set_variant("STD", "auto")
        checked.append(kernel)

    for kernel in [k for k in kernels if k.startswith("ten")]:
        af = kernel.endswith("_af")
        # per-batch rounding: the M16 model on the device, byte for byte
        ctx.set_params(hp, gpu.LFI_FLAG_TEN_ROUND_PER_BATCH)
        for layout in LAYOUTS:
            ctx.set_output_layout(layout)
            _upload_maps(ctx, case)
            poison.render(ctx, "TEN_WM", all_focus=af)
            FIX.check_views(case, kernel, ctx.download_views(), (layout, "round per batch", ctx.last_kernel_name()))
        # the default route: within 1 LSB of the reference's bytes, for which the oracle's views stand once their hashes are the file's
        m16 = oracle_c.blend_ten(lf, hp.focused_offsets, hp.offsets, hp.weights, model=oracle_c.TEN_M16, all_focus=af,
                                 map_plane=FIX.map_in(case, 0) if af else None, focus=hp.focus, rng=hp.range)
        FIX.check_views(case, kernel, m16, "the oracle's M16 views")
        ctx.set_params(hp)
        got = {}
        for layout in LAYOUTS:
            ctx.set_output_layout(layout)
            _upload_maps(ctx, case)
            poison.render(ctx, "TEN_WM", all_focus=af)
            got[layout] = ctx.download_views()
            worst = int(np.abs(got[layout].astype(int) - m16.astype(int)).max())
            print("%s %s %s (%s): max |HIP - reference| = %d LSB, %.4f %% of the bytes differ" %
                  (name, kernel, layout, ctx.last_kernel_name(), worst, 100.0 * (got[layout] != m16).mean()))
            assert worst <= TEN_TOL_LSB, (name, kernel, layout, worst)
            assert (got[layout][..., 3] == 255).all()
        assert (got["rgba"] == got["planar"]).all(), (name, kernel, "the two view layouts give different bytes")
        checked.append(kernel)

    assert set(checked) == set(kernels), (name, "kernels of the file that no check above covers", set(kernels) - set(checked))
    ctx.close()
