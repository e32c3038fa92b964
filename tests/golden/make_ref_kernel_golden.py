"""Writes tests/golden/ref_kernels.npz: what the reference's OWN kernels compute for tests/ref_kernel_cases.CASES.

Needs the reference tree (oracle/ref_kernels.py builds oracle/_ref/libref_kernels.so and its non-contracting twin from it); the
tests that read the file need neither.  Run from the repository root:  python tests/golden/make_ref_kernel_golden.py

The parameter arrays (weights, offsets, focus-map image ids) come from the oracle's host functions and are stored as data.  Every
kernel is run in both builds; the file records where they differ ("sensitive"), and is not written when
  * the contracting and the non-contracting build agree on every estimate case or on every all-focus STD case (the inputs would not
    tell nvcc's fused multiply-adds from separate operations),
  * a map has fewer than 8 levels (it would hardly test which map a kernel reads, or the filter),
  * the file exceeds SIZE_CAP.
"""
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ref_kernel_cases as rc  # noqa: E402
from oracle import lfi_oracle_c as oc  # noqa: E402
from oracle import ref_kernels as rk  # noqa: E402

SIZE_CAP = 300 * 1000
MIN_LEVELS = 8


def host_arrays(case):
    (cols, rows), (W, H) = case["grid"], case["size"]
    se = oc.interpret_trajectory(case["traj"], cols, rows)
    off, foc = oc.offsets(se, cols, rows, W, H, case["aspect"], case["focus"])
    return dict(weights=oc.weight_matrix_f16(se, cols, rows, rc.VIEWS, case["effect"]), offsets=off, focused=foc,
                ids=oc.focus_map_ids(se, cols, rows))


def run(case, kernel, lf, hp, maps, fused):
    cols, rows = case["grid"]
    focus, rng = float(np.float32(case["focus"])), float(np.float32(case["range"]))
    if kernel == "estimate":
        return rk.focus_estimate(lf, cols, rows, hp["offsets"], hp["ids"], focus, rng, case["radius"], fused=fused)
    if kernel == "filter":
        return rk.focus_filter(maps["estimate"], case["radius"], fused=fused)
    fn = rk.blend_std if kernel.startswith("std") else rk.blend_ten
    af = kernel.endswith("_af")
    return fn(lf, cols, rows, hp["focused"], hp["offsets"], hp["weights"], af, maps.get(0), maps.get(1), focus, rng, fused=fused)


def main():
    if not rk.available(build=True):
        sys.exit("the reference tree is needed: oracle/_ref/libref_kernels.so could not be built")
    arrays, index, checked_maps = {}, [], []
    for case in rc.CASES:
        name = case["name"]
        lf = rc.inputs(oc, case)
        hp = host_arrays(case)
        for k, a in hp.items():
            arrays[name + "." + k] = a
        maps = {}
        if case["map_seeds"]:
            for k in (0, 1):
                plane = rc.noise_map(oc, case, k)
                arrays["%s.map%d" % (name, k)] = plane
                maps[k] = rc.grey(plane)
                checked_maps.append((name, "map%d" % k, plane))
            assert (maps[0][..., 0] != maps[1][..., 0]).mean() > 0.9
        sensitive = []
        for kernel in case["kernels"]:
            out = run(case, kernel, lf, hp, maps, True)
            other = run(case, kernel, lf, hp, maps, False)
            if (out != other).any():
                sensitive.append(kernel)
            print("%-22s %-9s contraction changes %.4f %% of the bytes" % (name, kernel, 100.0 * (out != other).mean()))
            if kernel in ("estimate", "filter"):
                assert (out[..., 3] == 255).all() and (out[..., 0] == out[..., 1]).all() and (out[..., 0] == out[..., 2]).all()
                maps[kernel] = out
                arrays["%s.%s.map" % (name, kernel)] = out[..., 0].copy()
                checked_maps.append((name, kernel, out[..., 0]))
            else:
                assert (out[..., 3] == 255).all()
                arrays["%s.%s.hashes" % (name, kernel)] = rc.view_hashes(out)
                for v in (0, rc.VIEWS - 1):
                    arrays["%s.%s.view%d" % (name, kernel, v)] = out[v, ..., :3].copy()
        index.append(dict(case, sensitive=sensitive))

    for name, which, plane in checked_maps:
        levels = len(np.unique(plane))
        if levels < MIN_LEVELS:
            sys.exit("refused: %s %s has %d levels, fewer than %d" % (name, which, levels, MIN_LEVELS))
    for kernel in ("estimate", "std_af"):
        if not any(kernel in c["sensitive"] for c in index):
            sys.exit("refused: the contracting and the non-contracting build agree on every %s case" % kernel)
    arrays["index"] = np.frombuffer(json.dumps(index).encode(), np.uint8)
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    if buf.tell() > SIZE_CAP:
        sys.exit("refused: the file would have %d bytes, over the cap of %d" % (buf.tell(), SIZE_CAP))
    with open(rc.FIXTURE, "wb") as f:
        f.write(buf.getvalue())
    print("wrote %s: %d bytes, %d cases, %d kernel runs" % (os.path.relpath(rc.FIXTURE, ROOT), buf.tell(), len(index),
                                                           sum(len(c["kernels"]) for c in index)))


if __name__ == "__main__":
    main()
