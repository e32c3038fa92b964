"""The cases of tests/golden/ref_kernels.npz — outputs recorded from the reference's own kernels, run on the CPU (oracle/ref_kernels.py)
— and how a test reads them.  tests/golden/make_ref_kernel_golden.py writes the file from CASES; tests/test_ref_kernels.py (CPU) and
tests/test_gpu_ref_kernels.py (GPU) read it and need neither the reference tree nor the library.

Per case the file holds the parameter arrays the kernels were given (they come from the oracle's host functions: data), the input
recipe, the maps whole and, per blend kernel, the SHA-256 of each of the 64 views (RGBA bytes) with views 0 and 63 whole.  Alpha is
255 and a map is grey in every pixel the reference writes, so views are stored as RGB and maps as one channel; the hashes cover RGBA.
"""
import hashlib
import json
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_kernels.npz")
VIEWS = 64

# inputs: synthetic_lf(N, W, H, seed), colour bytes rounded down to multiples of `quant`, then the column bands [x0, x1) set to a flat value
# in EVERY image (0: black — the reference's maxCol starts at FLT_MIN, so an all-black tap has a dispersion of FLT_MIN, not 0)
BANDS_8X16 = [[0, 60, 64], [60, 100, 0]]

# name, cols, rows, W, H, trajectory, focus, range, aspect, effect, block radius, input (seed, quant, bands), map seeds (map 0, map 1), kernels
CASES = [
    # one batch of 16 images
    dict(name="g4x4_48x20", grid=(4, 4), size=(48, 20), traj="0,0,1,1", focus=0.31, range=0.0, aspect=1.5, effect=3.0, radius=None,
         seed=11, quant=1, bands=[], map_seeds=None, kernels=["std", "ten"]),
    # effect 7: subnormal fp16 weights
    dict(name="g8x8_48x20_e7", grid=(8, 8), size=(48, 20), traj="0.071,0.071,0.93,0.93", focus=0.23, range=0.0, aspect=1.783, effect=7.0,
         radius=None, seed=12, quant=1, bands=[], map_seeds=None, kernels=["std", "ten"]),
    # focus 1.1: the integer offsets carry most samples beyond the image, where the surface clamp applies
    dict(name="g8x8_48x20_e7_far", grid=(8, 8), size=(48, 20), traj="0.071,0.071,0.93,0.93", focus=1.1, range=0.0, aspect=1.783, effect=7.0,
         radius=None, seed=12, quant=1, bands=[], map_seeds=None, kernels=["std", "ten"]),
    # the parameters at which floating-point contraction is observable; negative focus
    dict(name="g8x4_100x50", grid=(8, 4), size=(100, 50), traj="0,0,1,1", focus=-0.1, range=0.7, aspect=1.5, effect=1.0, radius=(15, 25),
         seed=78, quant=1, bands=[], map_seeds=(79, 80), kernels=["estimate", "filter", "std_af"]),
    # the same grid at a width the tensor kernel can do; map 1 differs from map 0, which it reads
    dict(name="g8x4_96x50", grid=(8, 4), size=(96, 50), traj="0,0,1,1", focus=-0.1, range=0.7, aspect=1.5, effect=1.0, radius=(15, 25),
         seed=78, quant=1, bands=[], map_seeds=(79, 80), kernels=["ten_af"]),
    # 128 images, ragged edge blocks; inputs in steps of 16 (ties between focus steps) and partly flat or black (the FLT_MIN start); the
    # trajectory's centre lies outside the grid, so all offsets point one way and whole taps stay inside one band
    dict(name="g8x16_130x37_focus", grid=(8, 16), size=(130, 37), traj="-0.5,-0.5,-0.5,-0.5", focus=0.05, range=0.9, aspect=1.783,
         effect=3.0, radius=(20, 12), seed=13, quant=16, bands=BANDS_8X16, map_seeds=None, kernels=["estimate", "filter"]),
    # the same images blended; negative range
    dict(name="g8x16_130x37", grid=(8, 16), size=(130, 37), traj="0.071,0.071,0.93,0.93", focus=0.2, range=-0.45, aspect=1.783, effect=3.0,
         radius=None, seed=13, quant=16, bands=BANDS_8X16, map_seeds=(81, 82), kernels=["std", "std_af"]),
    # 256 images: MAX_IMAGES
    dict(name="g16x16_32x18", grid=(16, 16), size=(32, 18), traj="0,0,1,1", focus=0.25, range=0.5, aspect=1.5, effect=3.0, radius=None,
         seed=15, quant=1, bands=[], map_seeds=(83, 84), kernels=["std", "ten", "std_af", "ten_af"]),
]


def inputs(oracle, case):
    """The case's light field [N][H][W][4] from its recipe (oracle: either oracle module, for synthetic_lf)."""
    (cols, rows), (W, H) = case["grid"], case["size"]
    lf = oracle.synthetic_lf(cols * rows, W, H, case["seed"]).copy()
    q = int(case["quant"])
    if q > 1:
        lf[..., :3] = (lf[..., :3] // q) * q
    for x0, x1, value in case["bands"]:
        lf[:, :, x0:x1, :3] = value
    return lf


def noise_map(oracle, case, k):
    """Input map k of an all-focus case: one channel of synthetic noise, [H][W]."""
    W, H = case["size"]
    return oracle.synthetic_lf(1, W, H, case["map_seeds"][k])[0, :, :, 0].copy()


def grey(plane):
    """[H][W] → the RGBA map the kernels read and write: grey, opaque."""
    out = np.empty(plane.shape + (4,), np.uint8)
    out[..., :3] = plane[..., None]
    out[..., 3] = 255
    return out


def rgba(rgb):
    """[H][W][3] → the RGBA view the kernels write: opaque."""
    out = np.full(rgb.shape[:2] + (4,), 255, np.uint8)
    out[..., :3] = rgb
    return out


def view_hashes(views):
    """[V][H][W][4] → [V][32] u8: SHA-256 of each view's RGBA bytes."""
    return np.array([np.frombuffer(hashlib.sha256(np.ascontiguousarray(v, np.uint8).tobytes()).digest(), np.uint8) for v in views])


class Fixture:
    """tests/golden/ref_kernels.npz, read once."""

    def __init__(self, path=FIXTURE):
        with np.load(path) as z:
            self.arrays = {k: z[k] for k in z.files}
        self.cases = json.loads(bytes(self.arrays.pop("index")).decode())

    def case(self, name):
        return next(c for c in self.cases if c["name"] == name)

    def pairs(self):
        return [(c["name"], k) for c in self.cases for k in c["kernels"]]

    def array(self, case, key):
        return self.arrays[case["name"] + "." + key]

    def map_in(self, case, k):
        """Input map k of an all-focus case, RGBA."""
        return grey(self.array(case, "map%d" % k))

    def map_out(self, case, kernel):
        """The reference's estimate or filter output, RGBA."""
        return grey(self.array(case, kernel + ".map"))

    def params(self, case):
        """The parameter arrays the reference's kernels were given, as a lfinterpolator_amd.host.HostParams."""
        from lfinterpolator_amd.host import HostParams
        ids = self.array(case, "ids")
        radius = np.array(case["radius"] or [1, 1], np.int32)
        return HostParams(self.array(case, "focused"), self.array(case, "offsets"), self.array(case, "weights"), ids, float(np.float32(case["focus"])),
                          float(np.float32(case["range"])), radius)

    def check_views(self, case, kernel, views, what=""):
        """views [64][H][W][4] against the reference's: every hash, and views 0 and 63 byte for byte."""
        assert views.shape[0] == VIEWS
        want = self.array(case, kernel + ".hashes")
        got = view_hashes(views)
        bad = [v for v in range(VIEWS) if not (got[v] == want[v]).all()]
        for v in (0, VIEWS - 1):
            full = rgba(self.array(case, "%s.view%d" % (kernel, v)))
            diff = int((views[v] != full).sum())
            assert diff == 0, (case["name"], kernel, what, "view %d differs from the reference's in %d bytes" % (v, diff))
        assert not bad, (case["name"], kernel, what, "views whose SHA-256 differs from the reference's", bad[:8], len(bad))
