"""Generates tests/golden/codec_stb.npz: what the reference's own codec (stb_image / stb_image_write, built into
oracle/_ref/libref_codec.so by `make -C oracle ref`) makes of the files tests/test_host_io.py writes — the checker of
csrc/host/image_io.cpp and jpeg.cpp, stored so that those tests do not need the reference tree.

Keys (every value a numpy array; the files themselves are written by the tests' own helpers, here as there):
  png_<case>_want                              stbi_load(…, 4) of test_host_io._png_cases' files (PNG is lossless: the
                                               result depends on the image, not on the encoder)
  writer_ours_file                             csrc/host's write_png of WRITER_ARR (stbi_load gives WRITER_ARR back, checked here)
  writer_theirs_file                           stbi_write_png of WRITER_ARR
  adam7_<shape>_want                           stbi_load of test_host_io._adam7_png(_rand(*shape, 21))
  jpeg_<kind>_<h>x<w>_{file_sha256,sha256,shape}  per JPEG of test_jpeg_decode_matches_reference_codec: SHA-256 of the file Pillow
                                               wrote (its decode depends on every encoder choice), SHA-256 and shape of stbi_load's RGBA
  jpegcm_<name>_…, grid_<row>_<col>_…          the same for the Adobe-marked JPEGs and the JPEG grid of the loader test

Run from the repository root after `__graft_entry__.build()`, where the reference tree is present (build() then makes
oracle/_ref/):  python tests/golden/make_codec_golden.py
"""
import hashlib
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from conftest import GOLDEN_DIR  # noqa: E402
from oracle import ref_codec  # noqa: E402
from test_host_io import (ADAM7_SHAPES, CODEC_GOLDEN, JPEG_KINDS, JPEG_SIZES, WRITER_ARR, _adam7_png, _jpeg_colour_model_files,  # noqa: E402
                          _jpeg_file, _jpeg_grid, _png_cases, _rand)
import lfinterpolator_amd as L  # noqa: E402


def main():
    ref_codec.lib()                     # raises unless oracle/_ref/libref_codec.so is built
    out = {}

    def digests(key, path):
        rgba = ref_codec.load_rgba(path)
        out[key + "_file_sha256"] = np.array(hashlib.sha256(open(path, "rb").read()).hexdigest())
        out[key + "_sha256"] = np.array(hashlib.sha256(rgba.tobytes()).hexdigest())
        out[key + "_shape"] = np.array(rgba.shape)

    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        for name, path in _png_cases(tmp).items():
            out[f"png_{name}_want"] = ref_codec.load_rgba(path)

        ours = str(tmp / "ours.png")
        L.write_png(ours, WRITER_ARR)
        assert (ref_codec.load_rgba(ours) == WRITER_ARR).all(), "the reference's decoder does not read our PNG writer's file"
        out["writer_ours_file"] = np.fromfile(ours, dtype=np.uint8)
        theirs = str(tmp / "theirs.png")
        ref_codec.write_png(theirs, WRITER_ARR)
        out["writer_theirs_file"] = np.fromfile(theirs, dtype=np.uint8)

        for shape in ADAM7_SHAPES:
            path = str(tmp / "adam7.png")
            with open(path, "wb") as f:
                f.write(_adam7_png(_rand(*shape, 21)))
            out["adam7_" + "x".join(map(str, shape)) + "_want"] = ref_codec.load_rgba(path)

        for size in JPEG_SIZES:
            for kind in JPEG_KINDS:
                digests(f"jpeg_{kind}_{size[0]}x{size[1]}", _jpeg_file(tmp / f"{kind}.jpg", kind, size))
        for name, path in _jpeg_colour_model_files(tmp).items():
            digests(f"jpegcm_{name}", path)
        _jpeg_grid(tmp)
        for col in range(2):
            for row in range(3):
                digests(f"grid_{row}_{col}", str(tmp / f"{row}_{col}.jpg"))

    assert os.path.dirname(CODEC_GOLDEN) == GOLDEN_DIR
    np.savez_compressed(CODEC_GOLDEN, **out)
    print(f"wrote {CODEC_GOLDEN}: {len(out)} arrays, {os.path.getsize(CODEC_GOLDEN)} bytes")


if __name__ == "__main__":
    main()
