"""The derived planar copy of the inputs (csrc/hip/blend_planar.hpp planar_build, csrc/hip/yuv_derived.hpp) restated in numpy:
per image three byte planes (R, G, B) whose rows are padded on both sides with their edge pixels,

    plane[g][c][y][j] = image[g][y][clamp(j - padx - phase[g], 0, W - 1)][c]        for every j in [0, pitch)

`layout` is what Context.derived_layout() returns (pitch_bytes, rows, padx) or anything with those attributes."""
import numpy as np


def planes(images_rgba, layout, phases):
    """[N][3][rows][pitch] uint8 from images [N][H][W][4] uint8, H = layout.rows"""
    images = np.asarray(images_rgba, np.uint8)
    n, h, w, _ = images.shape
    assert h == layout.rows and len(phases) == n
    j = np.arange(layout.pitch_bytes)
    out = np.empty((n, 3, h, layout.pitch_bytes), np.uint8)
    for g in range(n):
        x = np.clip(j - layout.padx - int(phases[g]), 0, w - 1)
        out[g] = images[g][:, x, :3].transpose(2, 0, 1)
    return out
