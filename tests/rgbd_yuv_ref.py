"""lfi_download_rgbd_yuv restated: by definition the frame is lfi_download_quilt_yuv's frame (tests/quilt_yuv_ref.py) of the 2 x 1 quilt {view, grey
image of the depth}.  This file builds that quilt and restates nothing itself."""
import numpy as np

import quilt_yuv_ref


def grey(map_plane, invert=False):
    """the RGBA image (d, d, d, 255) of d = M or 255 - M, M the R byte plane of map_plane [H][W][4]"""
    d = np.asarray(map_plane)[..., 0].astype(np.uint8)
    if invert:
        d = (255 - d.astype(np.int64)).astype(np.uint8)   # before the resize
    out = np.repeat(d[..., None], 4, axis=2)
    out[..., 3] = 255
    return out


def frame(view, map_plane, tile_w, tile_h, invert, matrix, rng):
    """the tight I420 frame [frame_bytes] of 2·tile_w x tile_h: view [H][W][4] left, the depth of map_plane [H][W][4] right"""
    return quilt_yuv_ref.frame(np.stack([view, grey(map_plane, invert)]), 2, 1, tile_w, tile_h, matrix, rng)
