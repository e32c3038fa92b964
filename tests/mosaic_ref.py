"""Mosaic input (include/lfi.h: lfi_mosaic, lfi_mosaic_map, lfi_upload_mosaic_yuv, lfi_upload_mosaic) in numpy: the mapping of a frame's tiles
onto the grid's images, restated from the header's text, and the crops of the tiles.  No arithmetic of its own: a tile's Y, Cb and Cr are
cut out of the frame's planes, packed into a tight frame and handed to tests/yuv_in_ref.py (centre siting) or tests/yuv_left_ref.py (left
siting) as they are.  Shares no code with the product."""
import numpy as np

import yuv_in_ref as in_ref
import yuv_left_ref as left_ref

ROWS, GRID = 0, 1        # LFI_MOSAIC_ROWS, LFI_MOSAIC_GRID
BOTTOM_UP = 1            # LFI_MOSAIC_BOTTOM_UP


def mosaic_map(tiles_x, tiles_y, first_tile, n, order, flags, cols, rows, g0):
    """[n][3] int64, row k = (tx, ty, g) of tile first_tile + k — or None where lfi_mosaic_map refuses the mosaic"""
    if tiles_x < 1 or tiles_y < 1 or cols < 1 or rows < 1 or order not in (ROWS, GRID) or flags & ~BOTTOM_UP:
        return None
    if n < 1 or first_tile < 0 or first_tile + n > tiles_x * tiles_y or g0 < 0 or g0 + n > cols * rows:
        return None
    if order == GRID and (tiles_x != cols or tiles_y != rows or first_tile != 0 or n != cols * rows or g0 != 0):
        return None
    out = np.empty((n, 3), np.int64)
    for k in range(n):
        t = first_tile + k
        tx, r = t % tiles_x, t // tiles_x
        ty = tiles_y - 1 - r if flags & BOTTOM_UP else r
        out[k] = tx, ty, (tx * rows + r if order == GRID else g0 + k)
    return out


def tile_frame(frame, mw, mh, w, h, tx, ty):
    """the tight I420 frame of tile (tx, ty) of a tight I420 frame of mw x mh; w and h even"""
    assert w % 2 == 0 and h % 2 == 0
    y, cb, cr = in_ref.split(frame, mw, mh)
    return in_ref.pack(y[ty * h:(ty + 1) * h, tx * w:(tx + 1) * w], cb[ty * h // 2:(ty + 1) * h // 2, tx * w // 2:(tx + 1) * w // 2],
                       cr[ty * h // 2:(ty + 1) * h // 2, tx * w // 2:(tx + 1) * w // 2])


def expand(frame, mw, mh, w, h, tiles, matrix, rng, chroma=in_ref.BILINEAR, left=False):
    """{g: [h][w][4] uint8}: the images the tight I420 frame of mw x mh gives under the map `tiles` ([n][3] of mosaic_map) — every tile taken
    as a frame of its own, under centre (tests/yuv_in_ref.py) or left (tests/yuv_left_ref.py) siting"""
    ref = left_ref if left else in_ref
    return {int(g): ref.rgba(tile_frame(frame, mw, mh, w, h, int(tx), int(ty)), w, h, matrix, rng, chroma) for tx, ty, g in tiles}


def rgba_tiles(image, w, h, tiles):
    """{g: [h][w][4]}: the crops of an RGBA mosaic image [tiles_y * h][>= tiles_x * w][4]"""
    return {int(g): image[ty * h:(ty + 1) * h, tx * w:(tx + 1) * w] for tx, ty, g in tiles}
