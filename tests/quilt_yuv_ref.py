"""lfi_download_quilt_yuv restated: the definition is a composition of two that are restated already — tests/scaled_quilt_ref.py's quilt, taken as
one view by tests/yuv_ref.py's frame.  tests/yuv_surfaces_ref.py places the bytes (NV12 re-interleaved, pitches, offsets)."""
import scaled_quilt_ref
import yuv_ref


def frame(views, tiles_x, tiles_y, tile_w, tile_h, matrix, rng):
    """the tight I420 frame [frame_bytes] of the quilt of the first tiles_x·tiles_y of views [V][H][W][4]"""
    return yuv_ref.frame(scaled_quilt_ref.quilt(views, tiles_x, tiles_y, tile_w, tile_h), matrix, rng)
