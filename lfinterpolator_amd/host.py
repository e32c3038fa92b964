"""ctypes binding of the C++ host parameterisation (lib/liblfi_host.so, csrc/host/params.cpp)."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from .abi import LFI_LENT_BGR, LFI_LENT_INVERT, Lenticular, Mosaic, YuvSurfaces
from .abi import mosaic_map as _abi_mosaic_map
from .build import HOST_LIB

_lib = None


def load_host_library() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(HOST_LIB):
            raise RuntimeError(f"{HOST_LIB} is missing: run __graft_entry__.build()")
        lib = C.CDLL(HOST_LIB)
        lib.lfi_host_build_params.restype = C.c_int
        lib.lfi_host_build_params.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_float, C.c_float,
                                              C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32 * 2), C.c_char_p,
                                              C.c_size_t]
        lib.lfi_host_focus_ramp.restype = C.c_int
        lib.lfi_host_focus_ramp.argtypes = [C.c_float, C.c_float, C.c_int, C.c_void_p]
        lib.lfi_host_focus_candidates.restype = C.c_int
        lib.lfi_host_focus_candidates.argtypes = [C.c_float, C.c_float, C.c_int, C.c_void_p]
        lib.lfi_host_focus_tile_rect.restype = C.c_int
        lib.lfi_host_focus_tile_rect.argtypes = [C.c_int] * 6 + [C.c_void_p]
        lib.lfi_host_focus_auto_range.restype = C.c_int
        lib.lfi_host_focus_auto_range.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p]
        lib.lfi_host_focus_auto_range_steps.restype = C.c_int
        lib.lfi_host_focus_auto_range_steps.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                        C.c_void_p]
        lib.lfi_host_area_span.restype = C.c_int
        lib.lfi_host_area_span.argtypes = [C.c_int] * 3 + [C.c_void_p]
        lib.lfi_host_lenticular.restype = C.c_int
        lib.lfi_host_lenticular.argtypes = [C.c_double] * 4 + [C.c_int] * 4 + [C.POINTER(Lenticular), C.c_char_p, C.c_size_t]
        lib.lfi_host_lenticular_json.restype = C.c_int
        lib.lfi_host_lenticular_json.argtypes = [C.c_char_p] + [C.c_int] * 3 + [C.POINTER(Lenticular), C.c_void_p, C.c_char_p, C.c_size_t]
        lib.lfi_host_native_taps.restype = C.c_int
        lib.lfi_host_native_taps.argtypes = [C.c_int] * 3 + [C.c_void_p]
        lib.lfi_host_linear_tables.restype = C.c_int
        lib.lfi_host_linear_tables.argtypes = [C.c_void_p, C.c_void_p]
        lib.lfi_host_linear_encode.restype = C.c_int
        lib.lfi_host_linear_encode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        lib.lfi_host_y4m_frame_bytes.restype = C.c_size_t
        lib.lfi_host_y4m_frame_bytes.argtypes = [C.c_int, C.c_int]
        lib.lfi_host_y4m_write.restype = C.c_int
        lib.lfi_host_y4m_write.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_size_t] + [C.c_int] * 5 + [C.c_char_p, C.c_size_t]
        lib.lfi_host_y4m_write_sited.restype = C.c_int
        lib.lfi_host_y4m_write_sited.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_size_t] + [C.c_int] * 6 + [C.c_char_p, C.c_size_t]
        lib.lfi_host_y4m_frame_bytes_deep.restype = C.c_size_t
        lib.lfi_host_y4m_frame_bytes_deep.argtypes = [C.c_int, C.c_int, C.c_int]
        lib.lfi_host_y4m_write_deep.restype = C.c_int
        lib.lfi_host_y4m_write_deep.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_size_t] + [C.c_int] * 7 + [C.c_char_p, C.c_size_t]
        lib.lfi_host_y4m_info_deep.restype = C.c_int
        lib.lfi_host_y4m_info_deep.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
        lib.lfi_host_y4m_read_deep.restype = C.c_int
        lib.lfi_host_y4m_read_deep.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
        lib.lfi_host_y4m_input_siting.restype = C.c_int
        lib.lfi_host_y4m_input_siting.argtypes = [C.c_char_p, C.c_int]
        lib.lfi_host_y4m_info.restype = C.c_int
        lib.lfi_host_y4m_info.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
        lib.lfi_host_y4m_read.restype = C.c_int
        lib.lfi_host_y4m_read.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
        lib.lfi_host_load_grid_y4m.restype = C.c_int
        lib.lfi_host_load_grid_y4m.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
        lib.lfi_host_build_view_offsets.restype = C.c_int
        lib.lfi_host_build_view_offsets.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_float, C.c_void_p, C.c_int,
                                                    C.c_void_p, C.c_char_p, C.c_size_t]
        lib.lfi_host_build_view_centred_offsets.restype = C.c_int
        lib.lfi_host_build_view_centred_offsets.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_float, C.c_void_p, C.c_int,
                                                            C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
        lib.lfi_host_build_view_focus_ids.restype = C.c_int
        lib.lfi_host_build_view_focus_ids.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_void_p, C.POINTER(C.c_int32), C.c_char_p,
                                                      C.c_size_t]
        lib.lfi_host_float_to_half.restype = C.c_uint16
        lib.lfi_host_float_to_half.argtypes = [C.c_float]
        lib.lfi_host_half_to_float.restype = C.c_float
        lib.lfi_host_half_to_float.argtypes = [C.c_uint16]
        lib.lfi_host_load_image.restype = C.c_int
        lib.lfi_host_load_image.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_char_p, C.c_size_t]
        lib.lfi_host_write_png.restype = C.c_int
        lib.lfi_host_write_png.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_char_p, C.c_size_t]
        lib.lfi_host_load_grid.restype = C.c_int
        lib.lfi_host_load_grid.argtypes = [C.c_char_p] + [C.POINTER(C.c_int)] * 4 + [C.c_void_p, C.c_char_p, C.c_size_t]
        _lib = lib
    return _lib


@dataclass
class HostParams:
    """The reference's per-launch parameter block (src/kernels.cu:15-17, 63-69 + the weight matrix)."""
    focused_offsets: np.ndarray  # [N][2] int32
    offsets: np.ndarray          # [N][2] float32
    weights: np.ndarray          # [V][N] uint16 (fp16 bits)
    focus_map_ids: np.ndarray    # [≤32] int32
    focus: float
    range: float
    block_radius: np.ndarray     # [2] int32

    def rows(self, v0: int, v1: int) -> "HostParams":
        """The same block restricted to the weight rows [v0, v1) — what one rank of a view-sharded job needs."""
        return HostParams(self.focused_offsets, self.offsets, np.ascontiguousarray(self.weights[v0:v1]),
                          self.focus_map_ids, self.focus, self.range, self.block_radius)


def build_params(cols: int, rows: int, width: int, height: int, trajectory: str, focus: float = 0.0, range: float = 0.0,
                 effect: float = 3.0, aspect: float = 1.0, views: int = 64) -> HostParams:
    """What Interpolator::interpolate prepares before its launches (reference src/interpolator.cu:250-256)."""
    lib = load_host_library()
    n = cols * rows
    foc = np.zeros((n, 2), dtype=np.int32)
    off = np.zeros((n, 2), dtype=np.float32)
    w = np.zeros((max(views, 1), n), dtype=np.uint16)
    ids = np.zeros(32, dtype=np.int32)
    n_ids = C.c_int32()
    radius = (C.c_int32 * 2)()
    err = C.create_string_buffer(512)
    rc = lib.lfi_host_build_params(cols, rows, width, height, trajectory.encode(), focus, range, effect, aspect, views,
                                   foc.ctypes.data, off.ctypes.data, w.ctypes.data, ids.ctypes.data, C.byref(n_ids),
                                   C.byref(radius), err, len(err))
    if rc != 0:
        raise ValueError(err.value.decode())
    return HostParams(foc, off, w, ids[:n_ids.value].copy(), focus, range, np.array([radius[0], radius[1]], np.int32))


def focus_ramp(f0: float, f1: float, views: int) -> np.ndarray:
    """Per-view focus values from f0 (first view) to f1 (last view): f0 + ((f1 − f0) / (views − 1))·i in float32 (one view: f0)."""
    out = np.zeros(max(views, 1), dtype=np.float32)
    if load_host_library().lfi_host_focus_ramp(f0, f1, views, out.ctypes.data) != 0:
        raise ValueError("views must be positive")
    return out


def focus_candidates(focus: float, range: float, steps: int = 32) -> np.ndarray:
    """The focus candidates of Context.focus_curve (for 32 steps: of the focus-map estimate): fmaf(range / (steps − 1), i, focus) in float32."""
    out = np.zeros(max(steps, 0), dtype=np.float32)
    if load_host_library().lfi_host_focus_candidates(focus, range, steps, out.ctypes.data) != 0:
        raise ValueError("steps must be at least 2")
    return out


def focus_tile_rect(width: int, height: int, tiles_x: int, tiles_y: int, tx: int, ty: int):
    """Tile (tx, ty) of Context.focus_tiles' grid as (x0, y0, x1, y1): x0 = tx·width // tiles_x, x1 = (tx + 1)·width // tiles_x, likewise in y."""
    rect = np.zeros(4, dtype=np.int32)
    if load_host_library().lfi_host_focus_tile_rect(width, height, tiles_x, tiles_y, tx, ty, rect.ctypes.data) != 0:
        raise ValueError("the grid must fit the frame and the tile the grid")
    return tuple(int(v) for v in rect)


def focus_auto_range(best_index, focus: float, range: float, steps: int = 32):
    """The interval an all-focus render should search, from the tiles' best candidates of a search over [focus, focus + range] with `steps`
    candidates (Context.focus_tiles' steps: a multiple of 32 from 32 to 256): returns (focus', range' as np.float32, lo', hi') with
    lo' = max(min − 1, 0), hi' = min(max + 1, steps − 1), focus' = candidate lo', range' = candidate hi' − candidate lo' in float32,
    the candidates those of focus_candidates(focus, range, steps)."""
    idx = np.ascontiguousarray(best_index, dtype=np.int32).reshape(-1)
    f, r = C.c_float(), C.c_float()
    lo_hi = np.zeros(2, dtype=np.int32)
    lib = load_host_library()
    if steps == 32:
        rc = lib.lfi_host_focus_auto_range(idx.ctypes.data, len(idx), focus, range, C.byref(f), C.byref(r), lo_hi.ctypes.data)
    else:
        rc = lib.lfi_host_focus_auto_range_steps(idx.ctypes.data, len(idx), steps, focus, range, C.byref(f), C.byref(r), lo_hi.ctypes.data)
    if rc != 0:
        raise ValueError(f"needs at least one tile, steps a multiple of 32 from 32 to 256, indices in [0, {steps - 1}] and range > 0")
    return np.float32(f.value), np.float32(r.value), int(lo_hi[0]), int(lo_hi[1])


def area_span(src: int, dst: int, o: int):
    """Output pixel o of Context.download_quilt_scaled's area resize along an axis of src source and dst output pixels, as (first, last,
    w_first, w_last): the source pixels it overlaps on the grid of src·dst units and the overlaps with the first and the last one (every
    source pixel between them weighs dst) — the arithmetic the kernel runs."""
    out = np.zeros(4, dtype=np.int32)
    if load_host_library().lfi_host_area_span(src, dst, o, out.ctypes.data) != 0:
        raise ValueError("needs 1 <= dst <= src <= 65535 and 0 <= o < dst")
    return tuple(int(v) for v in out)


def lenticular(pitch: float, slope: float, center: float, dpi: float, invert: bool, out_w: int, out_h: int, n: int) -> Lenticular:
    """A lenticular display's calibration (lenses per inch, slant, phase offset in lens periods, pixels per inch, reversed view order) as the
    Lenticular Context.download_native takes, for an out_w × out_h image interlacing n views (csrc/host/lenticular.h: doubles, +, −, ×, ÷ and sqrt)."""
    lens = Lenticular()
    err = C.create_string_buffer(512)
    if load_host_library().lfi_host_lenticular(pitch, slope, center, dpi, int(bool(invert)), out_w, out_h, n, C.byref(lens), err, len(err)) != 0:
        raise ValueError(err.value.decode())
    assert lens.flags == (LFI_LENT_INVERT if invert else 0)
    return lens


def lenticular_file(path, out_w: int, out_h: int, n: int, with_screen: bool = False):
    """lenticular() from a display's calibration file (csrc/host/lenticular.h): a flat JSON object whose numeric entries are "name": x or
    "name": {"value": x}; pitch, slope, center and DPI are the calibration, invView sets LFI_LENT_INVERT and flipSubp LFI_LENT_BGR in the
    Lenticular's flags.  with_screen: returns (Lenticular, (screenW, screenH)) — the panel's size as the file states it, 0 where it does not.
    ValueError, naming the key, for a file that cannot be read, a key without a number, a missing key and a mirrored panel (flipImageX / Y)."""
    lens = Lenticular()
    screen = np.zeros(2, dtype=np.int32)
    err = C.create_string_buffer(512)
    if load_host_library().lfi_host_lenticular_json(os.fsencode(path), out_w, out_h, n, C.byref(lens), screen.ctypes.data, err, len(err)) != 0:
        raise ValueError(err.value.decode())
    assert lens.flags & ~(LFI_LENT_INVERT | LFI_LENT_BGR) == 0
    return (lens, (int(screen[0]), int(screen[1]))) if with_screen else lens


def native_taps(src: int, dst: int, o: int):
    """Output pixel o of Context.download_native's bilinear tile sampling (LFI_LENT_BILINEAR) along an axis of src tile and dst output pixels,
    as (p0, p1, f): the two tile pixels and the weight of p1 in 1/256 (p0 weighs 256 − f) — the arithmetic the kernel runs (csrc/native_taps.h)."""
    out = np.zeros(3, dtype=np.int32)
    if load_host_library().lfi_host_native_taps(src, dst, o, out.ctypes.data) != 0:
        raise ValueError("needs 1 <= src, dst <= 65535 and 0 <= o < dst")
    return tuple(int(v) for v in out)


def linear_tables():
    """The tables of linear-light blending (LFI_FLAG_LINEAR_LIGHT, csrc/linear_light.h) as the library holds them: (D, T) — D [256] uint16, the
    fp16 bit patterns of the decode table; T [256] uint32, the fp32 bit patterns of the thresholds (T[0] is a placeholder, 0)."""
    d, t = np.zeros(256, dtype=np.uint16), np.zeros(256, dtype=np.uint32)
    if load_host_library().lfi_host_linear_tables(d.ctypes.data, t.ctypes.data) != 0:
        raise ValueError("lfi_host_linear_tables failed")
    return d, t


def linear_encode(s) -> np.ndarray:
    """E(s) of linear-light blending for every float32 of s, by the epilogue the kernel runs (csrc/linear_light.h: linear_encode over the
    first-guess table linear_guess builds): uint8, the shape of s."""
    s = np.ascontiguousarray(s, dtype=np.float32)
    out = np.zeros(s.shape, dtype=np.uint8)
    if load_host_library().lfi_host_linear_encode(s.ctypes.data, s.size, out.ctypes.data) != 0:
        raise ValueError("lfi_host_linear_encode failed")
    return out


def write_y4m(path: str, frames: np.ndarray, width: int, height: int, fps=(30, 1), full_range: bool = False, left_sited: bool = False, depth: int = 8) -> None:
    """The I420 frames of Context.download_views_yuv420 / render_stream_yuv420 — [n][P] uint8 with rows of P ≥ frame bytes, the frame stride is
    the array's — as one Y4M file (csrc/host/y4m.h): `YUV4MPEG2 W H F<fps> Ip A1:1 C420jpeg XCOLORRANGE=LIMITED|FULL`, then `FRAME` + the
    frame's bytes per frame.  fps: (numerator, denominator).  left_sited: the frames were made under Context.set_yuv_siting(out_siting="left"),
    the header says C420mpeg2.  depth=10: the frames are I010 (every sample a little-endian u16, twice the bytes), the header says C420p10
    whatever the siting."""
    lib = load_host_library()
    if depth != 8:
        frames = np.asarray(frames)
        if frames.dtype != np.uint8 or frames.ndim != 2 or (frames.size and frames.strides[1] != 1):
            raise ValueError("frames must be [n][>= frame bytes] uint8 with contiguous rows")
        err = C.create_string_buffer(512)
        if lib.lfi_host_y4m_write_deep(str(path).encode(), frames.ctypes.data_as(C.c_void_p), frames.shape[0], frames.strides[0] if frames.size else 0, width,
                                       height, int(fps[0]), int(fps[1]), int(bool(full_range)), int(bool(left_sited)), int(depth), err, len(err)) != 0:
            raise ValueError(err.value.decode())
        return
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim != 2 or (frames.size and frames.strides[1] != 1):
        raise ValueError("frames must be [n][>= frame bytes] uint8 with contiguous rows")
    if frames.shape[1] < lib.lfi_host_y4m_frame_bytes(width, height):
        raise ValueError(f"a {width}x{height} frame has {lib.lfi_host_y4m_frame_bytes(width, height)} bytes, the rows have {frames.shape[1]}")
    err = C.create_string_buffer(512)
    head = (str(path).encode(), frames.ctypes.data_as(C.c_void_p), frames.shape[0], frames.strides[0] if frames.size else 0, width, height, int(fps[0]),
            int(fps[1]), int(bool(full_range)))
    if left_sited:
        rc = lib.lfi_host_y4m_write_sited(*head, 1, err, len(err))
    else:
        rc = lib.lfi_host_y4m_write(*head, err, len(err))
    if rc != 0:
        raise ValueError(err.value.decode())


def mosaic_map(tiles_x: int, tiles_y: int, cols: int, rows: int, order="rows", bottom_up: bool = False, first_tile: int = 0, n: int | None = None,
               g0: int = 0) -> np.ndarray:
    """Where the tiles of a mosaic frame go (lfi_mosaic_map, include/lfi.h): [n][3] int32, row k = (tx, ty, g) — tile k's column and row in
    the frame of tiles_x × tiles_y tiles and the image it becomes in a cols × rows grid."""
    return _abi_mosaic_map(Mosaic.make(tiles_x, tiles_y, order, bottom_up, first_tile, n), cols, rows, g0)


def _tight_mosaic_surfaces(ctx, frame: np.ndarray, tiles_x: int, tiles_y: int, fmt) -> YuvSurfaces:
    """one tight host frame of tiles_x·W × tiles_y·H as surfaces"""
    assert frame.dtype == np.uint8 and frame.ndim == 1 and frame.strides[0] == 1
    mw, mh = tiles_x * ctx.width, tiles_y * ctx.height
    assert frame.size >= mw * mh * 3 // 2
    nv12 = fmt in ("nv12", 1)
    return YuvSurfaces.make(fmt, "host", frame.ctypes.data, frame.size, mw, mw * mh, mw if nv12 else mw // 2,
                            0 if nv12 else mw * mh + (mw // 2) * (mh // 2), keep=frame)


def upload_mosaic_yuv(ctx, frame: np.ndarray, tiles_x: int, tiles_y: int, fmt="i420", order="grid", bottom_up: bool = False, matrix="709",
                      range="limited", chroma="bilinear") -> None:
    """Context.upload_mosaic_yuv of one tight host frame ([frame bytes] uint8: I420 or NV12 planes of tiles_x·W × tiles_y·H) that holds the
    whole grid of ctx: order "grid" for a cols × rows mosaic of cameras, "rows" for a quilt.  Keep `frame` alive until upload_wait / sync."""
    s = _tight_mosaic_surfaces(ctx, frame, tiles_x, tiles_y, fmt)
    ctx.upload_mosaic_yuv(Mosaic.make(tiles_x, tiles_y, order, bottom_up), s, 0, matrix, range, chroma)


def upload_mosaic_yuv_derived(ctx, frame: np.ndarray, tiles_x: int, tiles_y: int, fmt="i420", order="grid", bottom_up: bool = False, matrix="709",
                              range="limited", chroma="bilinear") -> None:
    """upload_mosaic_yuv for a context whose inputs were released (Context.upload_mosaic_yuv_derived): the same tight host frame goes
    straight into the derived planar copy.  Keep `frame` alive until upload_wait / sync."""
    s = _tight_mosaic_surfaces(ctx, frame, tiles_x, tiles_y, fmt)
    ctx.upload_mosaic_yuv_derived(Mosaic.make(tiles_x, tiles_y, order, bottom_up), s, 0, matrix, range, chroma)


def upload_mosaic(ctx, rgba: np.ndarray, tiles_x: int, tiles_y: int, order="grid", bottom_up: bool = False) -> None:
    """Context.upload_mosaic of one host RGBA image (tiles_y·H, tiles_x·W, 4) that holds the whole grid of ctx, e.g. a quilt loaded with
    load_image (order "rows", bottom_up for a Looking-Glass quilt).  Keep `rgba` alive until upload_wait / sync."""
    ctx.upload_mosaic(Mosaic.make(tiles_x, tiles_y, order, bottom_up), rgba, 0)


Y4M_SITE_MODES = {"centre": 0, "left": 1, "auto": 2}


def y4m_input_siting(chroma_tag: str, mode: str = "auto") -> str:
    """How the command line's --in-chroma-site MODE ("centre", "left", "auto") reads a Y4M file tagged C<chroma_tag> (csrc/host/y4m.h,
    y4mInputSiting): "centre" or "left".  auto: 420mpeg2 is left-sited; 420jpeg, 420paldv and plain 420 are read centre-sited."""
    rc = load_host_library().lfi_host_y4m_input_siting(str(chroma_tag).encode(), Y4M_SITE_MODES[mode])
    if rc < 0:
        raise ValueError("unknown siting mode")
    return ("centre", "left")[rc]


def read_y4m_info(path: str, deep: bool = False) -> dict:
    """The header of a Y4M file and its number of frames (csrc/host/y4m.h, Y4mReader): width, height, fps (numerator, denominator; (0, 0)
    without an F token), frames, chroma (the C tag without its C), centre_sited, full_range (True, False, or None without XCOLORRANGE).
    Raises ValueError for what the reader refuses.  deep: C420p10 files are accepted too and the result has `depth` (8 or 10)."""
    lib = load_host_library()
    out = np.zeros(8, dtype=np.int32)
    tag = C.create_string_buffer(32)
    err = C.create_string_buffer(512)
    if deep:
        if lib.lfi_host_y4m_info_deep(str(path).encode(), out.ctypes.data_as(C.c_void_p), tag, len(tag), err, len(err)) != 0:
            raise ValueError(err.value.decode())
        return dict(width=int(out[0]), height=int(out[1]), fps=(int(out[2]), int(out[3])), frames=int(out[4]),
                    full_range=None if out[5] < 0 else bool(out[5]), centre_sited=bool(out[6]), chroma=tag.value.decode(), depth=int(out[7]))
    if lib.lfi_host_y4m_info(str(path).encode(), out.ctypes.data_as(C.c_void_p), tag, len(tag), err, len(err)) != 0:
        raise ValueError(err.value.decode())
    return dict(width=int(out[0]), height=int(out[1]), fps=(int(out[2]), int(out[3])), frames=int(out[4]),
                full_range=None if out[5] < 0 else bool(out[5]), centre_sited=bool(out[6]), chroma=tag.value.decode())


def read_y4m(path: str, first: int = 0, n: int | None = None, deep: bool = False) -> np.ndarray:
    """Frames [first, first + n) (default: all from `first`) of a Y4M file as [n][frame_bytes] uint8 — what Context.upload_images_yuv420 takes.
    deep: C420p10 files are accepted too; their frames are I010 bytes, twice as many."""
    lib = load_host_library()
    info = read_y4m_info(path, deep)
    n = info["frames"] - first if n is None else n
    fb = lib.lfi_host_y4m_frame_bytes_deep(info["width"], info["height"], info.get("depth", 8))
    out = np.empty((max(n, 0), fb), dtype=np.uint8)
    err = C.create_string_buffer(512)
    if (lib.lfi_host_y4m_read_deep if deep else lib.lfi_host_y4m_read)(str(path).encode(), first, n, out.ctypes.data_as(C.c_void_p), fb, err, len(err)) != 0:
        raise ValueError(err.value.decode())
    return out


def load_grid_y4m(path: str, t: int = 0):
    """LfLoader on a directory of <row>_<col>.y4m files (a light-field video): returns (cols, rows, width, height, frames, full_range,
    [N][frame_bytes] u8 — frame t of every camera, g = col*rows + row).  Raises RuntimeError for what the loader refuses."""
    lib = load_host_library()
    out = np.zeros(6, dtype=np.int32)
    _err_call(lib.lfi_host_load_grid_y4m, str(path).encode(), t, out.ctypes.data_as(C.c_void_p), None, 0)
    cols, rows, w, h, frames, rng = (int(v) for v in out)
    fb = lib.lfi_host_y4m_frame_bytes(w, h)
    data = np.empty((cols * rows, fb), dtype=np.uint8)
    _err_call(lib.lfi_host_load_grid_y4m, str(path).encode(), t, out.ctypes.data_as(C.c_void_p), data.ctypes.data_as(C.c_void_p), fb)
    return cols, rows, w, h, frames, None if rng < 0 else bool(rng), data


def build_view_offsets(cols: int, rows: int, width: int, height: int, trajectory: str, aspect: float, focus_v) -> np.ndarray:
    """[V][N][2] int32 rows for Context.set_view_offsets: row v = the focused offsets of the trajectory's centre at focus_v[v]
    (Parameterizer::offsets)."""
    f = np.ascontiguousarray(np.atleast_1d(focus_v), dtype=np.float32)
    out = np.zeros((len(f), cols * rows, 2), dtype=np.int32)
    _err_call(load_host_library().lfi_host_build_view_offsets, cols, rows, width, height, trajectory.encode(), aspect, f.ctypes.data,
              len(f), out.ctypes.data)
    return out


def build_view_centred_offsets(cols: int, rows: int, width: int, height: int, trajectory: str, aspect: float, focus_v):
    """Each view shifted about its own camera: (O [V][N][2] float32 for Context.set_view_float_offsets, D [V][N][2] int32 for
    Context.set_view_offsets) — row v = Parameterizer::offsets at focus_v[v] for the trajectory collapsed onto camera v of V."""
    f = np.ascontiguousarray(np.atleast_1d(focus_v), dtype=np.float32)
    o = np.zeros((len(f), cols * rows, 2), dtype=np.float32)
    d = np.zeros((len(f), cols * rows, 2), dtype=np.int32)
    _err_call(load_host_library().lfi_host_build_view_centred_offsets, cols, rows, width, height, trajectory.encode(), aspect, f.ctypes.data,
              len(f), o.ctypes.data, d.ctypes.data)
    return o, d


def build_view_focus_ids(cols: int, rows: int, trajectory: str, views: int) -> np.ndarray:
    """Each view's focus-map images, [V][min(32, N)] int32 for Context.view_focus_maps — row v = the focus_map_ids build_params selects
    for the trajectory collapsed onto camera v of V."""
    out = np.zeros(max(views, 1) * 32, dtype=np.int32)
    n = C.c_int32(0)
    _err_call(load_host_library().lfi_host_build_view_focus_ids, cols, rows, trajectory.encode(), views, out.ctypes.data, C.byref(n))
    return out[:views * n.value].reshape(views, n.value).copy()


def _err_call(fn, *args):
    err = C.create_string_buffer(512)
    rc = fn(*args, err, len(err))
    if rc != 0:
        raise RuntimeError(err.value.decode())


def load_image(path: str) -> np.ndarray:
    """csrc/host/image_io.cpp: PNG / PPM → [H][W][4] u8."""
    lib = load_host_library()
    w, h = C.c_int(), C.c_int()
    _err_call(lib.lfi_host_load_image, path.encode(), C.byref(w), C.byref(h), None)
    out = np.empty((h.value, w.value, 4), dtype=np.uint8)
    _err_call(lib.lfi_host_load_image, path.encode(), C.byref(w), C.byref(h), out.ctypes.data_as(C.c_void_p))
    return out


def write_png(path: str, image: np.ndarray) -> None:
    image = np.ascontiguousarray(image, dtype=np.uint8)
    h, w, c = image.shape
    _err_call(load_host_library().lfi_host_write_png, path.encode(), w, h, c, image.ctypes.data_as(C.c_void_p))


def load_grid(path: str):
    """LfLoader::loadData: returns (cols, rows, [N][H][W][4] u8 with g = col*rows + row)."""
    lib = load_host_library()
    cols, rows, w, h = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _err_call(lib.lfi_host_load_grid, path.encode(), C.byref(cols), C.byref(rows), C.byref(w), C.byref(h), None)
    out = np.empty((cols.value * rows.value, h.value, w.value, 4), dtype=np.uint8)
    _err_call(lib.lfi_host_load_grid, path.encode(), C.byref(cols), C.byref(rows), C.byref(w), C.byref(h),
              out.ctypes.data_as(C.c_void_p))
    return cols.value, rows.value, out
