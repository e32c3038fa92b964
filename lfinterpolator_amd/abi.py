"""ctypes binding of include/lfi.h (lib/liblfi_hip.so).  Thin: every method is one C-ABI call."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

from .build import HIP_LIB

LFI_METHOD_STD = 0
LFI_METHOD_TEN_WM = 1
LFI_FLAG_UNIFIED_FOCUS_MAP = 1
LFI_FLAG_TEN_ROUND_PER_BATCH = 2
LFI_FLAG_SINGLE_SWEEP_DIRECTION = 4
LFI_FLAG_STD_ANALYTIC_BAND = 8
LFI_FLAG_STD_MEASURED_BAND = 16
LFI_FLAG_STD_BAND_PROBE_FAIL = 32
LFI_FLAG_DEEP_VIEWS = 64     # fixed-focus renders also keep 10 bits per channel from the accumulator: the deep planes (include/lfi.h)
LFI_FLAG_IN_FRAME = 128      # fixed-focus renders leave out the samples outside their image and renormalise the weights (include/lfi.h)
LFI_FLAG_LINEAR_LIGHT = 256  # fixed-focus renders decode sRGB to linear light before the sum and encode the sum (include/lfi.h)
LFI_KERNEL_FOCUS_ESTIMATE = 2
LFI_POISON_VIEWS = 1
LFI_POISON_SCRATCH = 2
LFI_POISON_MAPS = 4
LFI_POISON_FOCUS_WORKSPACE = 8
LFI_POISON_DERIVED = 16
LFI_POISON_VIEW_MAPS = 32
LFI_POISON_DEEP = 64
LFI_LENT_INVERT = 1
LFI_LENT_BGR = 4         # lfi_lenticular.flags: the panel's subpixels run B, G, R
LFI_LENT_BILINEAR = 8    # … bilinear tile sampling
LFI_LENT_BLEND = 16      # … every subpixel blends the two views nearest to its phase
LFI_RGBD_INVERT = 1
LFI_RGBD_VIEW_MAPS = 2
LFI_YUV_BT709 = 0
LFI_YUV_BT601 = 1
LFI_YUV_LIMITED = 0
LFI_YUV_FULL = 1
YUV_MATRICES = {"709": LFI_YUV_BT709, "601": LFI_YUV_BT601}
YUV_RANGES = {"limited": LFI_YUV_LIMITED, "full": LFI_YUV_FULL}
LFI_CHROMA_BILINEAR = 0
LFI_CHROMA_NEAREST = 1
YUV_CHROMAS = {"bilinear": LFI_CHROMA_BILINEAR, "nearest": LFI_CHROMA_NEAREST}
LFI_YUV_SITING_CENTRE = 0
LFI_YUV_SITING_LEFT = 1
YUV_SITINGS = {"centre": LFI_YUV_SITING_CENTRE, "left": LFI_YUV_SITING_LEFT}
LFI_YUV_I420 = 0
LFI_YUV_NV12 = 1
LFI_YUV_10BIT = 0x100      # the depth flag of a surface format: two bytes per sample (include/lfi.h)
LFI_YUV_I010 = LFI_YUV_I420 | LFI_YUV_10BIT   # planar, code in bits 9..0 of a little-endian u16 (yuv420p10le)
LFI_YUV_P010 = LFI_YUV_NV12 | LFI_YUV_10BIT   # semi-planar, code in bits 15..6 (p010le)
LFI_YUV_DEEP = 0x200       # a source flag on a 10-bit format, for lfi_download_views_yuv only: the frames are made from the deep views
LFI_YUV_GBRP10 = 4 | LFI_YUV_10BIT | LFI_YUV_DEEP   # no conversion: full-size planes G, B, R of 10-bit codes (ffmpeg's gbrp10le)
YUV_FORMATS = {"i420": LFI_YUV_I420, "nv12": LFI_YUV_NV12, "i010": LFI_YUV_I010, "p010": LFI_YUV_P010, "i010_deep": LFI_YUV_I010 | LFI_YUV_DEEP,
               "p010_deep": LFI_YUV_P010 | LFI_YUV_DEEP, "gbrp10": LFI_YUV_GBRP10}
LFI_MEM_HOST = 0
LFI_MEM_DEVICE = 1
YUV_MEMORIES = {"host": LFI_MEM_HOST, "device": LFI_MEM_DEVICE}
LFI_MOSAIC_ROWS = 0
LFI_MOSAIC_GRID = 1
LFI_MOSAIC_BOTTOM_UP = 1
MOSAIC_ORDERS = {"rows": LFI_MOSAIC_ROWS, "grid": LFI_MOSAIC_GRID}
METHODS = {"STD": LFI_METHOD_STD, "TEN_WM": LFI_METHOD_TEN_WM, "FOCUS": LFI_KERNEL_FOCUS_ESTIMATE}

# every symbol include/lfi.h declares
ABI_SYMBOLS = [
    "lfi_create", "lfi_destroy", "lfi_last_error", "lfi_abi_version", "lfi_device_count", "lfi_set_grid", "lfi_set_row_window",
    "lfi_upload_image", "lfi_attach_grid", "lfi_broadcast_grid", "lfi_grid_device_ptr", "lfi_fill_synthetic", "lfi_set_params",
    "lfi_attach_views", "lfi_views_device_ptr", "lfi_focus_map", "lfi_render", "lfi_benchmark", "lfi_timer_start",
    "lfi_timer_stop", "lfi_sync", "lfi_download_view", "lfi_download_map", "lfi_download_quilt", "lfi_download_quilt_tiles", "lfi_release_inputs", "lfi_alloc_pinned", "lfi_free_pinned", "lfi_upload_map", "lfi_set_stream",
    "lfi_set_variant", "lfi_list_variants", "lfi_download_coords", "lfi_download_prequant", "lfi_debug_mfma_f16",
    "lfi_grid_modified", "lfi_prepare", "lfi_memory_info", "lfi_last_kernel_name", "lfi_fill_synthetic_images", "lfi_set_output_layout", "lfi_view_layout", "lfi_fill_synthetic_scene", "lfi_upload_image_async", "lfi_upload_wait", "lfi_render_stream", "lfi_compare_view", "lfi_debug_mfma_f16_chain", "lfi_debug_pk_minmax3_f16", "lfi_std_band_info",
    "lfi_debug_poison", "lfi_set_view_offsets", "lfi_set_view_float_offsets", "lfi_view_focus_maps", "lfi_download_view_map",
    "lfi_upload_view_map", "lfi_focus_curve", "lfi_focus_tiles", "lfi_focus_tiles_steps", "lfi_focus_tiles_passes", "lfi_focus_route_info", "lfi_download_quilt_scaled", "lfi_download_quilt_tiles_scaled",
    "lfi_keep_views", "lfi_compare_views", "lfi_set_focus_steps", "lfi_focus_steps", "lfi_download_native",
    "lfi_download_views_yuv420", "lfi_render_stream_yuv420", "lfi_upload_images_yuv420",
    "lfi_yuv_surfaces_check", "lfi_yuv_surfaces_packed", "lfi_upload_images_yuv", "lfi_download_views_yuv",
    "lfi_download_quilt_yuv", "lfi_download_rgbd_yuv", "lfi_set_yuv_siting", "lfi_yuv_siting",
    "lfi_upload_images_yuv_derived", "lfi_debug_derived_layout", "lfi_debug_download_derived",
    "lfi_mosaic_map", "lfi_upload_mosaic_yuv", "lfi_upload_mosaic", "lfi_debug_mosaic_chunk",
    "lfi_upload_mosaic_yuv_derived", "lfi_debug_set_mosaic_chunk_cap", "lfi_debug_streams",
]


class LfiError(RuntimeError):
    pass


class _Params(C.Structure):
    _fields_ = [("views", C.c_int32), ("focused_offsets", C.c_void_p), ("offsets", C.c_void_p),
                ("weights_fp16", C.c_void_p), ("focus_map_ids", C.c_void_p), ("n_focus_ids", C.c_int32),
                ("focus", C.c_float), ("range", C.c_float), ("block_radius", C.c_int32 * 2), ("flags", C.c_uint32)]


class BenchStats(C.Structure):
    _fields_ = [("runs", C.c_int32), ("mean_ms", C.c_float), ("median_ms", C.c_float), ("min_ms", C.c_float),
                ("max_ms", C.c_float), ("back_to_back_ms", C.c_float)]


LFI_LAYOUT_RGBA = 0
LFI_LAYOUT_PLANAR_RGB = 1
LAYOUTS = {"rgba": LFI_LAYOUT_RGBA, "planar": LFI_LAYOUT_PLANAR_RGB}


class ViewLayout(C.Structure):
    _fields_ = [("layout", C.c_int32), ("rows", C.c_int32), ("row_pitch_bytes", C.c_size_t), ("plane_stride_bytes", C.c_size_t),
                ("view_stride_bytes", C.c_size_t)]


class Quality(C.Structure):
    _fields_ = [("mse", C.c_double * 3), ("psnr", C.c_double * 3), ("psnr_all", C.c_double), ("ssim", C.c_double * 3), ("ssim_all", C.c_double)]


class ViewQuality(C.Structure):
    """lfi_view_quality: one view of lfi_compare_views"""
    _fields_ = [("q", Quality), ("sq_err", C.c_uint64 * 3), ("differing_bytes", C.c_uint64), ("windows", C.c_uint64), ("max_abs_diff", C.c_int32)]


class StdBandInfo(C.Structure):
    _fields_ = [("probed", C.c_int32), ("within_budget", C.c_int32), ("analytic_forced", C.c_int32), ("sums", C.c_int32),
                ("worst_fraction", C.c_float), ("probe_ms", C.c_float), ("message", C.c_char * 160)]


class FocusCurveResult(C.Structure):
    _fields_ = [("best_index", C.c_int32), ("best_focus", C.c_float), ("pixels", C.c_uint64)]


LFI_FOCUS_ROUTE_PASSES = 8


class FocusRoute(C.Structure):
    """lfi_focus_route: the route of the context's last estimate call (include/lfi.h).  Context.focus_route returns it as a dict."""
    _fields_ = [("calls", C.c_int32), ("jobs", C.c_int32), ("estimate", C.c_char_p), ("declined", C.c_char_p), ("passes", C.c_int32),
                ("range_striped", C.c_int32), ("range_kernel", C.c_char_p), ("consumer", C.c_char_p), ("consumer_striped", C.c_int32),
                ("planes_padded", C.c_int32), ("planes_kept", C.c_int32), ("pad_shift", C.c_int32 * 2), ("We_p", C.c_int32), ("He_p", C.c_int32),
                ("Wp", C.c_int32), ("Hp", C.c_int32), ("R_cap", C.c_int32), ("C_cap", C.c_int32), ("range_cpw", C.c_int32 * LFI_FOCUS_ROUTE_PASSES),
                ("row_entries", C.c_uint32 * LFI_FOCUS_ROUTE_PASSES), ("col_entries", C.c_uint32 * LFI_FOCUS_ROUTE_PASSES)]


class Lenticular(C.Structure):
    """lfi_lenticular: the lens sheet of lfi_download_native in units of 2^-32 lens periods (host.lenticular builds one from a calibration,
    host.lenticular_file from a display's calibration file); flags: LFI_LENT_INVERT | LFI_LENT_BGR | LFI_LENT_BILINEAR | LFI_LENT_BLEND"""
    _fields_ = [("x_step", C.c_uint32), ("y_step", C.c_uint32), ("phase0", C.c_uint32), ("views", C.c_int32), ("flags", C.c_uint32)]


class YuvSurfaces(C.Structure):
    """lfi_yuv_surfaces: a batch of YUV 4:2:0 frames — format, memory space, pitches and plane offsets (include/lfi.h).  `keep` holds whatever
    owns the memory (a numpy array, a tensor) alive as long as the descriptor."""
    _fields_ = [("format", C.c_int32), ("memory", C.c_int32), ("base", C.c_void_p), ("frame_stride", C.c_size_t), ("y_pitch", C.c_size_t),
                ("c_offset", C.c_size_t), ("c_pitch", C.c_size_t), ("cr_offset", C.c_size_t)]
    keep = None

    @classmethod
    def make(cls, fmt, memory, base: int, frame_stride: int, y_pitch: int, c_offset: int, c_pitch: int, cr_offset: int = 0, keep=None) -> "YuvSurfaces":
        """from a raw pointer (a device one: e.g. a torch tensor's data_ptr()) plus layout; fmt: "i420" / "nv12", memory: "host" / "device"
        (or the LFI_* values)"""
        s = cls(YUV_FORMATS.get(fmt, fmt), YUV_MEMORIES.get(memory, memory), base, frame_stride, y_pitch, c_offset, c_pitch, cr_offset)
        s.keep = keep
        return s

    @classmethod
    def from_array(cls, fmt, frames: np.ndarray, y_pitch: int, c_offset: int, c_pitch: int, cr_offset: int = 0) -> "YuvSurfaces":
        """host surfaces in a numpy array [n][P] uint8: frame k is row k, the frame stride is the array's"""
        assert frames.dtype == np.uint8 and frames.ndim == 2 and frames.size and frames.strides[1] == 1
        return cls.make(fmt, LFI_MEM_HOST, frames.ctypes.data, frames.strides[0], y_pitch, c_offset, c_pitch, cr_offset, keep=frames)

    @classmethod
    def gbrp10_from_array(cls, frames: np.ndarray) -> "YuvSurfaces":
        """host LFI_YUV_GBRP10 surfaces over a numpy array [n][3: G,B,R][H][W] uint16 (C-contiguous): the tight frame of ffmpeg's gbrp10le"""
        assert frames.dtype == np.uint16 and frames.ndim == 4 and frames.shape[1] == 3 and frames.size and frames.flags.c_contiguous
        n, _, h, w = frames.shape
        return cls.make(LFI_YUV_GBRP10, LFI_MEM_HOST, frames.ctypes.data, 6 * w * h, 2 * w, 2 * w * h, 2 * w, 4 * w * h, keep=frames)

    @staticmethod
    def gbrp10_to_rgb(frames: np.ndarray) -> np.ndarray:
        """[n][3: G,B,R][H][W] uint16 -> [n][H][W][3: R,G,B] uint16"""
        return np.ascontiguousarray(frames[:, [2, 0, 1]].transpose(0, 2, 3, 1))

    def check(self, width: int, height: int, n: int) -> bool:
        """lfi_yuv_surfaces_check: does this describe n frames of width x height?"""
        return load_hip_library().lfi_yuv_surfaces_check(C.byref(self), width, height, n) == 0


def yuv_surfaces_packed(fmt, memory, base: int | None, width: int, height: int, keep=None) -> YuvSurfaces:
    """lfi_yuv_surfaces_packed: the tight layout of width x height frames at `base` (None: to be set later)"""
    s = YuvSurfaces()
    if load_hip_library().lfi_yuv_surfaces_packed(YUV_FORMATS.get(fmt, fmt), YUV_MEMORIES.get(memory, memory), base, width, height, C.byref(s)) != 0:
        raise LfiError("lfi_yuv_surfaces_packed: unknown format or memory, or a size below 1")
    s.keep = keep
    return s


class Mosaic(C.Structure):
    """lfi_mosaic: one frame of tiles_x·W × tiles_y·H that holds the grid's images as tiles — tiles [first_tile, first_tile + n) in ROWS order,
    mapped onto images by `order` (LFI_MOSAIC_ROWS: image g0 + k; LFI_MOSAIC_GRID: tile (tx, ty) is camera column tx, row ty) with
    LFI_MOSAIC_BOTTOM_UP in `flags` where the tile rows count from the frame's bottom (include/lfi.h)."""
    _fields_ = [("tiles_x", C.c_int32), ("tiles_y", C.c_int32), ("first_tile", C.c_int32), ("n", C.c_int32), ("order", C.c_int32), ("flags", C.c_uint32)]

    @classmethod
    def make(cls, tiles_x: int, tiles_y: int, order="rows", bottom_up: bool = False, first_tile: int = 0, n: int | None = None) -> "Mosaic":
        """order: "rows" / "grid" (or the LFI_MOSAIC_* values); n defaults to all tiles from first_tile"""
        return cls(tiles_x, tiles_y, first_tile, tiles_x * tiles_y - first_tile if n is None else n, MOSAIC_ORDERS.get(order, order),
                   LFI_MOSAIC_BOTTOM_UP if bottom_up else 0)


def mosaic_map(mosaic: Mosaic, cols: int, rows: int, g0: int = 0) -> np.ndarray:
    """lfi_mosaic_map for every tile of the mosaic: [n][3] int32, row k = (tx, ty, g) — the tile's column and row in the frame and the image
    it becomes in a cols × rows grid.  LfiError for what the call refuses."""
    lib = load_hip_library()
    out = np.zeros((max(mosaic.n, 0), 3), np.int32)
    if lib.lfi_mosaic_map(C.byref(mosaic), cols, rows, g0, 0, None, None, None) != 0:
        raise LfiError("lfi_mosaic_map: the mosaic does not map onto the grid (include/lfi.h)")
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    for k in np.arange(mosaic.n):
        if lib.lfi_mosaic_map(C.byref(mosaic), cols, rows, g0, int(k), C.byref(a), C.byref(b), C.byref(c)) != 0:
            raise LfiError("lfi_mosaic_map refused a tile of a mosaic it accepted")
        out[k] = a.value, b.value, c.value
    return out


LFI_YUV_DERIVED_SPAN = 384   # bytes (= pixels) of a plane row that a workgroup of lfi_upload_images_yuv_derived's kernel owns (include/lfi.h)


class DerivedLayout(C.Structure):
    """lfi_derived_layout: the derived planar copy of the inputs is [n][3][rows][pitch_bytes] bytes; byte j of a plane row of image g holds
    pixel clamp(j - padx - phase[g], 0, W - 1).  `phases` ([n] int32) is filled in by Context.derived_layout."""
    _fields_ = [("pitch_bytes", C.c_size_t), ("rows", C.c_int32), ("padx", C.c_int32), ("reach", C.c_int32), ("n", C.c_int32)]
    phases = None

    def __eq__(self, other):
        return (isinstance(other, DerivedLayout) and all(getattr(self, f) == getattr(other, f) for f, _ in self._fields_)
                and np.array_equal(self.phases, other.phases))

    __hash__ = None


class MemoryInfo(C.Structure):
    _fields_ = [("grid_bytes", C.c_size_t), ("derived_bytes", C.c_size_t), ("views_bytes", C.c_size_t), ("maps_bytes", C.c_size_t),
                ("workspace_bytes", C.c_size_t), ("derived_build_ms", C.c_float)]


_lib = None


def load_hip_library() -> C.CDLL:
    """Load lib/liblfi_hip.so; a missing library is an error, never a fallback."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm bundles its own HIP runtime under the same soname (libamdhip64.so.7) as /opt/rocm's, and the first one a
    # process loads wins.  If ours pulled in /opt/rocm's first, a later `import torch` would find "No HIP GPUs"; so when torch is
    # installed it goes first (bench.py and the distributed path need it anyway).  The C++ host code is unaffected.
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(HIP_LIB):
        raise LfiError(f"{HIP_LIB} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950); lfinterpolator_amd has no CPU fallback")
    lib = C.CDLL(HIP_LIB)
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    sig = {
        "lfi_create": (i, [i, C.POINTER(vp)]),
        "lfi_destroy": (i, [vp]),
        "lfi_last_error": (C.c_char_p, [vp]),
        "lfi_abi_version": (i, []),
        "lfi_device_count": (i, []),
        "lfi_set_grid": (i, [vp, i, i, i, i]),
        "lfi_set_row_window": (i, [vp, i, i, i, i]),
        "lfi_upload_image": (i, [vp, i, vp, sz]),
        "lfi_attach_grid": (i, [vp, vp, sz]),
        "lfi_broadcast_grid": (i, [C.POINTER(vp), i, i]),
        "lfi_grid_device_ptr": (i, [vp, C.POINTER(vp), C.POINTER(sz)]),
        "lfi_fill_synthetic": (i, [vp, C.c_uint32]),
        "lfi_set_params": (i, [vp, C.POINTER(_Params)]),
        "lfi_set_view_offsets": (i, [vp, vp, i]),
        "lfi_set_view_float_offsets": (i, [vp, vp, i]),
        "lfi_view_focus_maps": (i, [vp, vp, i, i]),
        "lfi_download_view_map": (i, [vp, i, i, vp, sz]),
        "lfi_upload_view_map": (i, [vp, i, i, vp, sz]),
        "lfi_attach_views": (i, [vp, vp, sz]),
        "lfi_views_device_ptr": (i, [vp, C.POINTER(vp), C.POINTER(sz)]),
        "lfi_focus_map": (i, [vp]),
        "lfi_set_focus_steps": (i, [vp, i]),
        "lfi_focus_steps": (i, [vp, C.POINTER(i)]),
        "lfi_focus_curve": (i, [vp, i, i, i, i, i, vp, C.POINTER(FocusCurveResult)]),
        "lfi_focus_tiles": (i, [vp, i, i, vp, C.POINTER(FocusCurveResult)]),
        "lfi_focus_tiles_steps": (i, [vp, i, i, i, vp, C.POINTER(FocusCurveResult)]),
        "lfi_focus_tiles_passes": (i, [vp]),
        "lfi_focus_route_info": (i, [vp, C.POINTER(FocusRoute)]),
        "lfi_render": (i, [vp, i, i, i, i]),
        "lfi_benchmark": (i, [vp, i, i, i, i, i, i, C.POINTER(BenchStats)]),
        "lfi_timer_start": (i, [vp]),
        "lfi_timer_stop": (i, [vp, C.POINTER(C.c_float)]),
        "lfi_sync": (i, [vp]),
        "lfi_download_view": (i, [vp, i, vp, sz]),
        "lfi_download_map": (i, [vp, i, vp, sz]),
        "lfi_release_inputs": (i, [vp]),
        "lfi_download_quilt": (i, [vp, i, i, i, vp, sz]),
        "lfi_download_quilt_tiles": (i, [vp, i, i, i, i, i, vp, sz]),
        "lfi_download_quilt_scaled": (i, [vp, i, i, i, i, i, vp, sz]),
        "lfi_download_quilt_tiles_scaled": (i, [vp, i, i, i, i, i, i, i, vp, sz]),
        "lfi_download_native": (i, [vp, C.POINTER(Lenticular), i, i, i, i, i, vp, sz]),
        "lfi_download_views_yuv420": (i, [vp, i, i, i, i, vp, sz]),
        "lfi_render_stream_yuv420": (i, [vp, i, i, vp, i, i, i, vp, sz]),
        "lfi_upload_images_yuv420": (i, [vp, i, i, i, i, i, vp, sz]),
        "lfi_yuv_surfaces_check": (i, [C.POINTER(YuvSurfaces), i, i, i]),
        "lfi_yuv_surfaces_packed": (i, [i, i, vp, i, i, C.POINTER(YuvSurfaces)]),
        "lfi_upload_images_yuv": (i, [vp, i, i, i, i, i, C.POINTER(YuvSurfaces)]),
        "lfi_download_views_yuv": (i, [vp, i, i, i, i, C.POINTER(YuvSurfaces)]),
        "lfi_download_quilt_yuv": (i, [vp, i, i, i, i, i, i, i, C.POINTER(YuvSurfaces)]),
        "lfi_download_rgbd_yuv": (i, [vp, i, i, i, C.c_uint32, i, i, i, i, C.POINTER(YuvSurfaces)]),
        "lfi_upload_images_yuv_derived": (i, [vp, i, i, i, i, i, C.POINTER(YuvSurfaces)]),
        "lfi_set_yuv_siting": (i, [vp, i, i]),
        "lfi_yuv_siting": (i, [vp, C.POINTER(i), C.POINTER(i)]),
        "lfi_debug_derived_layout": (i, [vp, C.POINTER(DerivedLayout), vp]),
        "lfi_mosaic_map": (i, [C.POINTER(Mosaic), i, i, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(i)]),
        "lfi_upload_mosaic_yuv": (i, [vp, C.POINTER(Mosaic), i, i, i, i, C.POINTER(YuvSurfaces)]),
        "lfi_upload_mosaic_yuv_derived": (i, [vp, C.POINTER(Mosaic), i, i, i, i, C.POINTER(YuvSurfaces)]),
        "lfi_debug_set_mosaic_chunk_cap": (i, [vp, sz]),
        "lfi_upload_mosaic": (i, [vp, C.POINTER(Mosaic), i, vp, sz]),
        "lfi_debug_mosaic_chunk": (i, [C.POINTER(Mosaic), i, i, sz, i, vp]),
        "lfi_debug_download_derived": (i, [vp, i, i, vp]),
        "lfi_debug_streams": (i, [vp, C.POINTER(vp)]),
        "lfi_alloc_pinned": (i, [sz, C.POINTER(vp)]),
        "lfi_free_pinned": (i, [vp]),
        "lfi_grid_modified": (i, [vp]),
        "lfi_upload_map": (i, [vp, i, vp, sz]),
        "lfi_set_stream": (i, [vp, vp]),
        "lfi_set_variant": (i, [vp, i, C.c_char_p]),
        "lfi_list_variants": (C.c_char_p, [i]),
        "lfi_download_coords": (i, [vp, i, i, i, vp]),
        "lfi_download_prequant": (i, [vp, i, i, i, vp]),
        "lfi_debug_mfma_f16": (i, [vp, vp, vp, vp]),
        "lfi_prepare": (i, [vp, i, i, i, i]),
        "lfi_render_stream": (i, [vp, i, i, vp, i, vp, sz]),
        "lfi_compare_view": (i, [vp, i, vp, sz, C.POINTER(Quality)]),
        "lfi_keep_views": (i, [vp, i, i]),
        "lfi_compare_views": (i, [vp, i, i, vp, sz, sz, C.POINTER(ViewQuality), C.POINTER(Quality)]),
        "lfi_upload_image_async": (i, [vp, i, vp, sz]),
        "lfi_upload_wait": (i, [vp]),
        "lfi_fill_synthetic_scene": (i, [vp, C.c_uint32]),
        "lfi_debug_mfma_f16_chain": (i, [vp, i, i, vp, vp, vp]),
        "lfi_debug_pk_minmax3_f16": (i, [vp, vp]),
        "lfi_debug_poison": (i, [vp, C.c_uint32, C.c_uint8]),
        "lfi_set_output_layout": (i, [vp, i]),
        "lfi_view_layout": (i, [vp, C.POINTER(ViewLayout)]),
        "lfi_fill_synthetic_images": (i, [vp, C.c_uint32, i, i]),
        "lfi_memory_info": (i, [vp, C.POINTER(MemoryInfo)]),
        "lfi_std_band_info": (i, [vp, C.POINTER(StdBandInfo)]),
        "lfi_last_kernel_name": (C.c_char_p, [vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)  # AttributeError here = the library does not export what lfi.h declares
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def broadcast_grid(contexts, root: int = 0) -> None:
    """lfi_broadcast_grid over a list of Context objects (single process, one context per GPU, RCCL)."""
    lib = load_hip_library()
    arr = (C.c_void_p * len(contexts))(*[c._h for c in contexts])
    rc = lib.lfi_broadcast_grid(arr, len(contexts), root)
    if rc != 0:
        raise LfiError(f"lfi_broadcast_grid failed ({rc}): {lib.lfi_last_error(contexts[root]._h).decode()}")


class Context:
    """One GPU context (lfi_ctx).  Mirrors the device-facing half of the reference's Interpolator."""

    def __init__(self, device: int = 0):
        self._lib = load_hip_library()
        handle = C.c_void_p()
        rc = self._lib.lfi_create(device, C.byref(handle))
        if rc != 0:
            raise LfiError(f"lfi_create failed ({rc}): {self._lib.lfi_last_error(None).decode()}")
        self._h = handle
        self.device = device
        self.cols = self.rows = self.width = self.height = self.views = 0
        self._keep = None
        self._pinned = []

    # -- helpers --------------------------------------------------------------------------------------------
    def _check(self, rc: int) -> None:
        if rc != 0:
            raise LfiError(f"lfi error {rc}: {self._lib.lfi_last_error(self._h).decode()}")

    def close(self) -> None:
        if getattr(self, "_h", None):
            for p in self._pinned: # arrays from pinned_empty must not be used after this
                self._lib.lfi_free_pinned(C.c_void_p(p))
            self._pinned = []
            self._lib.lfi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def n_images(self) -> int:
        return self.cols * self.rows

    # -- grid -------------------------------------------------------------------------------------------------
    def set_grid(self, cols: int, rows: int, width: int, height: int) -> None:
        self._check(self._lib.lfi_set_grid(self._h, cols, rows, width, height))
        self.cols, self.rows, self.width, self.height = cols, rows, width, height
        self.out_rows = (0, height)

    def set_row_window(self, out_y0: int, out_y1: int, in_y0: int, in_y1: int) -> None:
        """Render rows [out_y0, out_y1) only, holding input rows [in_y0, in_y1) only (row-band sharding)."""
        self._check(self._lib.lfi_set_row_window(self._h, out_y0, out_y1, in_y0, in_y1))
        self.out_rows = (out_y0, out_y1)

    def upload_image(self, g: int, rgba: np.ndarray) -> None:
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        assert rgba.shape == (self.height, self.width, 4)
        self._check(self._lib.lfi_upload_image(self._h, g, _ptr(rgba), self.width * 4))

    def upload_grid(self, lf: np.ndarray, asynchronous: bool = False) -> None:
        """lf: [N][H][W][4] u8 with g = col*rows + row."""
        assert lf.shape == (self.n_images, self.height, self.width, 4)
        for g in range(self.n_images):
            if asynchronous:
                self.upload_image_async(g, lf[g])
            else:
                self.upload_image(g, lf[g])

    def upload_image_async(self, g: int, rgba: np.ndarray) -> None:
        """Enqueue the copy on the context's copy stream; `rgba` may be pageable (staged, free on return) or from pinned_empty
        (DMA'd in place: keep it alive until upload_wait / sync)."""
        assert rgba.shape == (self.height, self.width, 4) and rgba.dtype == np.uint8 and rgba.flags.c_contiguous
        self._check(self._lib.lfi_upload_image_async(self._h, g, _ptr(rgba), self.width * 4))

    def upload_wait(self) -> None:
        self._check(self._lib.lfi_upload_wait(self._h))

    def upload_images_yuv420(self, frames: np.ndarray, g0: int = 0, matrix="709", range="limited", chroma="bilinear") -> None:
        """Images [g0, g0 + n) from n 8-bit YUV 4:2:0 frames (I420: Y, Cb, Cr planes, tightly packed), expanded to RGBA on the device
        (lfi_upload_images_yuv420).  frames: [n][P] uint8 with rows of P ≥ frame bytes — the frame stride is the array's; pageable (staged,
        free on return) or from pinned_empty (keep it alive until upload_wait / sync).  matrix: "709" / "601", range: "limited" / "full",
        chroma: "bilinear" / "nearest" (or the LFI_* values).  Ordered like upload_image_async."""
        assert frames.dtype == np.uint8 and frames.ndim == 2 and (frames.size == 0 or frames.strides[1] == 1)
        self._check(self._lib.lfi_upload_images_yuv420(self._h, g0, frames.shape[0], YUV_MATRICES.get(matrix, matrix), YUV_RANGES.get(range, range),
                                                       YUV_CHROMAS.get(chroma, chroma), _ptr(frames), frames.strides[0] if frames.size else 0))

    def upload_images_yuv(self, surfaces: YuvSurfaces, n: int, g0: int = 0, matrix="709", range="limited", chroma="bilinear") -> None:
        """Images [g0, g0 + n) from n frames of `surfaces` (lfi_upload_images_yuv): I420 or NV12, or 10-bit I010 or P010, pitched, host or device memory; device
        surfaces whose base, pitches, offsets and stride are multiples of 16 are read in place.  Ordered like upload_image_async: keep the
        memory alive and unchanged until upload_wait / sync."""
        self._check(self._lib.lfi_upload_images_yuv(self._h, g0, n, YUV_MATRICES.get(matrix, matrix), YUV_RANGES.get(range, range),
                                                    YUV_CHROMAS.get(chroma, chroma), C.byref(surfaces) if surfaces is not None else None))

    def upload_images_yuv_derived(self, surfaces: YuvSurfaces, n: int, g0: int = 0, matrix="709", range="limited", chroma="bilinear") -> None:
        """upload_images_yuv for a context whose inputs were released (lfi_upload_images_yuv_derived): the n frames go straight into the
        planes of images [g0, g0 + n) of the derived planar copy, padding included, in one pass.  Ordered like upload_images_yuv."""
        self._check(self._lib.lfi_upload_images_yuv_derived(self._h, g0, n, YUV_MATRICES.get(matrix, matrix), YUV_RANGES.get(range, range),
                                                            YUV_CHROMAS.get(chroma, chroma), C.byref(surfaces) if surfaces is not None else None))

    def upload_mosaic_yuv(self, mosaic: Mosaic, surfaces: YuvSurfaces, g0: int = 0, matrix="709", range="limited", chroma="bilinear") -> None:
        """The grid's images from ONE 8-bit YUV 4:2:0 frame of tiles_x·W × tiles_y·H in `surfaces` (lfi_upload_mosaic_yuv): every tile is expanded
        as a frame of its own into the image `mosaic` maps it to; a device frame whose base, pitches and offsets are multiples of 16 is read
        in place by one launch.  W and H must be even.  Ordered like upload_images_yuv: keep the memory alive and unchanged until
        upload_wait / sync."""
        self._check(self._lib.lfi_upload_mosaic_yuv(self._h, C.byref(mosaic) if mosaic is not None else None, g0, YUV_MATRICES.get(matrix, matrix),
                                                    YUV_RANGES.get(range, range), YUV_CHROMAS.get(chroma, chroma),
                                                    C.byref(surfaces) if surfaces is not None else None))

    def upload_mosaic_yuv_derived(self, mosaic: Mosaic, surfaces: YuvSurfaces, g0: int = 0, matrix="709", range="limited", chroma="bilinear") -> None:
        """upload_mosaic_yuv for a context whose inputs were released (lfi_upload_mosaic_yuv_derived): the frame's tiles go straight into the
        planes of their mapped images of the derived planar copy, padding included, in one pass.  Ordered like upload_images_yuv_derived."""
        self._check(self._lib.lfi_upload_mosaic_yuv_derived(self._h, C.byref(mosaic) if mosaic is not None else None, g0, YUV_MATRICES.get(matrix, matrix),
                                                            YUV_RANGES.get(range, range), YUV_CHROMAS.get(chroma, chroma),
                                                            C.byref(surfaces) if surfaces is not None else None))

    def set_mosaic_chunk_cap(self, cap_bytes: int = 0) -> None:
        """tests: the cap of the staging chunks of upload_mosaic_yuv and upload_mosaic_yuv_derived (lfi_debug_set_mosaic_chunk_cap); 0: the
        calls' own 256 MiB"""
        self._check(self._lib.lfi_debug_set_mosaic_chunk_cap(self._h, cap_bytes))

    def upload_mosaic(self, mosaic: Mosaic, rgba: np.ndarray, g0: int = 0) -> None:
        """The grid's images from one host RGBA image of tiles_y·H × tiles_x·W pixels (lfi_upload_mosaic): upload_image_async of every tile's
        rectangle; `rgba`: (tiles_y·H, P, 4) uint8 with rows of P ≥ tiles_x·W pixels — the row pitch is the array's.  Keep it alive until
        upload_wait / sync."""
        assert rgba.dtype == np.uint8 and rgba.ndim == 3 and rgba.shape[2] == 4 and rgba.strides[1:] == (4, 1)
        assert rgba.shape[0] == mosaic.tiles_y * self.height and rgba.shape[1] >= mosaic.tiles_x * self.width
        self._check(self._lib.lfi_upload_mosaic(self._h, C.byref(mosaic), g0, _ptr(rgba), rgba.strides[0]))

    def derived_layout(self) -> DerivedLayout:
        """the layout and per-image phases of the derived planar copy (lfi_debug_derived_layout); LfiError where the copy is not current"""
        lay = DerivedLayout()
        phases = np.zeros(256, np.int32)   # LFI_MAX_IMAGES
        self._check(self._lib.lfi_debug_derived_layout(self._h, C.byref(lay), _ptr(phases)))
        lay.phases = phases[:lay.n].copy()
        return lay

    def download_derived(self, g0: int = 0, n: int | None = None) -> np.ndarray:
        """the planes of images [g0, g0 + n) (default: all from g0) of the derived planar copy, [n][3][rows][pitch] uint8
        (lfi_debug_download_derived); in stream order behind renders and uploads"""
        lay = self.derived_layout()
        n = lay.n - g0 if n is None else n
        out = np.empty((max(n, 0), 3, lay.rows, lay.pitch_bytes), np.uint8)
        self._check(self._lib.lfi_debug_download_derived(self._h, g0, n, _ptr(out)))
        return out

    def yuv_surfaces_packed(self, fmt, memory="host", base: int | None = None, keep=None) -> YuvSurfaces:
        """the tight layout of this context's frames (lfi_yuv_surfaces_packed): frame stride yuv420_frame_bytes() for "i420" and "nv12", twice that
        for the 10-bit "i010" and "p010" (two bytes per sample)"""
        return yuv_surfaces_packed(fmt, memory, base, self.width, self.height, keep)

    def attach_grid(self, device_ptr: int, nbytes: int) -> None:
        self._check(self._lib.lfi_attach_grid(self._h, C.c_void_p(device_ptr), nbytes))

    def grid_device_ptr(self):
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._lib.lfi_grid_device_ptr(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def release_inputs(self) -> None:
        """Fixed-focus use only: the planar copy becomes the only copy of the inputs, the RGBA planes are freed."""
        self._check(self._lib.lfi_release_inputs(self._h))

    def grid_modified(self) -> None:
        """The input planes were written behind the library's back (attached buffer, raw device pointer)."""
        self._check(self._lib.lfi_grid_modified(self._h))

    def fill_synthetic(self, seed: int, g0: int | None = None, g1: int | None = None) -> None:
        if g0 is None and g1 is None:
            self._check(self._lib.lfi_fill_synthetic(self._h, seed))
        else:
            self._check(self._lib.lfi_fill_synthetic_images(self._h, seed, g0 or 0, self.n_images if g1 is None else g1))

    def fill_synthetic_scene(self, seed: int) -> None:
        """Structured light field (texture at a piecewise-constant focus) for focus-map timing; call after set_params."""
        self._check(self._lib.lfi_fill_synthetic_scene(self._h, seed))

    # -- parameters --------------------------------------------------------------------------------------------
    def set_params(self, hp, flags: int = 0) -> None:
        """hp: lfinterpolator_amd.host.HostParams (or anything with the same arrays)."""
        p = _Params()
        foc = np.ascontiguousarray(hp.focused_offsets, dtype=np.int32)
        off = np.ascontiguousarray(hp.offsets, dtype=np.float32)
        w = np.ascontiguousarray(hp.weights, dtype=np.uint16)
        ids = np.ascontiguousarray(hp.focus_map_ids, dtype=np.int32)
        assert foc.shape == (self.n_images, 2) and off.shape == (self.n_images, 2) and w.shape[1] == self.n_images
        p.views = w.shape[0]
        p.focused_offsets = foc.ctypes.data
        p.offsets = off.ctypes.data
        p.weights_fp16 = w.ctypes.data
        p.focus_map_ids = ids.ctypes.data if len(ids) else None
        p.n_focus_ids = len(ids)
        p.focus = float(hp.focus)
        p.range = float(hp.range)
        p.block_radius[0] = int(hp.block_radius[0])
        p.block_radius[1] = int(hp.block_radius[1])
        p.flags = flags
        self._check(self._lib.lfi_set_params(self._h, C.byref(p)))
        self.views = w.shape[0]

    def set_view_offsets(self, offsets_vn: np.ndarray | None) -> None:
        """Per-view focus (lfi_set_view_offsets): offsets_vn is [views][N][2] int32 — view v samples image g at pixel + offsets_vn[v][g]
        (lfinterpolator_amd.build_view_offsets computes them); None clears them."""
        self._set_view_rows(self._lib.lfi_set_view_offsets, offsets_vn, np.int32)

    def set_view_float_offsets(self, offsets_vn: np.ndarray | None) -> None:
        """Per-view float offsets for all-focus renders (lfi_set_view_float_offsets): offsets_vn is [views][N][2] float32 — view v samples
        image g at (int)fma(f, offsets_vn[v][g], pixel) (lfinterpolator_amd.build_view_centred_offsets computes them); None clears them."""
        self._set_view_rows(self._lib.lfi_set_view_float_offsets, offsets_vn, np.float32)

    def _set_view_rows(self, fn, rows_vn, dtype) -> None:
        if rows_vn is None:
            self._check(fn(self._h, None, 0))
            return
        r = np.ascontiguousarray(rows_vn, dtype=dtype)
        assert r.ndim == 3 and r.shape[1:] == (self.n_images, 2), r.shape
        self._check(fn(self._h, _ptr(r), r.shape[0]))

    def set_output_layout(self, layout) -> None:
        """'rgba' (the reference's planes) or 'planar' (alpha-free byte planes; downloads re-create alpha = 255)."""
        self._check(self._lib.lfi_set_output_layout(self._h, LAYOUTS[layout] if isinstance(layout, str) else layout))

    def view_layout(self) -> ViewLayout:
        vl = ViewLayout()
        self._check(self._lib.lfi_view_layout(self._h, C.byref(vl)))
        return vl

    def attach_views(self, device_ptr: int, nbytes: int) -> None:
        self._check(self._lib.lfi_attach_views(self._h, C.c_void_p(device_ptr), nbytes))

    def views_device_ptr(self):
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._lib.lfi_views_device_ptr(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    # -- kernels -------------------------------------------------------------------------------------------------
    def focus_map(self) -> None:
        self._check(self._lib.lfi_focus_map(self._h))

    def set_focus_steps(self, steps: int) -> None:
        """Fine focus maps (lfi_set_focus_steps): focus_map chooses every pixel's focus from `steps` candidates of [focus, focus + range], a
        multiple of 32 from 32 (the default: the reference's) to 256.  A context setting; view_focus_maps keeps 32 and focus_tiles takes its own `steps`."""
        self._check(self._lib.lfi_set_focus_steps(self._h, int(steps)))

    def set_yuv_siting(self, in_siting="centre", out_siting="centre") -> None:
        """Chroma siting of YUV 4:2:0 frames (lfi_set_yuv_siting): "centre" (JPEG, MPEG-1, Y4M's C420jpeg; the default) or "left" (MPEG-2,
        H.264, HEVC, AV1, Y4M's C420mpeg2) — in_siting for the frames the upload_images_yuv* calls read, out_siting for the frames
        download_views_yuv*, render_stream_yuv420 and download_quilt_yuv write (download_rgbd_yuv refuses left).  A context setting: it lives
        until it is changed.  Takes the names or the LFI_YUV_SITING_* values."""
        self._check(self._lib.lfi_set_yuv_siting(self._h, YUV_SITINGS.get(in_siting, in_siting), YUV_SITINGS.get(out_siting, out_siting)))

    def yuv_siting(self) -> tuple[str, str]:
        """(in_siting, out_siting) as names (lfi_yuv_siting)"""
        a, b = C.c_int(0), C.c_int(0)
        self._check(self._lib.lfi_yuv_siting(self._h, C.byref(a), C.byref(b)))
        names = {v: k for k, v in YUV_SITINGS.items()}
        return names[a.value], names[b.value]

    def focus_steps(self) -> int:
        out = C.c_int(0)
        self._check(self._lib.lfi_focus_steps(self._h, C.byref(out)))
        return out.value

    def focus_curve(self, x0: int, y0: int, x1: int, y1: int, steps: int = 32):
        """Autofocus (lfi_focus_curve): the focus curve of the region [x0, x1) x [y0, y1) over `steps` candidates of [focus, focus + range]
        of the current parameters.  Returns (cost [steps] uint64, best_index, best_focus as np.float32); the candidates themselves are
        lfinterpolator_amd.focus_candidates(focus, range, steps)."""
        cost = np.full(max(int(steps), 0), 0xC3C3C3C3C3C3C3C3, dtype=np.uint64)   # a sentinel: every element is written
        res = FocusCurveResult(-1, float("nan"), 0)
        self._check(self._lib.lfi_focus_curve(self._h, x0, y0, x1, y1, steps, _ptr(cost), C.byref(res)))
        self.focus_curve_pixels = int(res.pixels)   # the region's size as the library counted it
        return cost, int(res.best_index), np.float32(res.best_focus)

    def focus_tiles(self, tiles_x: int, tiles_y: int, steps: int = 32):
        """Focus tiles (lfi_focus_tiles; steps != 32: lfi_focus_tiles_steps): the focus curve of every tile of a tiles_x x tiles_y grid over the
        frame (the rectangles of lfinterpolator_amd.focus_tile_rect), over `steps` candidates of the current parameters — a multiple of 32 from
        32 (the estimate's) to 256, an argument of this call that set_focus_steps has nothing to do with.  Returns (cost
        [tiles_y][tiles_x][steps] uint64, best_index [tiles_y][tiles_x] int32, best_focus [tiles_y][tiles_x] float32); every tile is what
        focus_curve gives for its rectangle and `steps`."""
        ny, nx, steps = max(int(tiles_y), 0), max(int(tiles_x), 0), int(steps)
        cost = np.full((ny, nx, max(steps, 0)), 0xC3C3C3C3C3C3C3C3, dtype=np.uint64)   # a sentinel: every element is written
        res = (FocusCurveResult * max(nx * ny, 1))()
        for r in res:
            r.best_index, r.best_focus, r.pixels = -1, float("nan"), 0
        if steps == 32:
            self._check(self._lib.lfi_focus_tiles(self._h, tiles_x, tiles_y, _ptr(cost), res))
        else:
            self._check(self._lib.lfi_focus_tiles_steps(self._h, tiles_x, tiles_y, steps, _ptr(cost), res))
        self.focus_tiles_pixels = np.array([r.pixels for r in res[:nx * ny]], dtype=np.uint64).reshape(ny, nx)
        best_index = np.array([r.best_index for r in res[:nx * ny]], dtype=np.int32).reshape(ny, nx)
        best_focus = np.array([r.best_focus for r in res[:nx * ny]], dtype=np.float32).reshape(ny, nx)
        return cost, best_index, best_focus

    def focus_tiles_passes(self) -> int:
        """The factored passes the last focus_tiles call ran (steps // 32), or 0 where it took focus_curve's kernels tile by tile."""
        return int(self._lib.lfi_focus_tiles_passes(self._h))

    def focus_route(self) -> dict:
        """The route of the last estimate call — focus_map, focus_tiles, view_focus_maps — (lfi_focus_route_info): a dict of the record's
        fields, the names as str, the arrays as lists; the per-pass arrays hold `passes` entries."""
        r = FocusRoute()
        self._check(self._lib.lfi_focus_route_info(self._h, C.byref(r)))
        out = {}
        for name, kind in FocusRoute._fields_:
            v = getattr(r, name)
            if kind is C.c_char_p:
                v = (v or b"").decode()
            elif not isinstance(v, int):
                v = [int(x) for x in v]
                if len(v) == LFI_FOCUS_ROUTE_PASSES:
                    v = v[:r.passes]
            out[name] = v
        return out

    def view_focus_maps(self, ids_vk: np.ndarray) -> None:
        """Per-view focus maps (lfi_view_focus_maps): ids_vk is [views][n_ids] int32 — row v = the images view v's map samples
        (lfinterpolator_amd.build_view_focus_ids computes them); needs the float rows of set_view_float_offsets."""
        ids = np.ascontiguousarray(ids_vk, dtype=np.int32)
        assert ids.ndim == 2, ids.shape
        self._check(self._lib.lfi_view_focus_maps(self._h, _ptr(ids), ids.shape[0], ids.shape[1]))

    def render(self, method, all_focus: bool = False, v0: int = 0, v1: int | None = None) -> None:
        m = METHODS[method] if isinstance(method, str) else method
        self._check(self._lib.lfi_render(self._h, m, int(all_focus), v0, self.views if v1 is None else v1))

    def prepare(self, method, all_focus: bool = False, v0: int = 0, v1: int | None = None) -> None:
        m = METHODS[method] if isinstance(method, str) else method
        self._check(self._lib.lfi_prepare(self._h, m, int(all_focus), v0, self.views if v1 is None else v1))

    def memory_info(self) -> MemoryInfo:
        mi = MemoryInfo()
        self._check(self._lib.lfi_memory_info(self._h, C.byref(mi)))
        return mi

    def std_band_info(self) -> StdBandInfo:
        """The band method's self-check on this device (runs it if it has not run yet)."""
        info = StdBandInfo()
        self._check(self._lib.lfi_std_band_info(self._h, C.byref(info)))
        return info

    def last_kernel_name(self) -> str:
        return self._lib.lfi_last_kernel_name(self._h).decode()

    def render_stream(self, method, weights: np.ndarray, out: np.ndarray | None = None, all_focus: bool = False) -> None:
        """weights: [total_views][N] fp16 bits of the whole path; out: None or a [total_views][H][W][4] u8 array (ideally from
        pinned_empty) that receives every view."""
        m = METHODS[method] if isinstance(method, str) else method
        w = np.ascontiguousarray(weights, dtype=np.uint16)
        assert w.ndim == 2 and w.shape[1] == self.n_images
        if out is not None:
            assert out.shape == (w.shape[0], self.height, self.width, 4) and out.dtype == np.uint8 and out.flags.c_contiguous
        self._check(self._lib.lfi_render_stream(self._h, m, int(all_focus), _ptr(w), w.shape[0], _ptr(out) if out is not None else None,
                                                self.width * 4))

    def compare_view(self, v: int, reference: np.ndarray) -> Quality:
        ref = np.ascontiguousarray(reference, dtype=np.uint8)
        assert ref.shape == (self.height, self.width, 4)
        q = Quality()
        self._check(self._lib.lfi_compare_view(self._h, v, _ptr(ref), self.width * 4, C.byref(q)))
        return q

    def keep_views(self, v0: int = 0, n: int | None = None) -> None:
        """Keep views [v0, v0 + n) (default: all from v0) as they are now on the device, as the references of compare_views(None)
        (lfi_keep_views: stream-ordered device copy; later renders do not touch them)."""
        self._check(self._lib.lfi_keep_views(self._h, v0, self.views - v0 if n is None else n))

    def drop_kept_views(self) -> None:
        self._check(self._lib.lfi_keep_views(self._h, 0, 0))

    def compare_views(self, refs: np.ndarray | None = None, v0: int = 0, n: int | None = None):
        """PSNR / SSIM of views [v0, v0 + n) in one device pass (lfi_compare_views) against refs — [n][H][W][4] uint8 whose pixels are
        contiguous (row pitch and image stride are the array's: a slice of a larger array, or one from pinned_empty, is read in place) — or,
        refs None, against the kept views (keep_views).  n defaults to len(refs), or to all views from v0.
        Returns (the per-view records: a ctypes array of ViewQuality, the aggregate Quality)."""
        if refs is not None:
            assert refs.dtype == np.uint8 and refs.ndim == 4 and refs.shape[1:] == (self.height, self.width, 4), refs.shape
            assert refs.strides[2:] == (4, 1) and refs.strides[0] >= 0 and refs.strides[1] >= 0, refs.strides
            n = refs.shape[0] if n is None else n
            assert n <= refs.shape[0]
        elif n is None:
            n = self.views - v0
        out = (ViewQuality * max(n, 1))()
        agg = Quality()
        self._check(self._lib.lfi_compare_views(self._h, v0, n, _ptr(refs) if refs is not None else None, refs.strides[1] if refs is not None else 0,
                                                refs.strides[0] if refs is not None else 0, out, C.byref(agg)))
        return out, agg

    def benchmark(self, method, all_focus=False, v0=0, v1=None, warmup=3, runs=20) -> BenchStats:
        m = METHODS[method] if isinstance(method, str) else method
        st = BenchStats()
        self._check(self._lib.lfi_benchmark(self._h, m, int(all_focus), v0, self.views if v1 is None else v1, warmup,
                                            runs, C.byref(st)))
        return st

    def timer_start(self) -> None:
        self._check(self._lib.lfi_timer_start(self._h))

    def timer_stop(self) -> float:
        ms = C.c_float()
        self._check(self._lib.lfi_timer_stop(self._h, C.byref(ms)))
        return ms.value

    def sync(self) -> None:
        self._check(self._lib.lfi_sync(self._h))

    def set_stream(self, hip_stream: int | None) -> None:
        self._check(self._lib.lfi_set_stream(self._h, C.c_void_p(hip_stream or 0)))

    def set_variant(self, method, name: str) -> None:
        m = METHODS[method] if isinstance(method, str) else method
        self._check(self._lib.lfi_set_variant(self._h, m, name.encode()))

    def list_variants(self, method) -> list[str]:
        m = METHODS[method] if isinstance(method, str) else method
        return self._lib.lfi_list_variants(m).decode().split(",")

    # -- results -------------------------------------------------------------------------------------------------
    def download_view(self, v: int, out: np.ndarray | None = None) -> np.ndarray:
        """Whole-image array; with a row window only rows [out_y0, out_y1) are filled (the rest stays zero).
        `out` may be a page-locked array from `pinned_empty` (a true DMA instead of a staged copy)."""
        if out is None:
            out = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        assert out.shape == (self.height, self.width, 4) and out.dtype == np.uint8 and out.flags.c_contiguous
        self._check(self._lib.lfi_download_view(self._h, v, _ptr(out), self.width * 4))
        return out

    def download_views(self, v0: int = 0, v1: int | None = None, out: np.ndarray | None = None) -> np.ndarray:
        v1 = self.views if v1 is None else v1
        if out is None:
            return np.stack([self.download_view(v) for v in range(v0, v1)])
        assert out.shape == (v1 - v0, self.height, self.width, 4)
        for v in range(v0, v1):
            self.download_view(v, out[v - v0])
        return out

    def pinned_empty(self, shape, dtype=np.uint8) -> np.ndarray:
        """A numpy array over page-locked host memory (lfi_alloc_pinned); freed when the context is closed."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        self._check(self._lib.lfi_alloc_pinned(nbytes, C.byref(p)))
        self._pinned.append(p.value)
        buf = (C.c_uint8 * nbytes).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def download_quilt_tiles(self, out: np.ndarray, tiles_x: int, tiles_y: int, first_tile: int, n: int, v0: int = 0) -> None:
        """views v0 … v0+n-1 into tiles first_tile … of the quilt image `out` ((tiles_y·H, tiles_x·W, 4) uint8, C-contiguous)"""
        assert out.dtype == np.uint8 and out.flags.c_contiguous and out.shape == (tiles_y * self.height, tiles_x * self.width, 4)
        self._check(self._lib.lfi_download_quilt_tiles(self._h, tiles_x, tiles_y, first_tile, n, v0, _ptr(out), tiles_x * self.width * 4))

    def download_quilt(self, tiles_x: int, tiles_y: int, v0: int = 0) -> np.ndarray:
        out = np.full((tiles_y * self.height, tiles_x * self.width, 4), 0xC3, dtype=np.uint8)   # a sentinel, not zeros: every byte is written
        self._check(self._lib.lfi_download_quilt(self._h, tiles_x, tiles_y, v0, _ptr(out), tiles_x * self.width * 4))
        return out

    def download_quilt_tiles_scaled(self, out: np.ndarray, tiles_x: int, tiles_y: int, first_tile: int, n: int, tile_w: int, tile_h: int, v0: int = 0) -> None:
        """views v0 … v0+n-1, each resized to tile_w × tile_h by the exact area filter of lfi_download_quilt_scaled, into tiles first_tile … of
        the quilt image `out`: (tiles_y·tile_h, P, 4) uint8 with rows of P ≥ tiles_x·tile_w pixels — the row pitch is out's; the library refuses one that is too small"""
        assert out.dtype == np.uint8 and out.ndim == 3 and out.shape[0] == tiles_y * tile_h and out.shape[2] == 4 and (out.size == 0 or out.strides[1:] == (4, 1))
        self._check(self._lib.lfi_download_quilt_tiles_scaled(self._h, tiles_x, tiles_y, first_tile, n, v0, tile_w, tile_h, _ptr(out), out.strides[0]))

    def download_quilt_scaled(self, tiles_x: int, tiles_y: int, tile_w: int, tile_h: int, v0: int = 0, out: np.ndarray | None = None) -> np.ndarray:
        """the quilt of views v0 … with every view resized to tile_w × tile_h on the device (a 1 × 1 quilt: view v0 as a thumbnail); `out` as in
        download_quilt_tiles_scaled, by default a new (tiles_y·tile_h, tiles_x·tile_w, 4) array"""
        if out is None:
            out = np.full((tiles_y * max(tile_h, 0), tiles_x * max(tile_w, 0), 4), 0xC3, dtype=np.uint8)   # a sentinel, not zeros: every byte is written
        assert out.dtype == np.uint8 and out.ndim == 3 and out.shape[0] == tiles_y * tile_h and out.shape[2] == 4 and (out.size == 0 or out.strides[1:] == (4, 1))
        self._check(self._lib.lfi_download_quilt_scaled(self._h, tiles_x, tiles_y, v0, tile_w, tile_h, _ptr(out), out.strides[0]))
        return out

    def download_native(self, lens: "Lenticular | None", out_w: int, out_h: int, tile_w: int | None = None, tile_h: int | None = None, v0: int = 0,
                        out: np.ndarray | None = None) -> np.ndarray:
        """the native image of a lenticular display, out_w × out_h pixels, interlaced on the device from views v0 … v0+lens.views-1, each resized
        to tile_w × tile_h first (default: the views' size, read in place); `out`: (out_h, P, 4) uint8 with rows of P ≥ out_w pixels — the row
        pitch is out's; by default a new (out_h, out_w, 4) array"""
        tile_w = self.width if tile_w is None else tile_w
        tile_h = self.height if tile_h is None else tile_h
        if out is None:
            out = np.full((max(out_h, 0), max(out_w, 0), 4), 0xC3, dtype=np.uint8)   # a sentinel, not zeros: every byte is written
        assert out.dtype == np.uint8 and out.ndim == 3 and out.shape[0] == out_h and out.shape[2] == 4 and (out.size == 0 or out.strides[1:] == (4, 1))
        self._check(self._lib.lfi_download_native(self._h, C.byref(lens) if lens is not None else None, v0, out_w, out_h, tile_w, tile_h, _ptr(out),
                                                  out.strides[0] if out.size else 0))
        return out

    def yuv420_frame_bytes(self) -> int:
        """bytes of one I420 frame of a view: W·H + 2·((W + 1) // 2)·((H + 1) // 2)"""
        return self.width * self.height + 2 * ((self.width + 1) // 2) * ((self.height + 1) // 2)

    def download_views_yuv420(self, v0: int = 0, n: int | None = None, matrix="709", range="limited", out: np.ndarray | None = None) -> np.ndarray:
        """views [v0, v0 + n) (default: all from v0) as 8-bit YUV 4:2:0 frames (I420: Y, Cb, Cr planes, tightly packed), converted on the device
        (lfi_download_views_yuv420).  matrix: "709" / "601" (or LFI_YUV_BT*), range: "limited" / "full" (or LFI_YUV_*).  `out`: [n][P] uint8 with
        rows of P ≥ frame bytes — the frame stride is out's; by default a new [n][frame_bytes] array."""
        n = self.views - v0 if n is None else n
        fb = self.yuv420_frame_bytes()
        if out is None:
            out = np.full((max(n, 0), fb), 0xC3, dtype=np.uint8)   # a sentinel, not zeros: every byte is written
        assert out.dtype == np.uint8 and out.ndim == 2 and out.shape[0] == n and (out.size == 0 or out.strides[1] == 1)
        self._check(self._lib.lfi_download_views_yuv420(self._h, v0, n, YUV_MATRICES.get(matrix, matrix), YUV_RANGES.get(range, range), _ptr(out),
                                                        out.strides[0] if out.size else 0))
        return out[:, :fb] if out.size else out

    def download_views_yuv(self, surfaces: YuvSurfaces, n: int | None = None, v0: int = 0, matrix="709", range="limited") -> None:
        """views [v0, v0 + n) (default: all from v0) into n frames of `surfaces` (lfi_download_views_yuv): only the planes' own bytes are
        written; device surfaces whose base, pitches, offsets and stride are multiples of 16 are written by the kernel itself."""
        n = self.views - v0 if n is None else n
        self._check(self._lib.lfi_download_views_yuv(self._h, v0, n, YUV_MATRICES.get(matrix, matrix), YUV_RANGES.get(range, range),
                                                     C.byref(surfaces) if surfaces is not None else None))

    def download_deep_views(self, v0: int = 0, n: int | None = None) -> np.ndarray:
        """the deep views [v0, v0 + n) (default: all from v0) of the last deep render (set_params(..., flags=LFI_FLAG_DEEP_VIEWS)) as
        [n][H][W][3: R,G,B] uint16 10-bit codes: lfi_download_views_yuv into host LFI_YUV_GBRP10 surfaces"""
        n = self.views - v0 if n is None else n
        frames = np.full((max(n, 1), 3, self.height, self.width), 0xC3C3, dtype=np.uint16)   # a sentinel, not zeros: every sample is written
        self.download_views_yuv(YuvSurfaces.gbrp10_from_array(frames), n, v0)
        return YuvSurfaces.gbrp10_to_rgb(frames[:n])

    def download_quilt_yuv(self, tiles_x: int, tiles_y: int, v0: int, tile_w: int, tile_h: int, matrix, range, surfaces: YuvSurfaces) -> None:
        """the scaled quilt of views v0 … (download_quilt_scaled's tiles) as ONE YUV 4:2:0 frame of tiles_x·tile_w × tiles_y·tile_h in `surfaces`
        (lfi_download_quilt_yuv): a frame of a quilt video.  Only the planes' own bytes are written; even tile sizes take one kernel and no RGBA
        quilt; a device surface whose base, pitches and offsets are multiples of 16 is written by the kernel itself."""
        self._check(self._lib.lfi_download_quilt_yuv(self._h, tiles_x, tiles_y, v0, tile_w, tile_h, YUV_MATRICES.get(matrix, matrix),
                                                     YUV_RANGES.get(range, range), C.byref(surfaces) if surfaces is not None else None))

    def download_rgbd_yuv(self, v0: int, n: int, map_k: int, flags: int, tile_w: int, tile_h: int, matrix, range, surfaces: YuvSurfaces) -> None:
        """views [v0, v0 + n) with a focus map beside each as n YUV 4:2:0 frames of 2·tile_w × tile_h in `surfaces` (lfi_download_rgbd_yuv): RGB-D
        video, the colour left, the depth right.  The depth is the R byte of the context's map map_k, or with LFI_RGBD_VIEW_MAPS of each view's
        own map map_k; LFI_RGBD_INVERT takes 255 − it before the resize.  Tile sizes are even; only the planes' own bytes are written."""
        self._check(self._lib.lfi_download_rgbd_yuv(self._h, v0, n, map_k, flags, tile_w, tile_h, YUV_MATRICES.get(matrix, matrix),
                                                    YUV_RANGES.get(range, range), C.byref(surfaces) if surfaces is not None else None))

    def render_stream_yuv420(self, method, weights: np.ndarray, out: np.ndarray | None = None, all_focus: bool = False, matrix="709",
                             range="limited") -> np.ndarray:
        """render_stream with YUV 4:2:0 frames for its downloads (lfi_render_stream_yuv420): weights [total_views][N] fp16 bits of the whole
        path; `out`: [total_views][P] uint8 with rows of P ≥ frame bytes (ideally from pinned_empty), by default a new [total_views][frame_bytes]
        array.  Either view layout."""
        m = METHODS[method] if isinstance(method, str) else method
        w = np.ascontiguousarray(weights, dtype=np.uint16)
        assert w.ndim == 2 and w.shape[1] == self.n_images
        fb = self.yuv420_frame_bytes()
        if out is None:
            out = np.full((w.shape[0], fb), 0xC3, dtype=np.uint8)
        assert out.dtype == np.uint8 and out.ndim == 2 and out.shape[0] == w.shape[0] and (out.size == 0 or out.strides[1] == 1)
        self._check(self._lib.lfi_render_stream_yuv420(self._h, m, int(all_focus), _ptr(w), w.shape[0], YUV_MATRICES.get(matrix, matrix),
                                                       YUV_RANGES.get(range, range), _ptr(out), out.strides[0] if out.size else 0))
        return out[:, :fb] if out.size else out

    def download_map(self, k: int) -> np.ndarray:
        out = np.empty((self.height, self.width, 4), dtype=np.uint8)
        self._check(self._lib.lfi_download_map(self._h, k, _ptr(out), self.width * 4))
        return out

    def upload_map(self, k: int, rgba: np.ndarray) -> None:
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        assert rgba.shape == (self.height, self.width, 4)
        self._check(self._lib.lfi_upload_map(self._h, k, _ptr(rgba), self.width * 4))

    def download_view_map(self, v: int, k: int) -> np.ndarray:
        out = np.empty((self.height, self.width, 4), dtype=np.uint8)
        self._check(self._lib.lfi_download_view_map(self._h, v, k, _ptr(out), self.width * 4))
        return out

    def upload_view_map(self, v: int, k: int, rgba: np.ndarray) -> None:
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        assert rgba.shape == (self.height, self.width, 4)
        self._check(self._lib.lfi_upload_view_map(self._h, v, k, _ptr(rgba), self.width * 4))

    def download_coords(self, g: int, all_focus: bool = False, map_index: int = 1) -> np.ndarray:
        out = np.empty((self.height, self.width, 2), dtype=np.int32)
        self._check(self._lib.lfi_download_coords(self._h, g, int(all_focus), map_index, _ptr(out)))
        return out

    def download_prequant(self, method, v: int, all_focus: bool = False) -> np.ndarray:
        m = METHODS[method] if isinstance(method, str) else method
        out = np.empty((self.height, self.width, 3), dtype=np.float32)
        self._check(self._lib.lfi_download_prequant(self._h, m, int(all_focus), v, _ptr(out)))
        return out

    def debug_mfma_f16_chain(self, a_bits: np.ndarray, b_bits: np.ndarray, shape: int = 0) -> np.ndarray:
        """C[32][32] = A[32][K] · B[K][32] (fp16 bit patterns) through K/16 (shape 0) or K/32 (shape 1) chained MFMAs."""
        a = np.ascontiguousarray(a_bits, dtype=np.uint16)
        b = np.ascontiguousarray(b_bits, dtype=np.uint16)
        k = a.shape[1]
        assert a.shape == (32, k) and b.shape == (k, 32)
        c = np.empty((32, 32), dtype=np.float32)
        self._check(self._lib.lfi_debug_mfma_f16_chain(self._h, shape, k, _ptr(a), _ptr(b), _ptr(c)))
        return c

    def debug_pk_minmax3_f16(self) -> int:
        """Mismatching halves of v_pk_minimum3_f16 / v_pk_maximum3_f16 against integer min / max over all byte triples."""
        out = C.c_uint32(0xffffffff)
        self._check(self._lib.lfi_debug_pk_minmax3_f16(self._h, C.byref(out)))
        return int(out.value)

    def debug_streams(self) -> tuple[int, int, int]:
        """tests: the hipStream_t handles of the context's own compute stream, its copy stream and its side stream (lfi_debug_streams);
        the latter two are created if they do not exist yet"""
        out = (C.c_void_p * 3)()
        self._check(self._lib.lfi_debug_streams(self._h, out))
        return tuple(int(v or 0) for v in out)

    def poison(self, what: int, byte: int) -> None:
        """Fill the buffers selected by the LFI_POISON_* bits in `what` with `byte` (stream-ordered; caches are rebuilt by their next user)."""
        self._check(self._lib.lfi_debug_poison(self._h, what, byte))

    def debug_mfma_f16(self, a_bits: np.ndarray, b_bits: np.ndarray) -> np.ndarray:
        a = np.ascontiguousarray(a_bits, dtype=np.uint16)
        b = np.ascontiguousarray(b_bits, dtype=np.uint16)
        assert a.shape == (32, 16) and b.shape == (16, 32)
        c = np.empty((32, 32), dtype=np.float32)
        self._check(self._lib.lfi_debug_mfma_f16(self._h, _ptr(a), _ptr(b), _ptr(c)))
        return c
