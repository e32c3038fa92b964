"""lfinterpolator_amd — MI355X (gfx950) light-field view interpolation hot path.

The product is the C-ABI library ``lib/liblfi_hip.so`` (hand-written HIP kernels, ``include/lfi.h``) plus the C++ host
code in ``csrc/host`` (``Interpolator``, ``LfLoader``, the command line).  This Python package is plumbing for tests and
``bench.py``: a ctypes binding of the two shared libraries.  There is no CPU fallback — importing works without a GPU
(so that the build and symbol checks can run anywhere), but creating a context raises unless a gfx950 device and the
built library are present.
"""
from .abi import (LFI_METHOD_STD, LFI_METHOD_TEN_WM, LFI_FLAG_UNIFIED_FOCUS_MAP, LFI_FLAG_TEN_ROUND_PER_BATCH, LFI_FLAG_SINGLE_SWEEP_DIRECTION, LFI_FLAG_STD_ANALYTIC_BAND, LFI_FLAG_STD_MEASURED_BAND, LFI_FLAG_STD_BAND_PROBE_FAIL, LFI_FLAG_DEEP_VIEWS, LFI_FLAG_IN_FRAME, LFI_FLAG_LINEAR_LIGHT, LFI_POISON_DEEP, LFI_YUV_DEEP, LFI_YUV_GBRP10,
                  LFI_LAYOUT_RGBA, LFI_LAYOUT_PLANAR_RGB,
                  LFI_POISON_VIEWS, LFI_POISON_SCRATCH, LFI_POISON_MAPS, LFI_POISON_FOCUS_WORKSPACE, LFI_POISON_DERIVED, LFI_POISON_VIEW_MAPS, LFI_LENT_INVERT, LFI_LENT_BGR, LFI_LENT_BILINEAR, LFI_LENT_BLEND, LFI_RGBD_INVERT, LFI_RGBD_VIEW_MAPS,
                  LFI_YUV_BT709, LFI_YUV_BT601, LFI_YUV_LIMITED, LFI_YUV_FULL, LFI_CHROMA_BILINEAR, LFI_CHROMA_NEAREST, LFI_YUV_SITING_CENTRE, LFI_YUV_SITING_LEFT, YUV_SITINGS,
                  LFI_YUV_I420, LFI_YUV_NV12, LFI_YUV_10BIT, LFI_YUV_I010, LFI_YUV_P010, LFI_MEM_HOST, LFI_MEM_DEVICE, YuvSurfaces, yuv_surfaces_packed, DerivedLayout, LFI_YUV_DERIVED_SPAN,
                  LFI_MOSAIC_ROWS, LFI_MOSAIC_GRID, LFI_MOSAIC_BOTTOM_UP, Mosaic,
                  Context, Lenticular, LfiError, ViewQuality, load_hip_library, ABI_SYMBOLS)
from .host import HostParams, build_params, load_host_library, load_image, write_png, load_grid, focus_ramp, focus_candidates, focus_tile_rect, focus_auto_range, area_span, native_taps, linear_tables, linear_encode, lenticular, lenticular_file, write_y4m, read_y4m_info, read_y4m, y4m_input_siting, load_grid_y4m, mosaic_map, upload_mosaic_yuv, upload_mosaic_yuv_derived, upload_mosaic, build_view_offsets, build_view_centred_offsets, build_view_focus_ids
from .build import build_all
from .sharding import view_range, rank_params, broadcast_grid, allgather_grid, image_slice, row_band, input_rows, input_rows_all_focus
from . import build

__all__ = ["LFI_MOSAIC_ROWS", "LFI_MOSAIC_GRID", "LFI_MOSAIC_BOTTOM_UP", "Mosaic", "mosaic_map", "upload_mosaic_yuv", "upload_mosaic_yuv_derived", "upload_mosaic", "DerivedLayout", "LFI_YUV_DERIVED_SPAN", "LFI_LAYOUT_RGBA", "LFI_LAYOUT_PLANAR_RGB", "LFI_POISON_VIEWS", "LFI_POISON_SCRATCH", "LFI_POISON_MAPS", "LFI_POISON_FOCUS_WORKSPACE", "LFI_POISON_DERIVED", "LFI_POISON_VIEW_MAPS", "LFI_LENT_INVERT", "LFI_LENT_BGR", "LFI_LENT_BILINEAR", "LFI_LENT_BLEND", "LFI_RGBD_INVERT", "LFI_RGBD_VIEW_MAPS", "Lenticular", "lenticular", "lenticular_file", "native_taps", "linear_tables", "linear_encode", "LFI_YUV_BT709", "LFI_YUV_BT601", "LFI_YUV_LIMITED", "LFI_YUV_FULL", "LFI_CHROMA_BILINEAR", "LFI_CHROMA_NEAREST", "LFI_YUV_SITING_CENTRE", "LFI_YUV_SITING_LEFT", "YUV_SITINGS", "LFI_YUV_I420", "LFI_YUV_NV12", "LFI_YUV_10BIT", "LFI_YUV_I010", "LFI_YUV_P010", "LFI_MEM_HOST", "LFI_MEM_DEVICE", "YuvSurfaces", "yuv_surfaces_packed", "write_y4m", "read_y4m_info", "read_y4m", "y4m_input_siting", "load_grid_y4m", "LFI_METHOD_STD", "LFI_METHOD_TEN_WM", "LFI_FLAG_UNIFIED_FOCUS_MAP", "LFI_FLAG_TEN_ROUND_PER_BATCH", "LFI_FLAG_SINGLE_SWEEP_DIRECTION", "LFI_FLAG_STD_ANALYTIC_BAND", "LFI_FLAG_STD_MEASURED_BAND", "LFI_FLAG_STD_BAND_PROBE_FAIL", "LFI_FLAG_DEEP_VIEWS", "LFI_FLAG_IN_FRAME", "LFI_FLAG_LINEAR_LIGHT", "LFI_POISON_DEEP", "LFI_YUV_DEEP", "LFI_YUV_GBRP10",
           "Context", "LfiError", "ViewQuality", "load_hip_library", "ABI_SYMBOLS", "HostParams", "build_params", "load_host_library", "load_image", "write_png", "load_grid",
           "focus_ramp", "focus_candidates", "focus_tile_rect", "focus_auto_range", "area_span", "build_view_offsets", "build_view_centred_offsets", "build_view_focus_ids", "build_all", "view_range", "rank_params", "broadcast_grid", "allgather_grid", "image_slice", "row_band", "input_rows", "input_rows_all_focus"]
