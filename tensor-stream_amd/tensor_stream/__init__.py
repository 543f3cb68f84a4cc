"""tensor_stream: MI355X-native Video Post Processing path behind the reference's Python surface.

Same package name as the reference's (`from tensor_stream import ...`), so user code switches by
putting `tensor-stream_amd/` on sys.path.
"""
from .vpp import FourCC, FrameParameters, Planes, ResizeType, VideoProcessor, default_coeffs, describe, describe_rois, describe_rois_area, describe_rois_sized, sizes_for_height, pyramid_sizes, describe_letterbox, describe_letterbox_area, describe_warp, describe_perspective, describe_warp_bicubic, describe_perspective_bicubic, describe_remap, describe_mesh, letterbox_rect, output_shape, tensor_spec, perspective_from_opencv, perspective_from_quad, remap_from_grid, remap_from_opencv, remap_lds_hint, mesh_dims, mesh_error, mesh_expand, mesh_from_map, mesh_lds_hint, mesh_undistort, warp_from_opencv, warp_rotated_box  # noqa: F401

from ._native import Rect, Roi, TensorSpec  # noqa: F401
from .tensor_stream import FrameRate, FrameRing, LogsLevel, LogsType, StatusLevel, TensorStreamConverter  # noqa: F401

__version__ = "0.1.0"
