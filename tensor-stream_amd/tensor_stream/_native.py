"""ctypes binding of libtsvpp.so (the C ABI in include/tsvpp.h).

Fails loudly when the HIP library is missing: there is no CPU or PyTorch fallback for the VPP path.
"""
import ctypes
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_PKG, "..", "lib", "libtsvpp.so"))

TSVPP_MAX_BATCH = 128
TSVPP_MAX_ROIS = 64  # boxes per launch of tsvpp_convert_rois (their records travel in the kernarg segment)
TSVPP_MAX_ROIS_AREA = 64  # ... of tsvpp_convert_rois_area
TSVPP_MAX_ROIS_SIZED = 48  # ... of tsvpp_convert_rois_sized (64-byte records)
TSVPP_MAX_LETTERBOX = 32  # frames per launch of tsvpp_convert_letterbox
TSVPP_MAX_WARPS = 32  # outputs per launch of tsvpp_convert_warp
TSVPP_MAX_PERSP = 32  # outputs per launch of tsvpp_convert_perspective
TSVPP_MAX_REMAPS = 32  # outputs per launch of tsvpp_convert_remap
TSVPP_MAX_MESHES = 32  # outputs per launch of tsvpp_convert_mesh
TSVPP_F32, TSVPP_F16, TSVPP_BF16 = 0, 1, 2  # enum tsvpp_dtype: the element of the tensor entry points
TSVPP_OPT_INPUTS_READY = 1
TSVPP_OPT_COLOR_G_TERM = 2
TSVPP_OPT_UNSAFE_COEFFS = 3


class NV12(ctypes.Structure):
    """struct tsvpp_nv12: the AVFrame fields VideoProcessor::Convert reads."""
    _fields_ = [("y", ctypes.c_void_p), ("uv", ctypes.c_void_p),
                ("pitch_y", ctypes.c_int32), ("pitch_uv", ctypes.c_int32),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32)]


class Params(ctypes.Structure):
    """struct tsvpp_params: flat FrameParameters {resize, color, crop}."""
    _fields_ = [("crop_left", ctypes.c_int32), ("crop_top", ctypes.c_int32),
                ("crop_right", ctypes.c_int32), ("crop_bottom", ctypes.c_int32),
                ("dst_width", ctypes.c_int32), ("dst_height", ctypes.c_int32),
                ("resize_type", ctypes.c_int32), ("fourcc", ctypes.c_int32),
                ("planes", ctypes.c_int32), ("normalization", ctypes.c_int32)]


class Roi(ctypes.Structure):
    """struct tsvpp_roi: box [left, right) x [top, bottom) of frame `frame` (tsvpp_convert_rois)."""
    _fields_ = [("frame", ctypes.c_int32), ("left", ctypes.c_int32), ("top", ctypes.c_int32),
                ("right", ctypes.c_int32), ("bottom", ctypes.c_int32)]


class RoiSized(ctypes.Structure):
    """struct tsvpp_roi_sized: tsvpp_roi's box, then THIS box's output size (tsvpp_convert_rois_sized)."""
    _fields_ = [("frame", ctypes.c_int32), ("left", ctypes.c_int32), ("top", ctypes.c_int32),
                ("right", ctypes.c_int32), ("bottom", ctypes.c_int32), ("dst_width", ctypes.c_int32), ("dst_height", ctypes.c_int32)]


class Rect(ctypes.Structure):
    """struct tsvpp_rect: the inner rectangle of a letterboxed canvas (tsvpp_convert_letterbox)."""
    _fields_ = [("left", ctypes.c_int32), ("top", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32)]


class Warp(ctypes.Structure):
    """struct tsvpp_warp: the output -> source matrix of one output of tsvpp_convert_warp, and the frame it samples."""
    _fields_ = [("frame", ctypes.c_int32), ("m", ctypes.c_float * 6)]


class Persp(ctypes.Structure):
    """struct tsvpp_persp: the output -> source homography (row-major) of one output of tsvpp_convert_perspective, and the frame it samples."""
    _fields_ = [("frame", ctypes.c_int32), ("h", ctypes.c_float * 9)]


class Map(ctypes.Structure):
    """struct tsvpp_map: one coordinate map of tsvpp_convert_remap in DEVICE memory -- (x, y) fp32 pairs, row pitch in bytes (0: tight), LDS hint (0: none)."""
    _fields_ = [("xy", ctypes.c_void_p), ("pitch", ctypes.c_int32), ("lds_bytes", ctypes.c_int32)]


class Mesh(ctypes.Structure):
    """struct tsvpp_mesh: one warp mesh of tsvpp_convert_mesh in DEVICE memory -- rows x cols (x, y) fp32 control points, row pitch in bytes (0: tight), the cell
    size as two logarithms (2..8), LDS hint (0: none)."""
    _fields_ = [("xy", ctypes.c_void_p), ("pitch", ctypes.c_int32), ("log2_cw", ctypes.c_int32), ("log2_ch", ctypes.c_int32), ("lds_bytes", ctypes.c_int32)]


class Remap(ctypes.Structure):
    """struct tsvpp_remap: one output of tsvpp_convert_remap -- the frame it samples and the map it samples it through."""
    _fields_ = [("frame", ctypes.c_int32), ("map", ctypes.c_int32)]


class TensorSpec(ctypes.Structure):
    """struct tsvpp_tensor_spec: element type, per-channel mean and scale (= 1 / std) of the tensor entry points."""
    _fields_ = [("dtype", ctypes.c_int32), ("mean", ctypes.c_float * 3), ("scale", ctypes.c_float * 3)]


class Coeffs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in
                ("y_scale", "v_to_r", "u_to_b", "v_to_g", "u_to_g", "round_bias", "y_offset", "c_offset")]


# every symbol include/tsvpp.h declares (tests check that the library exports all of them)
SYMBOLS = ["tsvpp_create", "tsvpp_destroy", "tsvpp_consumer_stream", "tsvpp_out_dims", "tsvpp_out_bytes",
           "tsvpp_channels", "tsvpp_convert", "tsvpp_convert_batch", "tsvpp_prepare", "tsvpp_prepare_batch", "tsvpp_enable_markers", "tsvpp_get_coeffs",
           "tsvpp_set_coeffs", "tsvpp_default_coeffs", "tsvpp_area_pattern", "tsvpp_describe", "tsvpp_strerror", "tsvpp_version",
           "tsvpp_table_create", "tsvpp_table_destroy", "tsvpp_table_set", "tsvpp_convert_table", "tsvpp_trim", "tsvpp_set_option", "tsvpp_get_option", "tsvpp_consumer_next_stream", "tsvpp_consumer_synchronize",
           "tsvpp_debug_last_launch", "tsvpp_convert_rois", "tsvpp_describe_rois", "tsvpp_convert_rois_area", "tsvpp_describe_rois_area", "tsvpp_roi_area_rows", "tsvpp_debug_area_tables",
           "tsvpp_letterbox_rect", "tsvpp_convert_letterbox", "tsvpp_describe_letterbox",
           "tsvpp_tensor_bytes", "tsvpp_convert_rois_tensor", "tsvpp_describe_rois_tensor", "tsvpp_convert_letterbox_tensor", "tsvpp_describe_letterbox_tensor",
           "tsvpp_convert_letterbox_area", "tsvpp_describe_letterbox_area", "tsvpp_letterbox_area_rows",
           "tsvpp_rois_sized_bytes", "tsvpp_convert_rois_sized", "tsvpp_describe_rois_sized", "tsvpp_convert_rois_sized_tensor", "tsvpp_describe_rois_sized_tensor",
           "tsvpp_rois_sized_tile",
           "tsvpp_convert_warp", "tsvpp_describe_warp", "tsvpp_convert_warp_tensor", "tsvpp_describe_warp_tensor", "tsvpp_warp_rotated_box", "tsvpp_warp_footprint",
           "tsvpp_convert_warp_bicubic", "tsvpp_describe_warp_bicubic", "tsvpp_warp_bicubic_footprint",
           "tsvpp_convert_perspective", "tsvpp_describe_perspective", "tsvpp_convert_perspective_tensor", "tsvpp_describe_perspective_tensor", "tsvpp_persp_from_quad",
           "tsvpp_persp_footprint", "tsvpp_convert_perspective_bicubic", "tsvpp_describe_perspective_bicubic", "tsvpp_persp_bicubic_footprint",
           "tsvpp_convert_remap", "tsvpp_describe_remap", "tsvpp_convert_remap_tensor", "tsvpp_describe_remap_tensor", "tsvpp_remap_footprint", "tsvpp_remap_lds_need",
           "tsvpp_convert_mesh", "tsvpp_describe_mesh", "tsvpp_convert_mesh_tensor", "tsvpp_describe_mesh_tensor", "tsvpp_mesh_dims", "tsvpp_mesh_expand",
           "tsvpp_mesh_from_map", "tsvpp_mesh_error", "tsvpp_mesh_lds_need"]

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the VPP path is HIP-only (gfx950). Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C tensor-stream_amd/csrc`.")
    L = ctypes.CDLL(LIB_PATH)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    pp, pn = ctypes.POINTER(Params), ctypes.POINTER(NV12)
    L.tsvpp_create.argtypes = [i32, i32, ctypes.POINTER(vp)]
    L.tsvpp_destroy.argtypes = [vp]
    L.tsvpp_destroy.restype = None
    L.tsvpp_consumer_stream.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(vp)]
    L.tsvpp_consumer_next_stream.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(vp)]
    L.tsvpp_consumer_next_stream.restype = i32
    L.tsvpp_consumer_synchronize.argtypes = [vp, ctypes.c_char_p]
    L.tsvpp_consumer_synchronize.restype = i32
    L.tsvpp_out_dims.argtypes = [pp, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.tsvpp_out_bytes.argtypes = [pp, i32, i32]
    L.tsvpp_out_bytes.restype = ctypes.c_size_t
    L.tsvpp_channels.argtypes = [i32]
    L.tsvpp_channels.restype = ctypes.c_float
    L.tsvpp_convert.argtypes = [vp, pn, pp, vp, vp]
    L.tsvpp_convert_batch.argtypes = [vp, i32, pn, pp, ctypes.POINTER(vp), vp]
    L.tsvpp_table_create.argtypes = [vp, i32, ctypes.POINTER(vp)]
    L.tsvpp_table_destroy.argtypes = [vp]
    L.tsvpp_table_destroy.restype = None
    L.tsvpp_table_set.argtypes = [vp, i32, i32, pn, ctypes.POINTER(vp), vp]
    L.tsvpp_convert_table.argtypes = [vp, vp, i32, i32, pp, vp]
    L.tsvpp_trim.argtypes = [vp, ctypes.POINTER(ctypes.c_size_t)]
    L.tsvpp_trim.restype = i32
    L.tsvpp_set_option.argtypes = [vp, i32, i32]
    L.tsvpp_set_option.restype = i32
    L.tsvpp_get_option.argtypes = [vp, i32, ctypes.POINTER(i32)]
    L.tsvpp_get_option.restype = i32
    L.tsvpp_prepare.argtypes = [vp, pp, i32, i32]
    L.tsvpp_prepare_batch.argtypes = [vp, pp, i32, i32, i32, vp]
    L.tsvpp_enable_markers.argtypes = [vp, i32]
    L.tsvpp_get_coeffs.argtypes = [vp, ctypes.POINTER(Coeffs)]
    L.tsvpp_set_coeffs.argtypes = [vp, ctypes.POINTER(Coeffs)]
    L.tsvpp_default_coeffs.argtypes = [ctypes.POINTER(Coeffs)]
    L.tsvpp_default_coeffs.restype = None
    L.tsvpp_area_pattern.argtypes = [ctypes.c_float, vp, i32, ctypes.POINTER(i32)]
    L.tsvpp_describe.argtypes = [pp, i32, i32, i32, i32, i32, i32, ctypes.c_char_p, ctypes.c_size_t]
    pr = ctypes.POINTER(Roi)
    L.tsvpp_convert_rois.argtypes = [vp, i32, pn, i32, pr, pp, ctypes.POINTER(vp), vp]
    L.tsvpp_convert_rois.restype = i32
    L.tsvpp_describe_rois.argtypes = [pp, i32, pn, i32, pr, i32, ctypes.c_char_p, ctypes.c_size_t]
    L.tsvpp_describe_rois.restype = i32
    L.tsvpp_convert_rois_area.argtypes = L.tsvpp_convert_rois.argtypes
    L.tsvpp_convert_rois_area.restype = i32
    L.tsvpp_describe_rois_area.argtypes = L.tsvpp_describe_rois.argtypes
    L.tsvpp_describe_rois_area.restype = i32
    L.tsvpp_roi_area_rows.argtypes = [ctypes.c_float, i32, i32, vp, i32, ctypes.POINTER(i32)]
    L.tsvpp_roi_area_rows.restype = i32
    pc = ctypes.POINTER(Rect)
    L.tsvpp_letterbox_rect.argtypes = [i32, i32, i32, i32, pc]
    L.tsvpp_letterbox_rect.restype = i32
    L.tsvpp_convert_letterbox.argtypes = [vp, i32, pn, pp, pc, i32, i32, i32, ctypes.POINTER(vp), vp]
    L.tsvpp_convert_letterbox.restype = i32
    L.tsvpp_describe_letterbox.argtypes = [pp, i32, pn, pc, i32, ctypes.c_char_p, ctypes.c_size_t]
    L.tsvpp_describe_letterbox.restype = i32
    ps = ctypes.POINTER(TensorSpec)
    L.tsvpp_tensor_bytes.argtypes = [pp, ps]
    L.tsvpp_tensor_bytes.restype = ctypes.c_size_t
    L.tsvpp_convert_rois_tensor.argtypes = [vp, i32, pn, i32, pr, pp, ps, ctypes.POINTER(vp), vp]
    L.tsvpp_convert_rois_tensor.restype = i32
    L.tsvpp_describe_rois_tensor.argtypes = [pp, ps, i32, pn, i32, pr, i32, ctypes.c_char_p, ctypes.c_size_t]
    L.tsvpp_describe_rois_tensor.restype = i32
    L.tsvpp_convert_letterbox_tensor.argtypes = [vp, i32, pn, pp, ps, pc, i32, i32, i32, ctypes.POINTER(vp), vp]
    L.tsvpp_convert_letterbox_tensor.restype = i32
    L.tsvpp_describe_letterbox_tensor.argtypes = [pp, ps, i32, pn, pc, i32, ctypes.c_char_p, ctypes.c_size_t]
    L.tsvpp_describe_letterbox_tensor.restype = i32
    L.tsvpp_convert_letterbox_area.argtypes = [vp, i32, pn, pp, ps, pc, i32, i32, i32, ctypes.POINTER(vp), vp]  # (spec may be None)
    L.tsvpp_convert_letterbox_area.restype = i32
    L.tsvpp_describe_letterbox_area.argtypes = [pp, ps, i32, pn, pc, i32, ctypes.c_char_p, ctypes.c_size_t]
    L.tsvpp_describe_letterbox_area.restype = i32
    L.tsvpp_letterbox_area_rows.argtypes = [ctypes.c_float, i32, i32, vp, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.tsvpp_letterbox_area_rows.restype = i32
    pz = ctypes.POINTER(RoiSized)
    L.tsvpp_rois_sized_bytes.argtypes = [pp, ps, i32, i32]
    L.tsvpp_rois_sized_bytes.restype = ctypes.c_size_t
    L.tsvpp_convert_rois_sized.argtypes = [vp, i32, pn, i32, pz, pp, ctypes.POINTER(vp), vp]
    L.tsvpp_convert_rois_sized.restype = i32
    L.tsvpp_describe_rois_sized.argtypes = [pp, i32, pn, i32, pz, i32, ctypes.c_char_p, ctypes.c_size_t]
    L.tsvpp_describe_rois_sized.restype = i32
    L.tsvpp_convert_rois_sized_tensor.argtypes = [vp, i32, pn, i32, pz, pp, ps, ctypes.POINTER(vp), vp]
    L.tsvpp_convert_rois_sized_tensor.restype = i32
    L.tsvpp_describe_rois_sized_tensor.argtypes = [pp, ps, i32, pn, i32, pz, i32, ctypes.c_char_p, ctypes.c_size_t]
    L.tsvpp_describe_rois_sized_tensor.restype = i32
    L.tsvpp_rois_sized_tile.argtypes = [pp, i32, pn, i32, pz, i32, ctypes.c_uint, ctypes.POINTER(ctypes.c_int32)]
    L.tsvpp_rois_sized_tile.restype = i32
    pw = ctypes.POINTER(Warp)
    L.tsvpp_convert_warp.argtypes = [vp, i32, pn, i32, pw, pp, i32, i32, i32, ctypes.POINTER(vp), vp]
    L.tsvpp_convert_warp.restype = i32
    L.tsvpp_describe_warp.argtypes = [pp, i32, pn, i32, pw, i32, i32, i32, i32, ctypes.c_char_p, ctypes.c_size_t]
    L.tsvpp_describe_warp.restype = i32
    L.tsvpp_convert_warp_tensor.argtypes = [vp, i32, pn, i32, pw, pp, ps, i32, i32, i32, ctypes.POINTER(vp), vp]
    L.tsvpp_convert_warp_tensor.restype = i32
    L.tsvpp_describe_warp_tensor.argtypes = [pp, ps, i32, pn, i32, pw, i32, i32, i32, i32, ctypes.c_char_p, ctypes.c_size_t]
    L.tsvpp_describe_warp_tensor.restype = i32
    L.tsvpp_warp_rotated_box.argtypes = [ctypes.c_double] * 5 + [i32, i32, pw]
    L.tsvpp_warp_rotated_box.restype = i32
    L.tsvpp_warp_footprint.argtypes = [pw, i32, i32, i32, i32, i32, i32, ctypes.POINTER(ctypes.c_int32)]
    L.tsvpp_warp_footprint.restype = i32
    # (BICUBIC: one pair per call, spec may be None)
    L.tsvpp_convert_warp_bicubic.argtypes = L.tsvpp_convert_warp_tensor.argtypes
    L.tsvpp_convert_warp_bicubic.restype = i32
    L.tsvpp_describe_warp_bicubic.argtypes = L.tsvpp_describe_warp_tensor.argtypes
    L.tsvpp_describe_warp_bicubic.restype = i32
    L.tsvpp_warp_bicubic_footprint.argtypes = L.tsvpp_warp_footprint.argtypes
    L.tsvpp_warp_bicubic_footprint.restype = i32
    pq = ctypes.POINTER(Persp)
    L.tsvpp_convert_perspective.argtypes = [vp, i32, pn, i32, pq, pp, i32, i32, i32, ctypes.POINTER(vp), vp]
    L.tsvpp_convert_perspective.restype = i32
    L.tsvpp_describe_perspective.argtypes = [pp, i32, pn, i32, pq, i32, i32, i32, i32, ctypes.c_char_p, ctypes.c_size_t]
    L.tsvpp_describe_perspective.restype = i32
    L.tsvpp_convert_perspective_tensor.argtypes = [vp, i32, pn, i32, pq, pp, ps, i32, i32, i32, ctypes.POINTER(vp), vp]
    L.tsvpp_convert_perspective_tensor.restype = i32
    L.tsvpp_describe_perspective_tensor.argtypes = [pp, ps, i32, pn, i32, pq, i32, i32, i32, i32, ctypes.c_char_p, ctypes.c_size_t]
    L.tsvpp_describe_perspective_tensor.restype = i32
    L.tsvpp_persp_from_quad.argtypes = [ctypes.POINTER(ctypes.c_double), i32, i32, pq]
    L.tsvpp_persp_from_quad.restype = i32
    L.tsvpp_persp_footprint.argtypes = [pq, i32, i32, i32, i32, i32, i32, ctypes.POINTER(ctypes.c_int32)]
    L.tsvpp_persp_footprint.restype = i32
    L.tsvpp_convert_perspective_bicubic.argtypes = L.tsvpp_convert_perspective_tensor.argtypes
    L.tsvpp_convert_perspective_bicubic.restype = i32
    L.tsvpp_describe_perspective_bicubic.argtypes = L.tsvpp_describe_perspective_tensor.argtypes
    L.tsvpp_describe_perspective_bicubic.restype = i32
    L.tsvpp_persp_bicubic_footprint.argtypes = L.tsvpp_persp_footprint.argtypes
    L.tsvpp_persp_bicubic_footprint.restype = i32
    pm, pr, pf = ctypes.POINTER(Map), ctypes.POINTER(Remap), ctypes.POINTER(ctypes.c_float)
    L.tsvpp_convert_remap.argtypes = [vp, i32, pn, i32, pm, i32, pr, pp, i32, i32, i32, ctypes.POINTER(vp), vp]
    L.tsvpp_convert_remap.restype = i32
    L.tsvpp_describe_remap.argtypes = [pp, i32, pn, i32, pm, i32, pr, i32, i32, i32, i32, ctypes.c_char_p, ctypes.c_size_t]
    L.tsvpp_describe_remap.restype = i32
    L.tsvpp_convert_remap_tensor.argtypes = [vp, i32, pn, i32, pm, i32, pr, pp, ps, i32, i32, i32, ctypes.POINTER(vp), vp]
    L.tsvpp_convert_remap_tensor.restype = i32
    L.tsvpp_describe_remap_tensor.argtypes = [pp, ps, i32, pn, i32, pm, i32, pr, i32, i32, i32, i32, ctypes.c_char_p, ctypes.c_size_t]
    L.tsvpp_describe_remap_tensor.restype = i32
    L.tsvpp_remap_footprint.argtypes = [pf, i32, i32, i32, i32, i32, i32, i32, i32, i32, ctypes.POINTER(ctypes.c_int32)]
    L.tsvpp_remap_footprint.restype = i32
    L.tsvpp_remap_lds_need.argtypes = [pf, i32, i32, i32, i32, i32, i32]
    L.tsvpp_remap_lds_need.restype = i32
    pe, pi = ctypes.POINTER(Mesh), ctypes.POINTER(ctypes.c_int)
    L.tsvpp_convert_mesh.argtypes = [vp, i32, pn, i32, pe, i32, pr, pp, i32, i32, i32, ctypes.POINTER(vp), vp]
    L.tsvpp_convert_mesh.restype = i32
    L.tsvpp_describe_mesh.argtypes = [pp, i32, pn, i32, pe, i32, pr, i32, i32, i32, i32, ctypes.c_char_p, ctypes.c_size_t]
    L.tsvpp_describe_mesh.restype = i32
    L.tsvpp_convert_mesh_tensor.argtypes = [vp, i32, pn, i32, pe, i32, pr, pp, ps, i32, i32, i32, ctypes.POINTER(vp), vp]
    L.tsvpp_convert_mesh_tensor.restype = i32
    L.tsvpp_describe_mesh_tensor.argtypes = [pp, ps, i32, pn, i32, pe, i32, pr, i32, i32, i32, i32, ctypes.c_char_p, ctypes.c_size_t]
    L.tsvpp_describe_mesh_tensor.restype = i32
    L.tsvpp_mesh_dims.argtypes = [i32, i32, i32, i32, pi, pi]
    L.tsvpp_mesh_dims.restype = i32
    L.tsvpp_mesh_expand.argtypes = [pf, i32, i32, i32, i32, i32, pf, i32]
    L.tsvpp_mesh_expand.restype = i32
    L.tsvpp_mesh_from_map.argtypes = [pf, i32, i32, i32, i32, i32, pf, i32]
    L.tsvpp_mesh_from_map.restype = i32
    L.tsvpp_mesh_error.argtypes = [pf, i32, i32, i32, pf, i32, i32, i32, pf]
    L.tsvpp_mesh_error.restype = i32
    L.tsvpp_mesh_lds_need.argtypes = [pf, i32, i32, i32, i32, i32, i32, i32, i32]
    L.tsvpp_mesh_lds_need.restype = i32
    L.tsvpp_debug_area_tables.argtypes = [vp]
    L.tsvpp_debug_area_tables.restype = i32
    L.tsvpp_debug_last_launch.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    L.tsvpp_debug_last_launch.restype = i32
    L.tsvpp_strerror.argtypes = [i32]
    L.tsvpp_strerror.restype = ctypes.c_char_p
    L.tsvpp_version.argtypes = []
    L.tsvpp_version.restype = ctypes.c_char_p
    for f in ("tsvpp_create", "tsvpp_consumer_stream", "tsvpp_out_dims", "tsvpp_convert", "tsvpp_convert_batch",
              "tsvpp_prepare", "tsvpp_prepare_batch", "tsvpp_enable_markers", "tsvpp_get_coeffs", "tsvpp_set_coeffs", "tsvpp_area_pattern", "tsvpp_describe",
              "tsvpp_table_create", "tsvpp_table_set", "tsvpp_convert_table"):
        getattr(L, f).restype = i32
    _lib = L
    return L


def check(status):
    """The reference turns a non-zero status into std::runtime_error(std::to_string(status))
    (include/Common.h:116-123), which pybind surfaces as RuntimeError; same here, plus the text."""
    if status != 0:
        raise RuntimeError(f"{status}: {lib().tsvpp_strerror(status).decode()}")
