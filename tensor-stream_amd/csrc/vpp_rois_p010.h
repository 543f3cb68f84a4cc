// vpp_rois_p010.h -- what the P010 region-of-interest kernel (vpp_rois_p010.hip, vpp_rois_p010_tensor.hip) shares with the host API (tsvpp_rois_p010.cpp:
// tsvpp_convert_rois_p010 / tsvpp_describe_rois_p010).  The launch block is the ROI call's, RoiLaunch with its 48-byte RoiRec records (vpp_rois.h): plane addresses
// -- ADVANCED to the box origin, luma by top * pitch_y + 2 * left, chroma by (top / 2) * pitch_uv + 2 * left -- and pitches are in BYTES, the box's size in samples.
// The LDS need of a tile whose footprint is staged as raw 16-bit words is the P010 letterbox call's (p010_lds_need, vpp_letterbox_p010.h).  Product code -- never
// includes anything from oracle/.
#pragma once
#include "vpp_letterbox_p010.h"

namespace tsvpp {

static_assert(TSVPP_MAX_ROIS_P010 == TSVPP_MAX_ROIS, "the P010 entry point fills the ROI launch block");

// (vpp_rois_p010.hip) launches -- or, with `dry_run`, only names -- the kernel of (mode, out, vec, staged); mode is M_NEAREST or M_BILINEAR
hipError_t launch_rois_p010(Mode mode, OutKind out, bool vec, bool staged, const RoiLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                            size_t name_len, bool dry_run);
// (vpp_rois_p010_tensor.hip) the same for the tensor instantiations: `out` is O_F32_PLANAR or O_Y800_F32, the element is L.spec.dtype's
hipError_t launch_rois_p010_tensor(Mode mode, OutKind out, bool vec, bool staged, const RoiLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                   size_t name_len, bool dry_run);

} // namespace tsvpp
