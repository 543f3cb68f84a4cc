// vpp_rois_p010_bicubic.h -- what the P010 BICUBIC region-of-interest kernel (vpp_rois_p010_bicubic.hip, vpp_rois_p010_bicubic_tensor.hip) shares with the host
// API (tsvpp_rois_p010_bicubic.cpp: tsvpp_convert_rois_p010_bicubic / tsvpp_describe_rois_p010_bicubic).  The launch block is the P010 ROI call's RoiLaunch (plane
// addresses advanced to the box origin, pitches in BYTES, the box's size in samples; xr / yr are not read: N and n suffice) with the walk's three numbers behind
// it.  Product code -- never includes anything from oracle/.
#pragma once
#include "vpp_cubic_p010.h"
#include "vpp_rois_p010.h"

namespace tsvpp {

struct RoiCubicLaunch : RoiLaunch {
    int32_t band;     // source rows per band, 1 .. BOX_BAND_MAX_ROWS
    int32_t band_cpr; // 16-byte chunks per staged row the band buffers are sized for: the widest footprint row of the launch's tiles, either plane
    int32_t hrows;    // rows of Hbuf: the tallest footprint of the launch's tiles, either plane
};
static_assert(sizeof(RoiCubicLaunch) + 256 <= 4096, "RoiCubicLaunch no longer fits the kernarg segment");

// (vpp_rois_p010_bicubic.hip) launches -- or, with `dry_run`, only names -- the kernel of (out, vec)
hipError_t launch_rois_p010_bicubic(OutKind out, bool vec, const RoiCubicLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name, size_t name_len,
                                    bool dry_run);
// (vpp_rois_p010_bicubic_tensor.hip) the same for the tensor instantiations: `out` is O_F32_PLANAR or O_Y800_F32, the element is L.spec.dtype's
hipError_t launch_rois_p010_bicubic_tensor(OutKind out, bool vec, const RoiCubicLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                           size_t name_len, bool dry_run);

} // namespace tsvpp
