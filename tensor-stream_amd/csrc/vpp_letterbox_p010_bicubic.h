// vpp_letterbox_p010_bicubic.h -- what the P010 BICUBIC letterbox kernel (vpp_letterbox_p010_bicubic.hip, vpp_letterbox_p010_bicubic_tensor.hip) shares with the
// host API (tsvpp_letterbox_p010_bicubic.cpp: tsvpp_convert_letterbox_p010_bicubic / tsvpp_describe_letterbox_p010_bicubic).  The launch block is the P010
// letterbox call's LbLaunch (byte addresses and pitches, sizes in samples, pad 0..1023; xr / yr are not read: N and n suffice) with the walk's three numbers
// behind it.  Product code -- never includes anything from oracle/.
#pragma once
#include "vpp_cubic_p010.h"
#include "vpp_letterbox.h"

namespace tsvpp {

struct LbCubicLaunch : LbLaunch {
    int32_t band;     // source rows per band, 1 .. BOX_BAND_MAX_ROWS
    int32_t band_cpr; // 16-byte chunks per staged row the band buffers are sized for: the widest footprint row of the launch's tile parts, either plane
    int32_t hrows;    // rows of Hbuf: the tallest footprint of the launch's tile parts, either plane
};
static_assert(sizeof(LbCubicLaunch) + 256 <= 4096, "LbCubicLaunch no longer fits the kernarg segment");

// (vpp_letterbox_p010_bicubic.hip) launches -- or, with `dry_run`, only names -- the kernel of (out, vec)
hipError_t launch_letterbox_p010_bicubic(OutKind out, bool vec, const LbCubicLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                         size_t name_len, bool dry_run);
// (vpp_letterbox_p010_bicubic_tensor.hip) the same for the tensor instantiations: `out` is O_F32_PLANAR or O_Y800_F32, the element is L.spec.dtype's
hipError_t launch_letterbox_p010_bicubic_tensor(OutKind out, bool vec, const LbCubicLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                                size_t name_len, bool dry_run);

} // namespace tsvpp
