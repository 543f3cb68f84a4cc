// vpp_persp_bicubic.hip -- homography-warped outputs sampled BICUBIC (tsvpp_convert_perspective_bicubic without a spec, include/tsvpp.h): vpp_coord_bicubic_core.h's kernel
// with the library's colour back end (EL_LIB: every flavour of tsvpp_convert_perspective).  A translation unit of its own: the library builds in parallel and no existing unit is recompiled to other code.
//
// Arithmetic contract as everywhere: single IEEE-754 operations, contraction off; the only fused operations are those of the coordinate (vpp_warp.h, vpp_persp.h).
// Written for wave64 / CDNA4 only.

#include "vpp_coord_bicubic_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

// (the kernel and its tag: vpp_coord_bicubic_core.h; the launcher: vpp_tile_launch.h)
hipError_t launch_persp_bicubic(OutKind out, bool vec, bool staged, bool border, const PerspLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                size_t name_len, bool dry_run) {
    return launch_coord<PerspBicubicKernels>(out, vec, staged, border, L, grid, lds_bytes, stream, name, name_len, dry_run);
}

} // namespace tsvpp
