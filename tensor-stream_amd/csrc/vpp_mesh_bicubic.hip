// vpp_mesh_bicubic.hip -- control-grid warps sampled BICUBIC (tsvpp_convert_mesh_bicubic without a spec, include/tsvpp.h): vpp_map_bicubic_core.h's kernel with the
// library's colour back end (EL_LIB: every flavour of tsvpp_convert_mesh).  A translation unit of its own: the library builds in parallel and no existing unit
// is recompiled to other code.
//
// Arithmetic contract as everywhere: single IEEE-754 operations, contraction off; the only fused operations are those of the coordinate (vpp_remap.h, vpp_mesh.h).
// Written for wave64 / CDNA4 only.

#include "vpp_map_bicubic_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

// (the kernel and its tag: vpp_map_bicubic_core.h; the launcher: vpp_tile_launch.h)
hipError_t launch_mesh_bicubic(OutKind out, bool vec, bool staged, bool border, const MeshLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                            size_t name_len, bool dry_run) {
    return launch_coord<MeshBicubicKernels>(out, vec, staged, border, L, grid, lds_bytes, stream, name, name_len, dry_run);
}

} // namespace tsvpp
