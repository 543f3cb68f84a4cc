// vpp_mesh_tensor.hip -- the tensor instantiations of the control-grid kernel (tsvpp_convert_mesh_tensor, include/tsvpp.h): vpp_mesh_core.h's kernel with the store
// of vpp_tensor_store.h -- (q - mean[c]) * scale[c] as fp32 (EL_F32) or as fp16 / bf16 (EL_HALF, which branches on the launch's dtype).  A translation unit of its
// own: the library builds in parallel and vpp_mesh.hip's object does not grow.  Planar RGB / BGR and Y800 only.
//
// Arithmetic contract as everywhere: single IEEE-754 operations, contraction off.  Written for wave64 / CDNA4 only.

#include "vpp_mesh_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

// (the kernel and its tag: vpp_mesh_core.h, shared with vpp_mesh.hip; the launcher: vpp_tile_launch.h)
hipError_t launch_mesh_tensor(OutKind out, bool vec, bool staged, bool border, const MeshLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                              size_t name_len, bool dry_run) {
    return launch_coord_tensor<MeshKernels>(out, vec, staged, border, L, grid, lds_bytes, stream, name, name_len, dry_run);
}

} // namespace tsvpp
