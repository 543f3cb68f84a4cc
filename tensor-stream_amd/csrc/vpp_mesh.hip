// vpp_mesh.hip -- sparse control-grid warps: every output samples its frame BILINEAR where a device-resident warp mesh says, in one launch (tsvpp_convert_mesh,
// include/tsvpp.h).
//
// A mesh holds one (x, y) control point per 2^log2_cw x 2^log2_ch output pixels; the coordinate of an output pixel is the bilinear interpolation of the four
// control points of its cell -- three subtractions and three fused multiply-adds per component (mesh_lerp, vpp_mesh.h), a contract, so that the kernel is the
// coordinate-map kernel (vpp_remap.hip) on the expanded map, bit for bit, without that map ever existing: at 16 x 16 the mesh of a 1080p output is 67 KB where
// the map is 16.6 MB, the largest thing the dense kernel reads.
//
// Output side, records (64 bytes, wave-uniform, scalar loads out of the kernarg segment), footprint reduction, staging or gathering, sampler and colour back end
// are the dense kernel's own functions (vpp_remap_core.h); only the source of the coordinate differs (mesh_load, vpp_mesh_core.h).  The footprint is still reduced
// from the tile's own clamped coordinates, not bounded from the control points: with roundings in the interpolation such a bound would need a proof, and the
// reduction makes the staged / gathered decision exactly the dense call's on E(mesh).
//
// Arithmetic contract as everywhere: single IEEE-754 operations, contraction off; the only fused operations are mesh_lerp's, the chroma coordinate's (vpp_remap.h)
// and bilerp's.  Written for wave64 / CDNA4 only.

#include "vpp_mesh_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

// (the kernel and its tag: vpp_mesh_core.h, shared with vpp_mesh_tensor.hip; the launcher: vpp_tile_launch.h)
hipError_t launch_mesh(OutKind out, bool vec, bool staged, bool border, const MeshLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                       size_t name_len, bool dry_run) {
    return launch_coord<MeshKernels>(out, vec, staged, border, L, grid, lds_bytes, stream, name, name_len, dry_run);
}

} // namespace tsvpp
