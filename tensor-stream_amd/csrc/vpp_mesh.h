// vpp_mesh.h -- launch descriptor and coordinate rule of the control-grid kernel (vpp_mesh.hip), shared with the host API (tsvpp_mesh.cpp: tsvpp_convert_mesh /
// tsvpp_describe_mesh, their tensor forms and the host-only functions).  A warp mesh is a coordinate map that is COMPUTED from four control points instead of read:
// mesh_lerp below is the whole difference, and from the coordinate it returns on everything is the dense call's (vpp_remap.h: the clamp, the chroma coordinate, the
// footprint).  Product code -- never includes anything from oracle/.
#pragma once
#include "vpp_remap.h"

#pragma clang fp contract(off)

namespace tsvpp {

// What differs per output, as RemapRec: wave-uniform, read with scalar loads out of the kernarg segment.  The mesh is addressed, never copied: a replayed graph
// reads what the mesh holds then.
struct MeshRec {
    uint64_t y, uv, out, xy;   // plane addresses of the frame, output address, mesh address (8-byte aligned)
    int32_t pitch_y, pitch_uv;
    int32_t src_w, src_h;      // the frame
    int32_t mesh_pitch;        // bytes per control row (a multiple of 8, >= 8 * cols)
    int32_t log2_cw, log2_ch;  // cell size in output pixels, 2..8 each
    int32_t pad_;
};
static_assert(sizeof(MeshRec) == 64, "MeshRec layout");

// One launch: up to TSVPP_MAX_MESHES records (CoordLaunch, vpp_warp.h), 2.2 KiB of the kernarg segment
using MeshLaunch = CoordLaunch<MeshRec, TSVPP_MAX_MESHES>;
static_assert(sizeof(MeshLaunch) + 256 <= 4096, "MeshLaunch no longer fits the kernarg segment");
static_assert(coord_launch_layout<MeshLaunch, 2168, 2136>, "MeshLaunch layout");

constexpr int MESH_LOG2_MIN = 2, MESH_LOG2_MAX = 8;

// control points per axis of an output of `n` pixels at cell size 2^l: one beyond the cell of the last pixel
__host__ __device__ __forceinline__ int mesh_points(int n, int l) { return ((n - 1) >> l) + 2; }
// 1 / 2^l, exact (l = 2..8)
__host__ __device__ __forceinline__ float mesh_inv(int l) { return __builtin_bit_cast(float, (127 - l) << 23); }
// the position of output index `k` inside its cell, as a fraction of the cell: an integer below 2^l times a power of two, exact
__host__ __device__ __forceinline__ float mesh_frac(int k, int l) { return (float)(k & ((1 << l) - 1)) * mesh_inv(l); }

// THE coordinate (include/tsvpp.h): one component of an output pixel at fraction (tx, ty) of the cell with corners A B / C D.  Three subtractions and three
// explicit fused multiply-adds, each rounded once; kernel (mesh_load, vpp_mesh_core.h) and host (tsvpp_mesh_expand) alike
__host__ __device__ __forceinline__ float mesh_lerp(float A, float B, float C, float D, float tx, float ty) {
    const float top = __builtin_fmaf(tx, B - A, A);
    const float bot = __builtin_fmaf(tx, D - C, C);
    return __builtin_fmaf(ty, bot - top, top);
}

// (vpp_mesh.hip) launches -- or, with `dry_run`, only names -- the kernel of (out, vec, staged, border); `name` receives the name tsvpp_describe_mesh reports
hipError_t launch_mesh(OutKind out, bool vec, bool staged, bool border, const MeshLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                       size_t name_len, bool dry_run);
// (vpp_mesh_tensor.hip) the same for the tensor instantiations: `out` is O_F32_PLANAR or O_Y800_F32, the element is L.spec.dtype's
hipError_t launch_mesh_tensor(OutKind out, bool vec, bool staged, bool border, const MeshLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                              size_t name_len, bool dry_run);

} // namespace tsvpp
