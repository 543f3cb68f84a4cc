// vpp_map_bicubic.h -- what BICUBIC adds to the coordinate-map and the control-grid path (vpp_remap.h, vpp_mesh.h), shared by the kernels (vpp_map_bicubic_core.h)
// and the host API (tsvpp_remap.cpp, tsvpp_mesh.cpp: tsvpp_convert_remap_bicubic / tsvpp_convert_mesh_bicubic, their describe calls and the two host-only
// functions): a tile's footprint with the halo of the 4 x 4 taps.  The coordinate rules, the records and the launch blocks are the BILINEAR calls', the axis and
// the span rule are the matrix paths' BICUBIC (vpp_coord_bicubic.h); all untouched.  Product code -- never includes anything from oracle/.
#pragma once
#include "vpp_mesh.h"
#include "vpp_coord_bicubic.h"

#pragma clang fp contract(off)

namespace tsvpp {

// remap_span with the 4-tap halo: warp_cubic_span's rule -- [p(min) - 1, p(max) + 2] clamped into the plane, p the CLAMPED centre tap -- on the true extremes
// of the tile's clamped coordinates instead of four corners (its clamp is then a no-op)
__host__ __device__ inline void remap_cubic_span(float mn, float mx, int limit, int &lo, int &hi) { warp_cubic_span(mn, mx, mn, mx, limit, lo, hi); }
// THE footprint of a tile of the BICUBIC map calls from its extremes on a frame of w x h: host (tsvpp_remap_bicubic_footprint, tsvpp_remap_bicubic_lds_need)
// and kernel alike.  It contains remap_footprint's box, so an LDS hint computed for the BILINEAR call is too small here, never wrong: such tiles gather.
__host__ __device__ inline void remap_bicubic_footprint(const RemapExtremes &e, int w, int h, RoiFootprint &f) {
    remap_cubic_span(e.x_lo, e.x_hi, w, f.xlo, f.xhi);
    remap_cubic_span(e.y_lo, e.y_hi, h, f.ylo, f.yhi);
    remap_cubic_span(e.cx_lo, e.cx_hi, w >> 1, f.cxlo, f.cxhi);
    remap_cubic_span(e.cy_lo, e.cy_hi, h >> 1, f.cylo, f.cyhi);
}

// (vpp_remap_bicubic.hip, vpp_remap_bicubic_tensor.hip, vpp_mesh_bicubic.hip, vpp_mesh_bicubic_tensor.hip) the launchers, as launch_remap / launch_remap_tensor
hipError_t launch_remap_bicubic(OutKind out, bool vec, bool staged, bool border, const RemapLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                size_t name_len, bool dry_run);
hipError_t launch_remap_bicubic_tensor(OutKind out, bool vec, bool staged, bool border, const RemapLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream,
                                       char *name, size_t name_len, bool dry_run);
hipError_t launch_mesh_bicubic(OutKind out, bool vec, bool staged, bool border, const MeshLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                               size_t name_len, bool dry_run);
hipError_t launch_mesh_bicubic_tensor(OutKind out, bool vec, bool staged, bool border, const MeshLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream,
                                      char *name, size_t name_len, bool dry_run);

} // namespace tsvpp
