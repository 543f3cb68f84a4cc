// vpp_warp.h -- launch descriptor, coordinate expression and tile footprint of the affine-warp kernel (vpp_warp.hip), shared with the host API (tsvpp_warp.cpp:
// tsvpp_convert_warp / tsvpp_describe_warp and their tensor forms).  The tile, the staging rules and the LDS accounting are the ROI kernel's (vpp_rois.h); what this
// file adds is a source coordinate that depends on BOTH output indices.  Product code -- never includes anything from oracle/.
#pragma once
#include <cstddef>

#include "vpp_rois.h"

#pragma clang fp contract(off)

namespace tsvpp {

// What differs per warp.  Wave-uniform: the kernel indexes the record array with its workgroup's warp and reads the fields with scalar loads out of the kernarg
// segment.  The planes are those of the WHOLE frame: the matrix addresses luma pixels of the frame.
struct WarpRec {
    uint64_t y, uv, out;       // plane addresses of the frame, output address
    int32_t pitch_y, pitch_uv;
    int32_t src_w, src_h;      // the frame
    float m0, m1, m3, m4;      // the linear part of tsvpp_warp::m (output -> source)
    float tx, ty;              // m2 - 0.5f, m5 - 0.5f: the luma translations, rounded once on the host
    float ctx, cty;            // m2 * 0.5f - 0.5f, m5 * 0.5f - 0.5f: the chroma grid's (the product is exact)
};
static_assert(sizeof(WarpRec) == 72, "WarpRec layout");

// One launch of a coordinate path -- affine warp, perspective (vpp_persp.h), coordinate map (vpp_remap.h), control grid (vpp_mesh.h): up to N records of the
// path's own type, by value in the kernarg segment (HIP's hidden arguments take up to 256 bytes of the segment's 4 KiB).  The paths differ in the record alone.
template <class REC, int N> struct CoordLaunch {
    int32_t dst_w, dst_h;
    int32_t swap_rb, color_g;
    tsvpp_coeffs k;
    int32_t tiles_x, tiles_y, n;             // n: the records in use
    int32_t nt_stores, last_col0, u8_xchg;   // as LaunchDesc's
    int32_t lds_bytes;                       // dynamic LDS of the launch's staged footprints: a tile whose footprint needs more gathers from global memory
    float border_y, border_u, border_v;      // the constant-border kernels' sample, integer-valued (0..255): what the sampler would hand the colour back end
    REC r[N];
    tsvpp_tensor_spec spec;                  // the tensor instantiations' dtype, mean[3], scale[3], once per launch (vpp_tensor_store.h); behind the records, as RoiLaunch's
};
// (the layout every path's block has had since it was written: size, offset of the records, offset of the spec)
template <class L, size_t SIZE, size_t SPEC> constexpr bool coord_launch_layout = sizeof(L) == SIZE && offsetof(L, r) == 88 && offsetof(L, spec) == SPEC;

using WarpLaunch = CoordLaunch<WarpRec, TSVPP_MAX_WARPS>; // 2.4 KiB
static_assert(sizeof(WarpLaunch) + 256 <= 4096, "WarpLaunch no longer fits the kernarg segment");
static_assert(coord_launch_layout<WarpLaunch, 2424, 2392>, "WarpLaunch layout");

// The translations of a record from the matrix, each one fp32 operation (the multiplication by 0.5 is exact, so the chroma pair is rounded once as well)
__host__ __device__ inline void warp_translations(float m2, float m5, WarpRec &r) {
    r.tx = m2 - 0.5f;
    r.ty = m5 - 0.5f;
    r.ctx = m2 * 0.5f - 0.5f;
    r.cty = m5 * 0.5f - 0.5f;
}

// THE coordinate expression (include/tsvpp.h): u, v = the output pixel's centre (column + 0.5f, row + 0.5f), a / b / t = one row of the matrix.  Two explicit
// fused multiply-adds, each rounded once.  The inner one does not depend on the column: the kernel evaluates it once per row of a thread tile.
__host__ __device__ __forceinline__ float warp_inner(float v, float b, float t) { return __builtin_fmaf(v, b, t); }
__host__ __device__ __forceinline__ float warp_coord(float u, float a, float inner) { return __builtin_fmaf(u, a, inner); }

// First tap, second tap and weight of one axis: bilinear_axis's tail (vpp_axis.h) on a coordinate `f` that need not lie in the frame.  `f` is clamped into
// [-1, limit] before it becomes an integer -- no result changes (below 0 and above limit - 1 the tap is the edge pixel with weight 0 either way), and no tap index
// can leave the frame whatever the matrix.  The second tap is p + 1 where p + 1 < limit, else p; where the weight was forced to 0 at the low edge it is p as well
// (the zero multiplies it: any finite value gives the same bits), so both taps lie inside warp_span's box.
__host__ __device__ __forceinline__ void warp_axis(float f, int limit, int &p, int &p2, float &w) {
    f = fminf(fmaxf(f, -1.0f), (float)limit);
    const float pf = floorf(f);
    const int p0 = (int)pf;
    w = f - pf;
    p = p0;
    if (p0 < 0) { p = 0; w = 0.f; }
    if (p0 > limit - 1) { p = limit - 1; w = 0.f; }
    p2 = p0 + 1 < limit ? p0 + 1 : limit - 1;
}
// ... and whether a constant border replaces the sample: the position lies outside the frame [0, limit) (f is the position minus one half)
__host__ __device__ __forceinline__ bool warp_outside(float f, int limit) { return f < -0.5f || f >= (float)limit - 0.5f; }

// Source span of one axis over a tile: every operation of the coordinate is monotone in u and in v separately (rounding is monotone), so over the tile's index
// rectangle its extremes are attained at the four corner pixels.  [lo, hi] = floor of the minimum .. floor of the maximum + 1, clamped into the frame.
__host__ __device__ inline void warp_span(float f00, float f01, float f10, float f11, int limit, int &lo, int &hi) {
    float mn = fminf(fminf(f00, f01), fminf(f10, f11)), mx = fmaxf(fmaxf(f00, f01), fmaxf(f10, f11));
    mn = fminf(fmaxf(mn, -1.0f), (float)limit);
    mx = fminf(fmaxf(mx, -1.0f), (float)limit);
    lo = (int)floorf(mn);
    hi = (int)floorf(mx) + 1;
    roi_clamp(lo, hi, limit);
}
// ... of both axes of one grid (luma: the tile's pixels, the luma translations and the frame's size; chroma: its pairs, the chroma translations, half the size)
__host__ __device__ inline void warp_grid_span(const WarpRec &r, float tx, float ty, int j0, int j1, int i0, int i1, int w, int h, int &xlo, int &xhi, int &ylo, int &yhi) {
    const float u0 = (float)j0 + 0.5f, u1 = (float)j1 + 0.5f, v0 = (float)i0 + 0.5f, v1 = (float)i1 + 0.5f;
    const float ax0 = warp_inner(v0, r.m1, tx), ax1 = warp_inner(v1, r.m1, tx), ay0 = warp_inner(v0, r.m4, ty), ay1 = warp_inner(v1, r.m4, ty);
    warp_span(warp_coord(u0, r.m0, ax0), warp_coord(u1, r.m0, ax0), warp_coord(u0, r.m0, ax1), warp_coord(u1, r.m0, ax1), w, xlo, xhi);
    warp_span(warp_coord(u0, r.m3, ay0), warp_coord(u1, r.m3, ay0), warp_coord(u0, r.m3, ay1), warp_coord(u1, r.m3, ay1), h, ylo, yhi);
}
// Footprint of output columns [j0, j1] / rows [i0, i1] (even first, odd last: a tile) in both planes: the source bounding box of the tile.  Host and device alike:
// the host sizes the launch's LDS with exactly the numbers the kernel will compute.  A tile wholly outside the frame has a one-pixel footprint.
__host__ __device__ inline void warp_footprint(const WarpRec &r, int j0, int j1, int i0, int i1, RoiFootprint &f) {
    warp_grid_span(r, r.tx, r.ty, j0, j1, i0, i1, r.src_w, r.src_h, f.xlo, f.xhi, f.ylo, f.yhi);
    warp_grid_span(r, r.ctx, r.cty, j0 >> 1, j1 >> 1, i0 >> 1, i1 >> 1, r.src_w >> 1, r.src_h >> 1, f.cxlo, f.cxhi, f.cylo, f.cyhi);
}

// (vpp_warp.hip) launches -- or, with `dry_run`, only names -- the kernel of (out, vec, staged, border); `name` receives the name tsvpp_describe_warp reports
hipError_t launch_warp(OutKind out, bool vec, bool staged, bool border, const WarpLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                       size_t name_len, bool dry_run);
// (vpp_warp_tensor.hip) the same for the tensor instantiations: `out` is O_F32_PLANAR or O_Y800_F32, the element is L.spec.dtype's
hipError_t launch_warp_tensor(OutKind out, bool vec, bool staged, bool border, const WarpLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                              size_t name_len, bool dry_run);

} // namespace tsvpp
