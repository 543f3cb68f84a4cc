// vpp_coord_bicubic.h -- what BICUBIC through a coordinate adds to the affine and the perspective path (vpp_warp.h, vpp_persp.h), shared by the kernels
// (vpp_coord_bicubic_core.h) and the host API (tsvpp_warp.cpp, tsvpp_persp.cpp: tsvpp_convert_warp_bicubic / tsvpp_convert_perspective_bicubic and their describe
// calls): the axis of a 4-tap sample and a tile's footprint with the halo of the 4 x 4 taps.  The coordinate, the records and the launch blocks are the BILINEAR
// calls', untouched.  Product code -- never includes anything from oracle/.
#pragma once
#include "vpp_persp.h"

#pragma clang fp contract(off)

namespace tsvpp {

// Centre tap and weight of one axis: bicubic_axis's tail (vpp_axis.h) on a coordinate `f` that need not lie in the frame.  `f` is clamped into [-1, limit] before
// it becomes an integer, as warp_axis does and for its reason; f - floor(f) is exact in fp32.  The taps follow from p by bicubic_offsets (vpp_device.h).
__host__ __device__ __forceinline__ void warp_cubic_axis(float f, int limit, int &p, float &w) {
    f = fminf(fmaxf(f, -1.0f), (float)limit);
    const float pf = floorf(f);
    p = (int)pf;
    w = f - pf;
    if (p < 0) { p = 0; w = 0.f; }
    if (p > limit - 1) { p = limit - 1; w = 0.f; }
}

// warp_span with the 4-tap halo: every tap lies in [p - 1, p + 2] within the frame and the centre tap p is monotone in f, so [p(min) - 1, p(max) + 2], clamped
// into the frame, holds every tap of every sample whose coordinate lies between the four values.  p is the CLAMPED floor: a sample beyond the frame has weight 0
// and centre tap 0 or limit - 1, and its other taps -- multiplied by coefficients that are exactly zero, but fetched -- lie around that tap, not around floor(f).
__host__ __device__ inline void warp_cubic_span(float f00, float f01, float f10, float f11, int limit, int &lo, int &hi) {
    float mn = fminf(fminf(f00, f01), fminf(f10, f11)), mx = fmaxf(fmaxf(f00, f01), fmaxf(f10, f11));
    mn = fminf(fmaxf(mn, -1.0f), (float)limit);
    mx = fminf(fmaxf(mx, -1.0f), (float)limit);
    const int pmn = (int)floorf(mn), pmx = (int)floorf(mx);
    lo = (pmn < 0 ? 0 : pmn > limit - 1 ? limit - 1 : pmn) - 1;
    hi = (pmx < 0 ? 0 : pmx > limit - 1 ? limit - 1 : pmx) + 2;
    roi_clamp(lo, hi, limit);
}

// warp_grid_span / warp_footprint (vpp_warp.h) with that span: the corner coordinates are the affine call's
__host__ __device__ inline void warp_cubic_grid_span(const WarpRec &r, float tx, float ty, int j0, int j1, int i0, int i1, int w, int h, int &xlo, int &xhi, int &ylo, int &yhi) {
    const float u0 = (float)j0 + 0.5f, u1 = (float)j1 + 0.5f, v0 = (float)i0 + 0.5f, v1 = (float)i1 + 0.5f;
    const float ax0 = warp_inner(v0, r.m1, tx), ax1 = warp_inner(v1, r.m1, tx), ay0 = warp_inner(v0, r.m4, ty), ay1 = warp_inner(v1, r.m4, ty);
    warp_cubic_span(warp_coord(u0, r.m0, ax0), warp_coord(u1, r.m0, ax0), warp_coord(u0, r.m0, ax1), warp_coord(u1, r.m0, ax1), w, xlo, xhi);
    warp_cubic_span(warp_coord(u0, r.m3, ay0), warp_coord(u1, r.m3, ay0), warp_coord(u0, r.m3, ay1), warp_coord(u1, r.m3, ay1), h, ylo, yhi);
}
__host__ __device__ inline void warp_bicubic_footprint(const WarpRec &r, int j0, int j1, int i0, int i1, RoiFootprint &f) {
    warp_cubic_grid_span(r, r.tx, r.ty, j0, j1, i0, i1, r.src_w, r.src_h, f.xlo, f.xhi, f.ylo, f.yhi);
    warp_cubic_grid_span(r, r.ctx, r.cty, j0 >> 1, j1 >> 1, i0 >> 1, i1 >> 1, r.src_w >> 1, r.src_h >> 1, f.cxlo, f.cxhi, f.cylo, f.cyhi);
}

// persp_grid_span / persp_footprint (vpp_persp.h) with that span: the interval box is the perspective call's
__host__ __device__ inline void persp_cubic_grid_span(const PerspGrid &t, int j0, int j1, int i0, int i1, int w, int h, int &xlo, int &xhi, int &ylo, int &yhi) {
    const float u0 = (float)j0 + 0.5f, u1 = (float)j1 + 0.5f, v0 = (float)i0 + 0.5f, v1 = (float)i1 + 0.5f;
    float xmn, xmx, ymn, ymx, wmn, wmx;
    persp_term_range(u0, u1, v0, v1, t.ax, t.bx, t.cx, xmn, xmx);
    persp_term_range(u0, u1, v0, v1, t.ay, t.by, t.cy, ymn, ymx);
    persp_term_range(u0, u1, v0, v1, t.g, t.hh, t.k, wmn, wmx);
    const float rlo = persp_recip(wmx), rhi = persp_recip(wmn);
    warp_cubic_span(xmn * rlo, xmn * rhi, xmx * rlo, xmx * rhi, w, xlo, xhi);
    warp_cubic_span(ymn * rlo, ymn * rhi, ymx * rlo, ymx * rhi, h, ylo, yhi);
}
__host__ __device__ inline void persp_bicubic_footprint(const PerspRec &r, int j0, int j1, int i0, int i1, RoiFootprint &f) {
    persp_cubic_grid_span(r.luma, j0, j1, i0, i1, r.src_w, r.src_h, f.xlo, f.xhi, f.ylo, f.yhi);
    persp_cubic_grid_span(r.chroma, j0 >> 1, j1 >> 1, i0 >> 1, i1 >> 1, r.src_w >> 1, r.src_h >> 1, f.cxlo, f.cxhi, f.cylo, f.cyhi);
}

// (vpp_warp_bicubic.hip, vpp_warp_bicubic_tensor.hip, vpp_persp_bicubic.hip, vpp_persp_bicubic_tensor.hip) the launchers, as launch_warp / launch_warp_tensor
hipError_t launch_warp_bicubic(OutKind out, bool vec, bool staged, bool border, const WarpLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                               size_t name_len, bool dry_run);
hipError_t launch_warp_bicubic_tensor(OutKind out, bool vec, bool staged, bool border, const WarpLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream,
                                      char *name, size_t name_len, bool dry_run);
hipError_t launch_persp_bicubic(OutKind out, bool vec, bool staged, bool border, const PerspLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                size_t name_len, bool dry_run);
hipError_t launch_persp_bicubic_tensor(OutKind out, bool vec, bool staged, bool border, const PerspLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream,
                                       char *name, size_t name_len, bool dry_run);

} // namespace tsvpp
