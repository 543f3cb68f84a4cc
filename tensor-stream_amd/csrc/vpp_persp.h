// vpp_persp.h -- launch descriptor, coordinate expression and tile footprint of the perspective-warp kernel (vpp_persp.hip), shared with the host API
// (tsvpp_persp.cpp: tsvpp_convert_perspective / tsvpp_describe_perspective and their tensor forms) and with the request rules (persp_plan, tsvpp_plan.cpp: the
// horizon rule evaluates the denominator with the expression below).  The tile, the staging rules and the LDS accounting are the ROI kernel's (vpp_rois.h), the
// sampler's axis and the span of a set of coordinates the affine warp's (vpp_warp.h); what this file adds is a source coordinate with a divide in it.  Product
// code -- never includes anything from oracle/.
#pragma once
#include "vpp_warp.h"

#pragma clang fp contract(off)

namespace tsvpp {

// The terms of one grid (luma pixels, or chroma pairs): numerators nx = a u + b v + c of both axes and the denominator nw = g u + hh v + k, the half-pixel shift
// folded into the numerators (include/tsvpp.h).  Wave-uniform in the kernel.
struct PerspGrid {
    float ax, bx, cx; // X numerator
    float ay, by, cy; // Y numerator
    float g, hh, k;   // denominator
};
static_assert(sizeof(PerspGrid) == 36, "PerspGrid layout");

// What differs per output.  Wave-uniform: the kernel indexes the record array with its workgroup's output and reads the fields with scalar loads out of the
// kernarg segment.  The planes are those of the WHOLE frame.  Both grids are stored whole: the chroma denominator's 2 g and 2 hh are exact, and a product of
// wave-uniform floats would otherwise run on the vector unit and hold two VGPRs in kernels that stand at the 128 of their launch bounds.
struct PerspRec {
    uint64_t y, uv, out;       // plane addresses of the frame, output address
    int32_t pitch_y, pitch_uv;
    int32_t src_w, src_h;      // the frame
    PerspGrid luma, chroma;    // persp_terms() of tsvpp_persp::h
};
static_assert(sizeof(PerspRec) == 112, "PerspRec layout");

// One launch: up to TSVPP_MAX_PERSP records (CoordLaunch, vpp_warp.h), 3.6 KiB of the kernarg segment
using PerspLaunch = CoordLaunch<PerspRec, TSVPP_MAX_PERSP>;
static_assert(sizeof(PerspLaunch) + 256 <= 4096, "PerspLaunch no longer fits the kernarg segment");
static_assert(coord_launch_layout<PerspLaunch, 3704, 3672>, "PerspLaunch layout");

// The terms of both grids from the homography, each one fp32 operation with one rounding (the products by 0.5 and by 2 are exact)
__host__ __device__ inline void persp_terms(const float h[9], PerspGrid &luma, PerspGrid &chroma) {
    luma.ax = h[0] - 0.5f * h[6];
    luma.bx = h[1] - 0.5f * h[7];
    luma.cx = h[2] - 0.5f * h[8];
    luma.ay = h[3] - 0.5f * h[6];
    luma.by = h[4] - 0.5f * h[7];
    luma.cy = h[5] - 0.5f * h[8];
    luma.g = h[6];
    luma.hh = h[7];
    luma.k = h[8];
    chroma.ax = h[0] - h[6];
    chroma.bx = h[1] - h[7];
    chroma.cx = h[2] * 0.5f - h[8] * 0.5f;
    chroma.ay = h[3] - h[6];
    chroma.by = h[4] - h[7];
    chroma.cy = h[5] * 0.5f - h[8] * 0.5f;
    chroma.g = 2.0f * h[6];
    chroma.hh = 2.0f * h[7];
    chroma.k = h[8];
}

// THE coordinate expression (include/tsvpp.h): numerators and denominator are the affine warp's two fused multiply-adds (warp_inner, warp_coord), then ONE
// correctly rounded reciprocal that both axes share, and one product per axis.
__host__ __device__ __forceinline__ float persp_recip(float nw) { return 1.0f / nw; }
__host__ __device__ __forceinline__ float persp_term(float u, float v, float a, float b, float c) { return warp_coord(u, a, warp_inner(v, b, c)); }

// The horizon rule's bound: below it the request has no answer (persp_plan); at or above it every reciprocal is finite, positive and at most 2^64
constexpr float PERSP_MIN_DENOMINATOR = 0x1p-64f;

// Extremes of one term over the index rectangle [j0, j1] x [i0, i1]: every operation is monotone in u and in v separately (rounding is monotone), so they are
// attained at the four corners
__host__ __device__ inline void persp_term_range(float u0, float u1, float v0, float v1, float a, float b, float c, float &mn, float &mx) {
    const float i0 = warp_inner(v0, b, c), i1 = warp_inner(v1, b, c);
    const float t00 = warp_coord(u0, a, i0), t01 = warp_coord(u1, a, i0), t10 = warp_coord(u0, a, i1), t11 = warp_coord(u1, a, i1);
    mn = fminf(fminf(t00, t01), fminf(t10, t11));
    mx = fmaxf(fmaxf(t00, t01), fmaxf(t10, t11));
}
// ... of the denominator alone: the smallest one over the rectangle (the horizon rule asks it of the whole output, per grid)
__host__ __device__ inline float persp_min_denominator(const PerspGrid &t, int j0, int j1, int i0, int i1) {
    float mn, mx;
    persp_term_range((float)j0 + 0.5f, (float)j1 + 0.5f, (float)i0 + 0.5f, (float)i1 + 0.5f, t.g, t.hh, t.k, mn, mx);
    return mn;
}

// Source span of both axes of one grid over a tile.  The quotient of two monotone functions is not monotone after rounding, so the coordinates of the corner
// pixels bound nothing here.  The interval box does: numerators and denominator each have rigorous ranges (above); the reciprocal, correctly rounded, is
// monotone, so every pixel's rw lies in [1 / nwmax, 1 / nwmin]; a correctly rounded product is monotone in each factor, so every pixel's n * rw lies between the
// least and the greatest of the four products of the ranges' ends.  Those four go into warp_span, as the four corner coordinates of an affine tile do -- and for
// an affine map (nw the same everywhere) they are exactly those.  The request rules guarantee nwmin >= PERSP_MIN_DENOMINATOR.
__host__ __device__ inline void persp_grid_span(const PerspGrid &t, int j0, int j1, int i0, int i1, int w, int h, int &xlo, int &xhi, int &ylo, int &yhi) {
    const float u0 = (float)j0 + 0.5f, u1 = (float)j1 + 0.5f, v0 = (float)i0 + 0.5f, v1 = (float)i1 + 0.5f;
    float xmn, xmx, ymn, ymx, wmn, wmx;
    persp_term_range(u0, u1, v0, v1, t.ax, t.bx, t.cx, xmn, xmx);
    persp_term_range(u0, u1, v0, v1, t.ay, t.by, t.cy, ymn, ymx);
    persp_term_range(u0, u1, v0, v1, t.g, t.hh, t.k, wmn, wmx);
    const float rlo = persp_recip(wmx), rhi = persp_recip(wmn);
    warp_span(xmn * rlo, xmn * rhi, xmx * rlo, xmx * rhi, w, xlo, xhi);
    warp_span(ymn * rlo, ymn * rhi, ymx * rlo, ymx * rhi, h, ylo, yhi);
}
// Footprint of output columns [j0, j1] / rows [i0, i1] (even first, odd last: a tile) in both planes.  Host and device alike: the host sizes the launch's LDS
// with exactly the numbers the kernel will compute.
__host__ __device__ inline void persp_footprint(const PerspRec &r, int j0, int j1, int i0, int i1, RoiFootprint &f) {
    persp_grid_span(r.luma, j0, j1, i0, i1, r.src_w, r.src_h, f.xlo, f.xhi, f.ylo, f.yhi);
    persp_grid_span(r.chroma, j0 >> 1, j1 >> 1, i0 >> 1, i1 >> 1, r.src_w >> 1, r.src_h >> 1, f.cxlo, f.cxhi, f.cylo, f.cyhi);
}

// (vpp_persp.hip) launches -- or, with `dry_run`, only names -- the kernel of (out, vec, staged, border); `name` receives the name tsvpp_describe_perspective reports
hipError_t launch_persp(OutKind out, bool vec, bool staged, bool border, const PerspLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                        size_t name_len, bool dry_run);
// (vpp_persp_tensor.hip) the same for the tensor instantiations: `out` is O_F32_PLANAR or O_Y800_F32, the element is L.spec.dtype's
hipError_t launch_persp_tensor(OutKind out, bool vec, bool staged, bool border, const PerspLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                               size_t name_len, bool dry_run);

} // namespace tsvpp
