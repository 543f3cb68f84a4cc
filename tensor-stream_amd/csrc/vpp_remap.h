// vpp_remap.h -- launch descriptor, coordinate rules and tile footprint of the coordinate-map kernel (vpp_remap.hip), shared with the host API (tsvpp_remap.cpp:
// tsvpp_convert_remap / tsvpp_describe_remap, their tensor forms and the two host-only functions).  The tile, the staging rules, the LDS accounting and the sampler
// from the clamped coordinate on are the affine kernel's (vpp_rois.h, vpp_warp.h); what this file adds is a coordinate that is READ, not computed -- so the host
// cannot know a tile's footprint and the kernel reduces it itself.  Product code -- never includes anything from oracle/.
#pragma once
#include "vpp_warp.h"

#pragma clang fp contract(off)

namespace tsvpp {

// What differs per output.  Wave-uniform: the kernel indexes the record array with its workgroup's output and reads the fields with scalar loads out of the
// kernarg segment.  The planes are those of the WHOLE frame; the map is addressed, never copied: a replayed graph reads what the map holds then.
struct RemapRec {
    uint64_t y, uv, out, xy;   // plane addresses of the frame, output address, map address (8-byte aligned)
    int32_t pitch_y, pitch_uv;
    int32_t src_w, src_h;      // the frame
    int32_t map_pitch, pad_;   // bytes per map row (a multiple of 8, >= 8 * dst_w)
};
static_assert(sizeof(RemapRec) == 56, "RemapRec layout");

// One launch: up to TSVPP_MAX_REMAPS records (CoordLaunch, vpp_warp.h), 1.9 KiB of the kernarg segment.  lds_bytes is the launch's hint or budget: the host
// knows no footprint
using RemapLaunch = CoordLaunch<RemapRec, TSVPP_MAX_REMAPS>;
static_assert(sizeof(RemapLaunch) + 256 <= 4096, "RemapLaunch no longer fits the kernarg segment");
static_assert(coord_launch_layout<RemapLaunch, 1912, 1880>, "RemapLaunch layout");

// static LDS of the staged kernels' footprint reduction: eight extremes per wave (counts against the workgroup's LDS budget like roi_static_lds)
constexpr int REMAP_REDUCE_LDS = 2 * 8 * 4;

// THE clamp (include/tsvpp.h): every bit pattern becomes a coordinate in [-1, limit]; fmaxf first, so a NaN counts as -1
__host__ __device__ __forceinline__ float remap_clamp(float f, int limit) { return fminf(fmaxf(f, -1.0f), (float)limit); }
// THE chroma coordinate of a pair from one component of the four luma entries of its 2 x 2 block: three additions in this order, one explicit fused multiply-add
__host__ __device__ __forceinline__ float remap_chroma(float c00, float c01, float c10, float c11) {
    const float s = (c00 + c01) + (c10 + c11);
    return __builtin_fmaf(s, 0.125f, -0.25f);
}

// The extremes of the clamped coordinates of a tile's pixels and pairs: what the workgroup reduces and the host loop accumulates.  min / max of numbers (no NaN
// survives the clamp) are exact and independent of the order, so both arrive at the same eight values.
struct RemapExtremes {
    float x_lo, x_hi, y_lo, y_hi, cx_lo, cx_hi, cy_lo, cy_hi;
};
// Source span of one axis: warp_span's rule on the true extremes instead of four corners
__host__ __device__ inline void remap_span(float mn, float mx, int limit, int &lo, int &hi) {
    lo = (int)floorf(mn);
    hi = (int)floorf(mx) + 1;
    roi_clamp(lo, hi, limit);
}
// THE footprint of a tile from its extremes on a frame of w x h: host (tsvpp_remap_footprint, tsvpp_remap_lds_need) and kernel alike
__host__ __device__ inline void remap_footprint(const RemapExtremes &e, int w, int h, RoiFootprint &f) {
    remap_span(e.x_lo, e.x_hi, w, f.xlo, f.xhi);
    remap_span(e.y_lo, e.y_hi, h, f.ylo, f.yhi);
    remap_span(e.cx_lo, e.cx_hi, w >> 1, f.cxlo, f.cxhi);
    remap_span(e.cy_lo, e.cy_hi, h >> 1, f.cylo, f.cyhi);
}

// (vpp_remap.hip) launches -- or, with `dry_run`, only names -- the kernel of (out, vec, staged, border); `name` receives the name tsvpp_describe_remap reports
hipError_t launch_remap(OutKind out, bool vec, bool staged, bool border, const RemapLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                        size_t name_len, bool dry_run);
// (vpp_remap_tensor.hip) the same for the tensor instantiations: `out` is O_F32_PLANAR or O_Y800_F32, the element is L.spec.dtype's
hipError_t launch_remap_tensor(OutKind out, bool vec, bool staged, bool border, const RemapLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                               size_t name_len, bool dry_run);

} // namespace tsvpp
