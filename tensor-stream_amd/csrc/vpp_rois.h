// vpp_rois.h -- launch descriptor and tile geometry of the region-of-interest kernel (vpp_rois.hip), shared with the host API
// (tsvpp_rois.cpp: tsvpp_convert_rois / tsvpp_describe_rois and their AREA counterparts, kernel vpp_rois_area.hip).  Product code -- never includes anything
// from oracle/.
#pragma once
#include <float.h>

#include "vpp_kernels.h"
#include "vpp_axis.h"

#pragma clang fp contract(off)

namespace tsvpp {

// Workgroup of the ROI kernel: ROI_TX x ROI_TY thread tiles of 4 x 2 output pixels = a 32 x 32 pixel tile, two waves.  Boxes are small (NN-input sizes: 112 / 224 /
// 256 squared), many, and their ratios differ: 32 columns divide 224 and 256 exactly, a 32 x 32 tile at a ratio of 4.6 (a 512-pixel box to 112) still taps
// only 164 x 148 luma bytes + half as many chroma bytes = 36 KiB, inside the 40 KiB budget that keeps four workgroups on a CU.
constexpr int ROI_TX = 8, ROI_TY = 16, ROI_TX_SHIFT = 3;
constexpr int ROI_TILE_W = ROI_TX * 4, ROI_TILE_H = ROI_TY * 2, ROI_THREADS = ROI_TX * ROI_TY;

// What differs per box.  Wave-uniform: the kernel indexes the record array with its workgroup's box and reads the fields with scalar loads out of the kernarg segment.
struct RoiRec {
    uint64_t y, uv, out;       // plane addresses ADVANCED to the box origin (luma: top * pitch_y + left; chroma: (top / 2) * pitch_uv + left), output address
    int32_t pitch_y, pitch_uv; // of the box's frame
    int32_t src_w, src_h;      // the box
    float xr, yr;              // (float)src_w / dst_w, (float)src_h / dst_h   (reference src/Resize.cu:418-419)
};
static_assert(sizeof(RoiRec) == 48, "RoiRec layout");

// One launch: up to TSVPP_MAX_ROIS boxes, by value in the kernarg segment (3.1 KiB; HIP's hidden arguments take up to 256 bytes of the segment's 4 KiB).
struct RoiLaunch {
    int32_t dst_w, dst_h;
    int32_t swap_rb, color_g;
    tsvpp_coeffs k;
    int32_t tiles_x, tiles_y, n_rois;
    int32_t nt_stores, last_col0, u8_xchg; // as LaunchDesc's
    int32_t lds_bytes;                     // dynamic LDS of the launch's staged footprints: a tile whose footprint needs more gathers from global memory
    int32_t area_lds;                      // vpp_rois_area.hip: bytes of the weight rows in front of the staged footprint (a multiple of 16); 0 in vpp_rois.hip
    RoiRec r[TSVPP_MAX_ROIS];
    tsvpp_tensor_spec spec;                // the tensor instantiations' dtype, mean[3], scale[3], once per launch (vpp_tensor_store.h); behind the records: every offset the
                                           // other instantiations read is what it was
};
static_assert(sizeof(RoiLaunch) + 256 <= 4096, "RoiLaunch no longer fits the kernarg segment");
static_assert(TSVPP_MAX_ROIS_AREA <= TSVPP_MAX_ROIS, "the AREA entry point fills the same launch block");

// ---- AREA for boxes (tsvpp_convert_rois_area) ---------------------------------------------------------------------------------------------------------
// Per box as make_plan decides per request (reference src/Resize.cu:435): both ratios above 1 run the weighted box, anything else the 2x2 blend.
__host__ __device__ inline int roi_area_mode(float xr, float yr) { return (xr > 1.0f && yr > 1.0f) ? M_AREA_DOWN : M_AREA_UP; }
// taps of one axis of the down-scale: ceil(scale), as build_area_rows (tsvpp_area.cpp)
__host__ __device__ inline int roi_area_taps(float scale) { return (int)ceilf(scale); }
constexpr int ROI_AREA_MAX_TAPS = 40;    // per axis; above it TSVPP_UNSUPPORTED (a 1920-wide frame to 112 columns has 18, 1080 rows to 30 have 36)
constexpr int ROI_AREA_MAX_DST = 65536;  // kMaxPatternRows (tsvpp_area.cpp): the generator below never runs further than the output is wide / high
// Weight rows a tile keeps in LDS per axis: its 32 luma indices, then the (at most) 17 chroma indices [first >> 1, last >> 1]; a row is `taps` floats at a stride
// of taps | 1 (odd: the eight columns of a wave's lanes, 4 rows apart, fall into eight different banks).  Behind the rows of both axes: one RoiAreaRow record per
// row (+ one slot per axis that takes the stores of indices outside both ranges), which the chain lanes write and all lanes expand into the rows.
static_assert(ROI_TILE_W == ROI_TILE_H, "one row count serves both axes");
constexpr int ROI_AREA_ROWS = ROI_TILE_W + ROI_TILE_W / 2 + 1;
__host__ __device__ inline int roi_area_stride(int taps) { return taps | 1; }
__host__ __device__ inline int roi_area_rows_floats(int taps_x, int taps_y) { return ROI_AREA_ROWS * (roi_area_stride(taps_x) + roi_area_stride(taps_y)); }
__host__ __device__ inline int roi_area_lds(int taps_x, int taps_y) { return (4 * (roi_area_rows_floats(taps_x, taps_y) + 2 * 3 * (ROI_AREA_ROWS + 1)) + 15) & ~15; }

// The weight rows of the AREA down-scale, one output index at a time: the float operations of build_area_rows (tsvpp_area.cpp; reference generateResizePattern,
// src/Resize.cu:359-386) in its order, as a generator that needs no table.  build_area_rows emits rows until `(float)k * scale` has no fraction and the kernels
// read row j % rows; here the same test, made after every row, wraps the pattern index to 0 and clears the carry -- which is rows[j % rows] without knowing
// `rows`.  A row whose last fraction is <= FLT_EPSILON leaves the carry as it was, as there.  Not a closed form: `scale - carry` rounds, so the carry of index
// j depends on every row before it.  What IS collapsed is build_area_rows' loop `while (left - 1 > 0) left = left - 1`: left < 2^6 and every difference is a
// multiple of ulp(left) below left, so each of those subtractions is exact and m of them are `left - m`, m = max(ceil(left) - 1, 0), exact as well -- the step
// has no loop and no branch (a first version with the loop and per-entry stores ran ~330 ns per index on one lane, this one ~75 ns: profiles/rois_area_ab.txt, both variants).
// tests/test_rois_area_cpu.py pins the result against build_area_rows' own table, bit for bit.
struct RoiAreaGen {
    int k = 0;          // index inside the pattern
    float carry = 0.0f; // part of the next source pixel the previous row has consumed
};
// One row, unexpanded: [lead, if != 0] [1.0 x ones] [tail, if > FLT_EPSILON] [0 ...], cut or padded to taps entries
struct RoiAreaRow {
    float lead;
    int ones;
    float tail;
};
// entry e of the row
__host__ __device__ __forceinline__ float roi_area_weight(const RoiAreaRow &r, int e) {
    const int n = r.lead != 0.0f ? 1 : 0;
    if (e < n) return r.lead;
    if (e < n + r.ones) return 1.0f;
    return (e == n + r.ones && r.tail > FLT_EPSILON) ? r.tail : 0.0f;
}
// Row of the generator's current index; steps to the next index.
__host__ __device__ __forceinline__ RoiAreaRow roi_area_step(float scale, RoiAreaGen &g) {
    RoiAreaRow r;
    r.lead = g.carry;
    float left = scale - g.carry; // (carry == 0, where build_area_rows does not subtract: scale - 0 is scale)
    const float m = fmaxf(ceilf(left) - 1.0f, 0.0f);
    left = left - m;
    r.ones = (int)m;
    r.tail = left;
    g.carry = left > FLT_EPSILON ? 1.0f - left : g.carry;
    g.k++;
    const float pos = (float)g.k * scale;
    const bool more = pos - (float)(int)pos > FLT_EPSILON; // build_area_rows stops where this fails: the pattern has closed
    g.k = more ? g.k : 0;
    g.carry = more ? g.carry : 0.0f;
    return r;
}

// Source footprint of output indices [o0, o1] along one axis: first and last source sample any of them taps -- axis_span (vpp_device.h) with the mode as a
// run-time value, for host and device alike (the host sizes the launch's LDS with exactly the numbers the kernel will compute).
__host__ __device__ inline void roi_axis_span(int mode, int o0, int o1, float ratio, int limit, int &lo, int &hi) {
    if (mode == M_NEAREST) {
        lo = (int)(ratio * (float)o0);
        hi = (int)(ratio * (float)o1);
    } else if (mode == M_BILINEAR) {
        float w;
        bilinear_axis(o0, ratio, limit, lo, w);
        bilinear_axis(o1, ratio, limit, hi, w);
        hi += 1;
    } else if (mode == M_BICUBIC) {
        double w;
        bicubic_axis(o0, ratio, limit, lo, w);
        bicubic_axis(o1, ratio, limit, hi, w);
        lo -= 1;
        hi += 2;
    } else if (mode == M_AREA_UP) {
        float w;
        areaup_axis(o0, ratio, lo, w);
        areaup_axis(o1, ratio, hi, w);
        hi += 1;
    } else { // M_AREA_DOWN
        lo = (int)(ratio * (float)o0);
        hi = (int)(ratio * (float)o1) + roi_area_taps(ratio) - 1;
    }
}

// Footprint of the tile that starts at output (i_first, j_first) in both planes, as tile_footprint (vpp_device.h) computes it: luma columns / rows, chroma
// PAIR columns / rows (the same formulas on the chroma grid's own indices), clamped into the box.
struct RoiFootprint {
    int xlo, xhi, ylo, yhi, cxlo, cxhi, cylo, cyhi;
};
__host__ __device__ inline void roi_clamp(int &lo, int &hi, int limit) {
    lo = lo < 0 ? 0 : lo;
    hi = hi > limit - 1 ? limit - 1 : hi;
    if (lo > hi) lo = hi; // (never for a valid request)
}
// last output column / row of the tile that starts at `first`
__host__ __device__ inline int tile_last(int first, int tile, int dst) { return (first + tile < dst ? first + tile : dst) - 1; }
// Source footprint of output columns [a0, a1] / rows [b0, b1] of an item in both planes.  The ROI kernels hand in their tile (first .. tile_last), the letterbox
// kernel the part of its tile inside the rectangle (tile_inner_range), in the rectangle's own indices: a run that need not start at a tile's first index nor be a
// tile long.  Host and device alike: the host sizes the launch's LDS with exactly the numbers the kernel will compute.
__host__ __device__ inline void tile_span_x(int mode, int a0, int a1, int src_w, float xr, RoiFootprint &f) {
    roi_axis_span(mode, a0, a1, xr, src_w, f.xlo, f.xhi);
    roi_clamp(f.xlo, f.xhi, src_w);
    roi_axis_span(mode, a0 >> 1, a1 >> 1, xr, src_w, f.cxlo, f.cxhi);
    roi_clamp(f.cxlo, f.cxhi, src_w >> 1);
}
__host__ __device__ inline void tile_span_y(int mode, int b0, int b1, int src_h, float yr, RoiFootprint &f) {
    roi_axis_span(mode, b0, b1, yr, src_h, f.ylo, f.yhi);
    roi_clamp(f.ylo, f.yhi, src_h);
    roi_axis_span(mode, b0 >> 1, b1 >> 1, yr, src_h, f.cylo, f.cyhi);
    roi_clamp(f.cylo, f.cyhi, src_h >> 1);
}
// The part of output indices [first, last] of one axis that lies inside the rectangle [origin, origin + size) (vpp_letterbox.h), as indices of the rectangle's
// own grid: [lo, hi], empty (lo > hi) where the tile does not touch the rectangle.  `first`, `origin` and `size` are even and `last` is odd, so lo is even, hi is
// odd and the chroma pairs of the part are [lo >> 1, hi >> 1].
__host__ __device__ inline void tile_inner_range(int first, int last, int origin, int size, int &lo, int &hi) {
    lo = (first > origin ? first : origin) - origin;
    hi = (last < origin + size - 1 ? last : origin + size - 1) - origin;
}
// 16-byte chunks of one staged row that holds `span` bytes at any misalignment (0..15) of its first byte
__host__ __device__ inline int roi_chunks(int span) { return ((span + 14) >> 4) + 1; }
// LDS bytes of a staged tile: luma rows, then chroma rows
__host__ __device__ inline int roi_lds_need(const RoiFootprint &f, bool luma_only) {
    const int ny = f.yhi - f.ylo + 1, nuv = luma_only ? 0 : f.cyhi - f.cylo + 1;
    return 16 * (ny * roi_chunks(f.xhi - f.xlo + 1) + nuv * roi_chunks(2 * (f.cxhi - f.cxlo + 1)));
}
// ... and whether the staging loop can serve it: the lanes of one row are a power of two of the workgroup's threads
__host__ __device__ inline bool roi_stageable(const RoiFootprint &f) {
    return roi_chunks(f.xhi - f.xlo + 1) <= ROI_THREADS && roi_chunks(2 * (f.cxhi - f.cxlo + 1)) <= ROI_THREADS;
}
// first output column of tile column `tx` (tile_col0, vpp_device.h: the shifted last tile column of outputs 4 k + 2 columns wide)
__host__ __device__ inline int roi_tile_col0(int tx, int dst_w, int last_col0) {
    const int j = tx * ROI_TILE_W;
    return (last_col0 > 0 && j + ROI_TILE_W > dst_w) ? last_col0 : j;
}

// static LDS of the kernel's output side (MergedRun's exchange slabs, vpp_device.h): counts against the workgroup's LDS budget
inline int roi_static_lds(OutKind out, bool vec) {
    if (!vec) return 0;
    return out == O_F32_MERGED ? 256 * 48 : (out == O_U8_MERGED ? 256 * 12 : 0);
}

// (vpp_rois.hip) launches -- or, with `info`, only names -- the kernel of (mode, out, vec, staged); `name` receives the name tsvpp_describe_rois reports
hipError_t launch_rois(Mode mode, OutKind out, bool vec, bool staged, const RoiLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                       size_t name_len, bool dry_run);
// (vpp_rois_area.hip) the same for the AREA kernel; `lds_bytes` = L.area_lds + L.lds_bytes
hipError_t launch_rois_area(OutKind out, bool vec, bool staged, const RoiLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name, size_t name_len,
                            bool dry_run);
// (vpp_rois_tensor.hip / vpp_rois_area_tensor.hip) the same for the tensor instantiations: `out` is O_F32_PLANAR or O_Y800_F32 (three planes or one), the element is
// L.spec.dtype's
hipError_t launch_rois_tensor(Mode mode, OutKind out, bool vec, bool staged, const RoiLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                              size_t name_len, bool dry_run);
hipError_t launch_rois_area_tensor(OutKind out, bool vec, bool staged, const RoiLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                   size_t name_len, bool dry_run);

} // namespace tsvpp
