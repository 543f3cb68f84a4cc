// vpp_letterbox.h -- launch descriptor and tile geometry of the letterbox kernel (vpp_letterbox.hip), shared with the host API (tsvpp_letterbox.cpp:
// tsvpp_convert_letterbox / tsvpp_describe_letterbox).  The tile, the footprint functions and the staging rules are the ROI kernel's (vpp_rois.h); what this
// file adds is the inner rectangle of a canvas.  Product code -- never includes anything from oracle/.
#pragma once
#include "vpp_rois.h"

#pragma clang fp contract(off)

namespace tsvpp {

// What differs per frame.  Wave-uniform: the kernel indexes the record array with its workgroup's frame and reads the fields with scalar loads out of the kernarg
// segment.  The rectangle travels in 32-bit fields (32 records of 64 bytes fit the segment), so a canvas side has no limit of its own.
struct LbRec {
    uint64_t y, uv, out;              // plane addresses of the frame, address of its canvas
    int32_t pitch_y, pitch_uv;
    int32_t src_w, src_h;             // the frame
    float xr, yr;                     // (float)src_w / width, (float)src_h / height   (reference src/Resize.cu:418-419, with the inner rectangle as the output)
    int32_t left, top, width, height; // the inner rectangle inside the canvas: all even
};
static_assert(sizeof(LbRec) == 64, "LbRec layout");

// One launch: up to TSVPP_MAX_LETTERBOX frames, by value in the kernarg segment (2.1 KiB; HIP's hidden arguments take up to 256 bytes of the segment's 4 KiB).
struct LbLaunch {
    int32_t dst_w, dst_h; // the canvas
    int32_t swap_rb, color_g;
    tsvpp_coeffs k;
    int32_t tiles_x, tiles_y, n_frames;
    int32_t nt_stores, last_col0, u8_xchg; // as LaunchDesc's
    int32_t lds_bytes;                     // dynamic LDS of the launch's staged footprints: a tile whose footprint needs more gathers from global memory
    float pad_y, pad_u, pad_v;             // the pad sample, integer-valued (0..255): what the samplers would hand the colour back end
    LbRec r[TSVPP_MAX_LETTERBOX];
    tsvpp_tensor_spec spec;                // the tensor instantiations' dtype, mean[3], scale[3], once per launch (vpp_tensor_store.h); behind the records, as RoiLaunch's
};
static_assert(sizeof(LbLaunch) + 256 <= 4096, "LbLaunch no longer fits the kernarg segment");

// The part of canvas indices [first, last] of one axis that lies inside the rectangle [origin, origin + size), as indices of the rectangle's own grid:
// [lo, hi], empty (lo > hi) where the tile does not touch the rectangle.  `first`, `origin` and `size` are even and `last` is odd, so lo is even, hi is odd and
// the chroma pairs of the part are [lo >> 1, hi >> 1].
__host__ __device__ inline void lb_inner_range(int first, int last, int origin, int size, int &lo, int &hi) {
    lo = (first > origin ? first : origin) - origin;
    hi = (last < origin + size - 1 ? last : origin + size - 1) - origin;
}

// Source footprint of inner columns [a0, a1] / inner rows [b0, b1] in both planes: roi_span_x / roi_span_y (vpp_rois.h) for a run that need not start at a tile's
// first index nor be a tile long.  Host and device alike: the host sizes the launch's LDS with exactly the numbers the kernel will compute.
__host__ __device__ inline void lb_span_x(int mode, int a0, int a1, int src_w, float xr, RoiFootprint &f) {
    roi_axis_span(mode, a0, a1, xr, src_w, f.xlo, f.xhi);
    roi_clamp(f.xlo, f.xhi, src_w);
    roi_axis_span(mode, a0 >> 1, a1 >> 1, xr, src_w, f.cxlo, f.cxhi);
    roi_clamp(f.cxlo, f.cxhi, src_w >> 1);
}
__host__ __device__ inline void lb_span_y(int mode, int b0, int b1, int src_h, float yr, RoiFootprint &f) {
    roi_axis_span(mode, b0, b1, yr, src_h, f.ylo, f.yhi);
    roi_clamp(f.ylo, f.yhi, src_h);
    roi_axis_span(mode, b0 >> 1, b1 >> 1, yr, src_h, f.cylo, f.cyhi);
    roi_clamp(f.cylo, f.cyhi, src_h >> 1);
}
// last canvas column / row of the tile that starts at `first`
__host__ __device__ inline int lb_tile_last(int first, int tile, int dst) { return (first + tile < dst ? first + tile : dst) - 1; }

// (vpp_letterbox.hip) launches -- or, with `dry_run`, only names -- the kernel of (mode, out, vec, staged); `name` receives the name tsvpp_describe_letterbox reports
hipError_t launch_letterbox(Mode mode, OutKind out, bool vec, bool staged, const LbLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                            size_t name_len, bool dry_run);
// (vpp_letterbox_tensor.hip) the same for the tensor instantiations: `out` is O_F32_PLANAR or O_Y800_F32, the element is L.spec.dtype's
hipError_t launch_letterbox_tensor(Mode mode, OutKind out, bool vec, bool staged, const LbLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                   size_t name_len, bool dry_run);

} // namespace tsvpp
