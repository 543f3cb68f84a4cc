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

// (the part of a tile inside the rectangle and its source footprint: tile_inner_range, tile_span_x / tile_span_y, vpp_rois.h)

// (vpp_letterbox.hip) launches -- or, with `dry_run`, only names -- the kernel of (mode, out, vec, staged); `name` receives the name tsvpp_describe_letterbox reports
hipError_t launch_letterbox(Mode mode, OutKind out, bool vec, bool staged, const LbLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                            size_t name_len, bool dry_run);
// (vpp_letterbox_tensor.hip) the same for the tensor instantiations: `out` is O_F32_PLANAR or O_Y800_F32, the element is L.spec.dtype's
hipError_t launch_letterbox_tensor(Mode mode, OutKind out, bool vec, bool staged, const LbLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                   size_t name_len, bool dry_run);

} // namespace tsvpp
