// tsvpp_plan.cpp -- a request resolved on the host alone: tsvpp_params (+ frame geometry, + boxes) -> Plan / RoiPlan.  No HIP runtime call.
// The order in which make_plan, rois_plan and letterbox_plan return their statuses is part of the ABI (tests/test_plan_cpu.py, test_rois_cpu.py, test_abi_cpu.py,
// test_letterbox_cpu.py).
#include <cmath>

#include "tsvpp_host.h"
#include "vpp_mesh.h"
#include "vpp_persp.h"
#include "vpp_rois.h"

using namespace tsvpp;

namespace {

// Per-thread memo of a geometry predicate: a consumer thread converts thousands of frames with a handful of geometries (a
// full scan of a dyadic request costs dst_w + dst_h coordinate evaluations, ~20 us -- several single-frame conversions).
struct GeomMemo {
    struct Entry { int cls, dw, dh, sw, sh; bool res; };
    Entry e[16];
    int n = 0, next = 0;
    const bool *find(int cls, int dw, int dh, int sw, int sh) const {
        for (int i = 0; i < n; i++)
            if (e[i].cls == cls && e[i].dw == dw && e[i].dh == dh && e[i].sw == sw && e[i].sh == sh) return &e[i].res;
        return nullptr;
    }
    bool put(int cls, int dw, int dh, int sw, int sh, bool res) {
        e[next] = Entry{ cls, dw, dh, sw, sh, res };
        next = (next + 1) % 16;
        if (n < 16) n++;
        return res;
    }
};

// Is every interpolation weight of this request zero?  (odd integer ratios; then BILINEAR and
// BICUBIC reduce exactly to their centre tap, src/Resize.cu:17-23, 45-50 with w = 0)
bool all_weights_zero(Mode m, int dst_w, int dst_h, float xr, float yr, int src_w, int src_h) {
    static thread_local GeomMemo memo;
    if (const bool *hit = memo.find((int)m, dst_w, dst_h, src_w, src_h)) return *hit;
    auto remember = [&](bool r) { return memo.put((int)m, dst_w, dst_h, src_w, src_h, r); };
    for (int axis = 0; axis < 2; axis++) {
        const int n = axis ? dst_h : dst_w, lim = axis ? src_h : src_w;
        const float r = axis ? yr : xr;
        for (int o = 0; o < n; o++) { // the chroma grid uses indices 0 .. n/2-1, a subset
            int p;
            if (m == M_BILINEAR) {
                float w;
                bilinear_axis(o, r, lim, p, w);
                if (w != 0.0f) return remember(false);
            } else {
                double w;
                bicubic_axis(o, r, lim, p, w);
                if (w != 0.0) return remember(false);
            }
        }
    }
    return remember(true);
}

// BILINEAR: is every weight of ONE axis zero (an odd integer ratio on that axis only -- BASELINE config C3: 1280 -> 256 columns, ratio 5, rows at
// 2.8125)?  The taps that a zero weight multiplies need not be fetched (sample_luma / sample_chroma: LaunchDesc::wx_zero / wy_zero).
bool axis_weights_zero(int axis, int n, int lim, float r) {
    static thread_local GeomMemo memo;
    if (const bool *hit = memo.find(axis, n, 0, lim, 0)) return *hit;
    for (int o = 0; o < n; o++) {
        int p;
        float w;
        bilinear_axis(o, r, lim, p, w);
        if (w != 0.0f) return memo.put(axis, n, 0, lim, 0, false);
    }
    return memo.put(axis, n, 0, lim, 0, true);
}

// Is every interpolation weight of this request a multiple of 1/16?  (ratios 1.5, 2, 2.5, 4, 0.5, 1.25, 2.25 ...: then the
// reference's float / double evaluation is exact and the integer kernels -- vpp_bicubic_int.hip, the integer thread tile of
// the 2x2-tap kernel -- reproduce it bit for bit.)  BILINEAR and BICUBIC share one coordinate formula (src/Resize.cu:276-303,
// 321-347); the AREA up-scale variant has its own (:221-234).
bool weights_dyadic(Mode m, int dst_w, int dst_h, float xr, float yr, int src_w, int src_h) {
    static thread_local GeomMemo memo;
    const int cls = (m == M_AREA_UP) ? 1 : 0;
    if (const bool *hit = memo.find(cls, dst_w, dst_h, src_w, src_h)) return *hit;
    auto remember = [&](bool r) { return memo.put(cls, dst_w, dst_h, src_w, src_h, r); };
    for (int axis = 0; axis < 2; axis++) {
        const int n = axis ? dst_h : dst_w, lim = axis ? src_h : src_w;
        const float r = axis ? yr : xr;
        for (int o = 0; o < n; o++) { // the chroma grid uses indices 0 .. n/2-1, a subset
            int p;
            float w;
            if (m == M_AREA_UP) areaup_axis(o, r, p, w);
            else bilinear_axis(o, r, lim, p, w); // bicubic_axis: the same fp32 coordinate, widened afterwards
            const float s = w * 16.0f;
            if (s != std::floor(s)) return remember(false);
        }
    }
    return remember(true);
}

// resize_type -> Mode.  AREA answers M_AREA_DOWN: make_plan splits it by the ratios, rois_plan per box (and only for the AREA entry point).  False: unknown (the reference launches nothing and
// returns garbage).
bool resize_mode(int resize_type, Mode &m) {
    switch (resize_type) {
    case TSVPP_NEAREST: m = M_NEAREST; return true;
    case TSVPP_BILINEAR: m = M_BILINEAR; return true;
    case TSVPP_BICUBIC: m = M_BICUBIC; return true;
    case TSVPP_AREA: m = M_AREA_DOWN; return true;
    default: return false;
    }
}

// The colour and luma flavours of the fused kernels: RGB24 / BGR24 by layout and element type, Y800 by element type.  False: another FourCC (make_plan's own).
bool color_flavour(int fourcc, int planes, bool f32, OutKind &out, int &swap_rb) {
    switch (fourcc) {
    case TSVPP_RGB24: case TSVPP_BGR24:
        swap_rb = fourcc == TSVPP_BGR24 ? 1 : 0;
        out = f32 ? (planes == TSVPP_PLANAR ? O_F32_PLANAR : O_F32_MERGED) : (planes == TSVPP_PLANAR ? O_U8_PLANAR : O_U8_MERGED);
        return true;
    case TSVPP_Y800:
        swap_rb = 0;
        out = f32 ? O_Y800_F32 : O_Y800_U8;
        return true;
    default: return false;
    }
}

// ---- what rois_plan and letterbox_plan share (the caller has tested `p` and `frames` for null) ----
// TSVPP_ERROR class: parameters and frames that describe no request at all
int tile_frames_error(int n_frames, const tsvpp_nv12 *frames) {
    for (int f = 0; f < n_frames; f++) {
        const tsvpp_nv12 &fr = frames[f];
        if (fr.width <= 0 || fr.height <= 0) return TSVPP_ERROR;
        if (pitch_or_width(fr.pitch_y, fr.width) < fr.width || pitch_or_width(fr.pitch_uv, fr.width) < fr.width) return TSVPP_ERROR;
    }
    return TSVPP_OK;
}
int tile_request_error(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames) {
    if (p->crop_left || p->crop_top || p->crop_right || p->crop_bottom) return TSVPP_ERROR; // the boxes are the crops / the whole frame goes into the rectangle
    if (p->dst_width <= 0 || p->dst_height <= 0) return TSVPP_ERROR;
    return tile_frames_error(n_frames, frames);
}
// TSVPP_UNSUPPORTED class: sizes NV12 has no answer for
int tile_request_odd(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames) {
    if ((p->dst_width | p->dst_height) & 1) return TSVPP_UNSUPPORTED;
    for (int f = 0; f < n_frames; f++)
        if ((frames[f].width | frames[f].height) & 1) return TSVPP_UNSUPPORTED;
    return TSVPP_OK;
}
// TSVPP_UNSUPPORTED class: a frame whose plane spans the kernels' 32-bit offsets cannot carry (the calls that sample the whole frame; tile_request_odd has passed)
int tile_frame_spans(int n_frames, const tsvpp_nv12 *frames) {
    for (int f = 0; f < n_frames; f++) {
        const tsvpp_nv12 &fr = frames[f];
        if (source_span_status(fr.width, fr.height, pitch_or_width(fr.pitch_y, fr.width), pitch_or_width(fr.pitch_uv, fr.width)) != TSVPP_OK) return TSVPP_UNSUPPORTED;
    }
    return TSVPP_OK;
}
// TSVPP_UNSUPPORTED class: the resize type (`area`: the entry point answers AREA and nothing else), the output flavour and size, the grid of launches of up to
// `max_items` items
// ... its two halves: the resize type and the output flavour of the request,
int tile_output_flavour(const tsvpp_params *p, bool area, RoiPlan &pl) {
    if (!resize_mode(p->resize_type, pl.mode) || (pl.mode == M_AREA_DOWN) != area) return TSVPP_UNSUPPORTED;
    if (p->planes != TSVPP_PLANAR && p->planes != TSVPP_MERGED) return TSVPP_UNSUPPORTED;
    if (!color_flavour(p->fourcc, p->planes, p->normalization != 0, pl.out, pl.swap_rb)) return TSVPP_UNSUPPORTED; // NV12, UYVY, YUV444, HSV: not yet
    return TSVPP_OK;
}
// ... and one output of dst_w x dst_h in that flavour: its bytes, and the grid of a launch of `max_items` of them
int tile_output_size(const tsvpp_params *p, int dst_w, int dst_h, int max_items, size_t &out_bytes) {
    const int channels = p->fourcc == TSVPP_Y800 ? 1 : 3;
    out_bytes = (size_t)channels * (size_t)dst_w * (size_t)dst_h * (p->normalization != 0 ? sizeof(float) : 1);
    if (out_bytes >= ((size_t)1 << 32)) return TSVPP_UNSUPPORTED; // kernels use 32-bit offsets inside an output
    // one workgroup per output tile and item
    if ((long)((dst_w + ROI_TILE_W - 1) / ROI_TILE_W) * ((dst_h + ROI_TILE_H - 1) / ROI_TILE_H) * max_items >= (1L << 31)) return TSVPP_UNSUPPORTED;
    return TSVPP_OK;
}
int tile_output_plan(const tsvpp_params *p, bool area, int max_items, RoiPlan &pl) {
    if (tile_output_flavour(p, area, pl) != TSVPP_OK) return TSVPP_UNSUPPORTED;
    pl.dst_w = p->dst_width;
    pl.dst_h = p->dst_height;
    if (tile_output_size(p, pl.dst_w, pl.dst_h, max_items, pl.out_bytes) != TSVPP_OK) return TSVPP_UNSUPPORTED;
    pl.down = pl.taps_x = pl.taps_y = 0;
    return TSVPP_OK;
}

} // namespace

namespace tsvpp {

// Stage selection of VideoProcessor::Convert (reference src/VideoProcessor.cpp:106-142).
int make_plan(const tsvpp_params *p, int in_w, int in_h, Plan &pl) {
    if (!p || in_w <= 0 || in_h <= 0) return TSVPP_ERROR;
    if ((in_w | in_h) & 1) return TSVPP_UNSUPPORTED; // NV12 needs even sizes (reference: undefined)
    const int cw = p->crop_right - p->crop_left, ch = p->crop_bottom - p->crop_top;
    // crop only if the box is strictly smaller in BOTH dimensions (src/VideoProcessor.cpp:109)
    const bool crop = cw > 0 && ch > 0 && cw < in_w && ch < in_h;
    pl.src_w = in_w;
    pl.src_h = in_h;
    pl.off_x = pl.off_y = 0;
    if (crop) {
        if (p->crop_left < 0 || p->crop_top < 0 || p->crop_right > in_w || p->crop_bottom > in_h) return TSVPP_ERROR;
        if ((cw | ch) & 1) return TSVPP_UNSUPPORTED; // reference writes chroma out of bounds here
        pl.src_w = cw;
        pl.src_h = ch;
        pl.off_x = p->crop_left;
        pl.off_y = p->crop_top;
    }
    pl.dst_w = pl.src_w;
    pl.dst_h = pl.src_h;
    pl.mode = M_NONE;
    pl.xr = pl.yr = 1.0f;
    if (p->dst_width < 0 || p->dst_height < 0) return TSVPP_ERROR;
    if (p->dst_width && p->dst_height && (p->dst_width != pl.src_w || p->dst_height != pl.src_h)) {
        if ((p->dst_width | p->dst_height) & 1) return TSVPP_UNSUPPORTED; // reference leaves chroma unwritten
        pl.dst_w = p->dst_width;
        pl.dst_h = p->dst_height;
        pl.xr = (float)pl.src_w / (float)pl.dst_w; // src/Resize.cu:418-419
        pl.yr = (float)pl.src_h / (float)pl.dst_h;
        if (!resize_mode(p->resize_type, pl.mode)) return TSVPP_UNSUPPORTED;
        if (pl.mode == M_AREA_DOWN && !(pl.xr > 1.0f && pl.yr > 1.0f)) pl.mode = M_AREA_UP; // src/Resize.cu:435
    }
    pl.point_kind = PK_NONE;
    if (pl.mode == M_NEAREST) pl.point_kind = PK_NEAREST;
    else if ((pl.mode == M_BILINEAR || pl.mode == M_BICUBIC) && all_weights_zero(pl.mode, pl.dst_w, pl.dst_h, pl.xr, pl.yr, pl.src_w, pl.src_h))
        pl.point_kind = pl.mode == M_BILINEAR ? PK_BILINEAR0 : PK_BICUBIC0;
    pl.wx_zero = pl.wy_zero = 0;
    if (pl.mode == M_BILINEAR && pl.point_kind == PK_NONE) {
        pl.wx_zero = axis_weights_zero(0, pl.dst_w, pl.src_w, pl.xr) ? 1 : 0;
        pl.wy_zero = (!pl.wx_zero && axis_weights_zero(1, pl.dst_h, pl.src_h, pl.yr)) ? 1 : 0;
    }
    pl.w_dyadic = ((pl.mode == M_BICUBIC || pl.mode == M_BILINEAR || pl.mode == M_AREA_UP) && pl.point_kind == PK_NONE &&
                   weights_dyadic(pl.mode, pl.dst_w, pl.dst_h, pl.xr, pl.yr, pl.src_w, pl.src_h)) ? 1 : 0;
    pl.fourcc = p->fourcc;
    switch (p->fourcc) {
    case TSVPP_RGB24: case TSVPP_BGR24: case TSVPP_Y800: case TSVPP_NV12: case TSVPP_HSV: break; // output flavours of the fused kernels
    case TSVPP_UYVY: case TSVPP_YUV444: break;                                                    // second pass over the (resized) NV12
    default: return TSVPP_UNSUPPORTED;
    }
    if (p->planes != TSVPP_PLANAR && p->planes != TSVPP_MERGED) return TSVPP_UNSUPPORTED;
    // element type: src/VideoProcessor.cpp:139-142; HSV always runs the float kernels (src/ColorConversion.cu:357-370)
    const bool f32 = p->normalization != 0 || p->fourcc == TSVPP_HSV;
    pl.f32 = f32;
    if (!color_flavour(p->fourcc, p->planes, f32, pl.out, pl.swap_rb)) {
        if (p->fourcc == TSVPP_NV12) pl.out = f32 ? O_NV12_F32 : O_NV12_U8;
        else if (p->fourcc == TSVPP_HSV) pl.out = O_HSV_F32;
        else pl.out = O_NV12_U8; // UYVY / YUV444: pass 1
    }
    // channelsByFourCC: 1.5 for NV12 (src/VideoProcessor.cpp:4-14)
    const size_t elems = p->fourcc == TSVPP_NV12 ? (size_t)pl.dst_w * pl.dst_h * 3 / 2
                                                 : (size_t)(tsvpp_channels(p->fourcc) * (float)pl.dst_w) * (size_t)pl.dst_h;
    pl.out_bytes = elems * (f32 ? sizeof(float) : 1);
    if (pl.out_bytes >= ((size_t)1 << 32)) return TSVPP_UNSUPPORTED; // kernels use 32-bit offsets inside a frame
    return TSVPP_OK;
}

// What Convert's source planes add to make_plan's answer (tsvpp_convert*, tsvpp_describe): pitches of 0 resolved by the caller.  The region the kernels see is the
// plan's source -- the crop box, the planes advanced to its origin -- or the whole frame.
int plan_source_status(const Plan &pl, int in_w, int pitch_y, int pitch_uv) {
    if (pitch_y < in_w || pitch_uv < in_w) return TSVPP_ERROR;
    return source_span_status(pl.src_w, pl.src_h, pitch_y, pitch_uv);
}

int rois_plan(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois, RoiPlan &pl, bool area) {
    // TSVPP_ERROR: arguments that describe no request at all
    if (!p || !frames || !rois || n_frames <= 0 || n_rois <= 0) return TSVPP_ERROR;
    if (tile_request_error(p, n_frames, frames) != TSVPP_OK) return TSVPP_ERROR;
    for (int i = 0; i < n_rois; i++) {
        const tsvpp_roi &b = rois[i];
        if (b.frame < 0 || b.frame >= n_frames) return TSVPP_ERROR;
        const tsvpp_nv12 &fr = frames[b.frame];
        if (b.left < 0 || b.top < 0 || b.right <= b.left || b.bottom <= b.top || b.right > fr.width || b.bottom > fr.height) return TSVPP_ERROR;
    }
    // TSVPP_UNSUPPORTED: requests the library (or NV12 itself) has no answer for
    if (tile_request_odd(p, n_frames, frames) != TSVPP_OK) return TSVPP_UNSUPPORTED;
    for (int i = 0; i < n_rois; i++)
        if (((rois[i].right - rois[i].left) | (rois[i].bottom - rois[i].top)) & 1) return TSVPP_UNSUPPORTED;
    for (int i = 0; i < n_rois; i++) { // the source limit, per box: the kernel is handed the planes advanced to the box's origin
        const tsvpp_nv12 &fr = frames[rois[i].frame];
        if (source_span_status(rois[i].right - rois[i].left, rois[i].bottom - rois[i].top, pitch_or_width(fr.pitch_y, fr.width),
                               pitch_or_width(fr.pitch_uv, fr.width)) != TSVPP_OK)
            return TSVPP_UNSUPPORTED;
    }
    // AREA has an entry point of its own (tsvpp_convert_rois_area: its down-scale generates weight rows per tile), which answers nothing else
    if (tile_output_plan(p, area, TSVPP_MAX_ROIS, pl) != TSVPP_OK) return TSVPP_UNSUPPORTED;
    if (area) {
        if (pl.dst_w > ROI_AREA_MAX_DST || pl.dst_h > ROI_AREA_MAX_DST) return TSVPP_UNSUPPORTED;
        for (int i = 0; i < n_rois; i++) {
            const float xr = (float)(rois[i].right - rois[i].left) / (float)pl.dst_w, yr = (float)(rois[i].bottom - rois[i].top) / (float)pl.dst_h;
            if (roi_area_mode(xr, yr) != M_AREA_DOWN) continue;
            const int tx = roi_area_taps(xr), ty = roi_area_taps(yr);
            if (tx > ROI_AREA_MAX_TAPS || ty > ROI_AREA_MAX_TAPS) return TSVPP_UNSUPPORTED;
            pl.down++;
            pl.taps_x = tx > pl.taps_x ? tx : pl.taps_x;
            pl.taps_y = ty > pl.taps_y ? ty : pl.taps_y;
        }
    }
    return TSVPP_OK;
}

// tsvpp_convert_rois_sized and its siblings (include/tsvpp.h): rois_plan's rules in rois_plan's order -- every TSVPP_ERROR condition over all boxes, then every
// TSVPP_UNSUPPORTED one -- with the output size taken per box.  pl.dst_w / dst_h stay 0 (there is no one size), pl.out_bytes is the largest output's.
int rois_sized_plan(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi_sized *rois, RoiPlan &pl) {
    // TSVPP_ERROR: arguments that describe no request at all
    if (!p || !frames || !rois || n_frames <= 0 || n_rois <= 0) return TSVPP_ERROR;
    if (p->crop_left || p->crop_top || p->crop_right || p->crop_bottom) return TSVPP_ERROR; // the boxes are the crops
    if (p->dst_width || p->dst_height) return TSVPP_ERROR;                                  // the sizes are the boxes': a caller who sets these believes they apply
    if (tile_frames_error(n_frames, frames) != TSVPP_OK) return TSVPP_ERROR;
    for (int i = 0; i < n_rois; i++) {
        const tsvpp_roi_sized &b = rois[i];
        if (b.frame < 0 || b.frame >= n_frames) return TSVPP_ERROR;
        const tsvpp_nv12 &fr = frames[b.frame];
        if (b.left < 0 || b.top < 0 || b.right <= b.left || b.bottom <= b.top || b.right > fr.width || b.bottom > fr.height) return TSVPP_ERROR;
        if (b.dst_width <= 0 || b.dst_height <= 0) return TSVPP_ERROR;
    }
    // TSVPP_UNSUPPORTED: requests the library (or NV12 itself) has no answer for
    for (int f = 0; f < n_frames; f++)
        if ((frames[f].width | frames[f].height) & 1) return TSVPP_UNSUPPORTED;
    for (int i = 0; i < n_rois; i++)
        if (((rois[i].right - rois[i].left) | (rois[i].bottom - rois[i].top) | rois[i].dst_width | rois[i].dst_height) & 1) return TSVPP_UNSUPPORTED;
    for (int i = 0; i < n_rois; i++) { // the source limit, per box: the kernel is handed the planes advanced to the box's origin
        const tsvpp_nv12 &fr = frames[rois[i].frame];
        if (source_span_status(rois[i].right - rois[i].left, rois[i].bottom - rois[i].top, pitch_or_width(fr.pitch_y, fr.width),
                               pitch_or_width(fr.pitch_uv, fr.width)) != TSVPP_OK)
            return TSVPP_UNSUPPORTED;
    }
    // AREA: its kernel generates weight rows per tile behind a serial chain over the output columns -- the wrong shape for wide strips, a follow-up
    if (tile_output_flavour(p, false, pl) != TSVPP_OK) return TSVPP_UNSUPPORTED;
    pl.dst_w = pl.dst_h = 0;
    pl.out_bytes = 0;
    pl.down = pl.taps_x = pl.taps_y = 0;
    for (int i = 0; i < n_rois; i++) {
        size_t bytes;
        if (tile_output_size(p, rois[i].dst_width, rois[i].dst_height, TSVPP_MAX_ROIS_SIZED, bytes) != TSVPP_OK) return TSVPP_UNSUPPORTED;
        pl.out_bytes = bytes > pl.out_bytes ? bytes : pl.out_bytes;
    }
    return TSVPP_OK;
}

// The rectangle of frame k: the caller's, or the default one (tsvpp_letterbox_rect; sizes are positive and the canvas even by the time this is asked)
tsvpp_rect letterbox_rect_of(const tsvpp_nv12 *in, const tsvpp_rect *rects, int k, int dst_w, int dst_h) {
    if (rects) return rects[k];
    tsvpp_rect r = {};
    (void)tsvpp_letterbox_rect(in[k].width, in[k].height, dst_w, dst_h, &r);
    return r;
}

// The request rules of both letterbox calls, in the one order that decides which status a request with two faults gets; `area`: which of them is asked (each
// answers TSVPP_UNSUPPORTED to the other's resize types)
static int letterbox_request(const tsvpp_params *p, int n, const tsvpp_nv12 *in, const tsvpp_rect *rects, int pad_y, int pad_u, int pad_v, bool area, RoiPlan &pl) {
    // TSVPP_ERROR: arguments that describe no request at all
    if (!p || !in || n <= 0) return TSVPP_ERROR;
    if (tile_request_error(p, n, in) != TSVPP_OK) return TSVPP_ERROR;
    for (int f = 0; rects && f < n; f++) {
        const tsvpp_rect &r = rects[f];
        if (r.width <= 0 || r.height <= 0 || r.left < 0 || r.top < 0) return TSVPP_ERROR;
        if ((long)r.left + r.width > p->dst_width || (long)r.top + r.height > p->dst_height) return TSVPP_ERROR;
    }
    if (pad_y < 0 || pad_y > 255 || pad_u < 0 || pad_u > 255 || pad_v < 0 || pad_v > 255) return TSVPP_ERROR;
    // TSVPP_UNSUPPORTED: requests the library (or NV12 itself) has no answer for
    if (tile_request_odd(p, n, in) != TSVPP_OK) return TSVPP_UNSUPPORTED;
    for (int f = 0; rects && f < n; f++) // (the default rectangle of an even canvas is even)
        if ((rects[f].left | rects[f].top | rects[f].width | rects[f].height) & 1) return TSVPP_UNSUPPORTED;
    if (tile_frame_spans(n, in) != TSVPP_OK) return TSVPP_UNSUPPORTED;
    // AREA: its down-scale needs weight rows, which a kernel of its own generates per tile (vpp_letterbox_area.hip, tsvpp_convert_letterbox_area).  The rectangle
    // travels in 32-bit fields: a canvas side has no limit of its own, the grid has
    return tile_output_plan(p, area, TSVPP_MAX_LETTERBOX, pl);
}

int letterbox_plan(const tsvpp_params *p, int n, const tsvpp_nv12 *in, const tsvpp_rect *rects, int pad_y, int pad_u, int pad_v, RoiPlan &pl) {
    return letterbox_request(p, n, in, rects, pad_y, pad_u, pad_v, false, pl);
}

// tsvpp_convert_letterbox_area: the letterbox call's rules, then tsvpp_convert_rois_area's limits with the rectangle as the output -- the generator never runs
// further than a rectangle is wide / high, and a down-scale frame's weight rows must fit the tile's LDS
int letterbox_area_plan(const tsvpp_params *p, int n, const tsvpp_nv12 *in, const tsvpp_rect *rects, int pad_y, int pad_u, int pad_v, RoiPlan &pl) {
    const int sts = letterbox_request(p, n, in, rects, pad_y, pad_u, pad_v, true, pl);
    if (sts != TSVPP_OK) return sts;
    for (int f = 0; f < n; f++) {
        const tsvpp_rect rc = letterbox_rect_of(in, rects, f, pl.dst_w, pl.dst_h);
        if (rc.width > ROI_AREA_MAX_DST || rc.height > ROI_AREA_MAX_DST) return TSVPP_UNSUPPORTED;
        const float xr = (float)in[f].width / (float)rc.width, yr = (float)in[f].height / (float)rc.height;
        if (roi_area_mode(xr, yr) != M_AREA_DOWN) continue;
        const int tx = roi_area_taps(xr), ty = roi_area_taps(yr);
        if (tx > ROI_AREA_MAX_TAPS || ty > ROI_AREA_MAX_TAPS) return TSVPP_UNSUPPORTED;
        pl.down++;
        pl.taps_x = tx > pl.taps_x ? tx : pl.taps_x;
        pl.taps_y = ty > pl.taps_y ? ty : pl.taps_y;
    }
    return TSVPP_OK;
}

// The border of the coordinate paths: (-1, -1, -1) replicates the frame's edge, anything else is a sample, each value 0..255
static bool coord_border_ok(int border_y, int border_u, int border_v) {
    if (border_y == -1 && border_u == -1 && border_v == -1) return true;
    return border_y >= 0 && border_y <= 255 && border_u >= 0 && border_u <= 255 && border_v >= 0 && border_v <= 255;
}

// The request skeleton of the four coordinate paths (warp_plan, persp_plan, remap_plan, mesh_plan), once: the rules they share, in the one order that decides
// which status a request with two faults gets.  A path passes what it alone knows: `given` -- its own arrays are there and not empty; index_ok(i) -- item i names
// a frame (and a map, a mesh) of the request; path_error() / path_unsupported() -- whether one of its own TSVPP_ERROR / TSVPP_UNSUPPORTED rules is broken.
// `limit` = outputs per launch; `filter` = the one resize type the entry point samples with (M_BILINEAR, or M_BICUBIC for the *_bicubic calls)
template <class INDEX, class ERR, class UNS>
int coord_plan(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, bool given, int n, int border_y, int border_u, int border_v, int limit, Mode filter,
               RoiPlan &pl, INDEX index_ok, ERR path_error, UNS path_unsupported) {
    // TSVPP_ERROR: arguments that describe no request at all
    if (!p || !frames || n_frames <= 0 || !given || n <= 0) return TSVPP_ERROR;
    if (tile_request_error(p, n_frames, frames) != TSVPP_OK) return TSVPP_ERROR;
    for (int i = 0; i < n; i++)
        if (!index_ok(i)) return TSVPP_ERROR;
    if (!coord_border_ok(border_y, border_u, border_v)) return TSVPP_ERROR;
    if (path_error()) return TSVPP_ERROR;
    // TSVPP_UNSUPPORTED: requests the library (or NV12 itself) has no answer for
    if (tile_request_odd(p, n_frames, frames) != TSVPP_OK) return TSVPP_UNSUPPORTED;
    if (tile_frame_spans(n_frames, frames) != TSVPP_OK) return TSVPP_UNSUPPORTED;
    // every other resize type belongs to another entry point (BICUBIC warps: tsvpp_convert_warp_bicubic) or is a follow-up (NEAREST, AREA)
    if (tile_output_plan(p, false, limit, pl) != TSVPP_OK || pl.mode != filter) return TSVPP_UNSUPPORTED;
    return path_unsupported() ? TSVPP_UNSUPPORTED : TSVPP_OK;
}

// ... of the matrix paths: REC is tsvpp_warp (K = 6 entries) or tsvpp_persp (K = 9).  `any` = some entry of some matrix satisfies the predicate
template <class REC, int K>
int matrix_plan(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n, const REC *recs, float (REC::*entries)[K], int border_y, int border_u,
                int border_v, int limit, Mode filter, RoiPlan &pl) {
    const auto any = [&](auto pred) {
        for (int i = 0; i < n; i++)
            for (int k = 0; k < K; k++)
                if (pred((recs[i].*entries)[k])) return true;
        return false;
    };
    return coord_plan(
        p, n_frames, frames, recs != nullptr, n, border_y, border_u, border_v, limit, filter, pl, [&](int i) { return recs[i].frame >= 0 && recs[i].frame < n_frames; },
        [&] { return any([](float v) { return !std::isfinite(v); }); },
        // with every entry inside 2^24 and indices below 2^31 no numerator or denominator overflows: every one is finite
        [&] { return any([](float v) { return std::fabs(v) > 16777216.0f; }); });
}

int warp_plan(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_warps, const tsvpp_warp *warps, int border_y, int border_u, int border_v, RoiPlan &pl,
              Mode filter) {
    return matrix_plan(p, n_frames, frames, n_warps, warps, &tsvpp_warp::m, border_y, border_u, border_v, TSVPP_MAX_WARPS, filter, pl);
}

int persp_plan(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n, const tsvpp_persp *persps, int border_y, int border_u, int border_v, RoiPlan &pl,
               Mode filter) {
    const int sts = matrix_plan(p, n_frames, frames, n, persps, &tsvpp_persp::h, border_y, border_u, border_v, TSVPP_MAX_PERSP, filter, pl);
    if (sts != TSVPP_OK) return sts;
    // the horizon: the denominator, as the kernel evaluates it, is monotone in each index, so its least value over the output is that of a corner pixel (luma
    // grid) or corner pair (chroma grid).  Below 2^-64 a reciprocal could overflow or change sign: no answer
    for (int i = 0; i < n; i++) {
        PerspGrid luma, chroma;
        persp_terms(persps[i].h, luma, chroma);
        if (!(persp_min_denominator(luma, 0, pl.dst_w - 1, 0, pl.dst_h - 1) >= PERSP_MIN_DENOMINATOR)) return TSVPP_UNSUPPORTED;
        if (!(persp_min_denominator(chroma, 0, (pl.dst_w >> 1) - 1, 0, (pl.dst_h >> 1) - 1) >= PERSP_MIN_DENOMINATOR)) return TSVPP_UNSUPPORTED;
    }
    return TSVPP_OK;
}

// item i of a map path names a frame and a grid (a map, a mesh) of the request
static bool remap_index_ok(const tsvpp_remap &r, int n_frames, int n_grids) { return r.frame >= 0 && r.frame < n_frames && r.map >= 0 && r.map < n_grids; }

int remap_plan(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_maps, const tsvpp_map *maps, int n, const tsvpp_remap *remaps, int border_y,
               int border_u, int border_v, RoiPlan &pl) {
    return coord_plan(
        p, n_frames, frames, maps && remaps && n_maps > 0, n, border_y, border_u, border_v, TSVPP_MAX_REMAPS, M_BILINEAR, pl,
        [&](int i) { return remap_index_ok(remaps[i], n_frames, n_maps); },
        [&] {
            for (int m = 0; m < n_maps; m++) {
                if (maps[m].pitch != 0 && ((long)maps[m].pitch < 8L * p->dst_width || (maps[m].pitch & 7))) return true;
                if (maps[m].pitch == 0 && 8L * p->dst_width > 0x7fffffffL) return true; // (the tight pitch travels in 32 bits)
                if (maps[m].lds_bytes < 0) return true;
            }
            return false;
        },
        [] { return false; });
}

int mesh_plan(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_meshes, const tsvpp_mesh *meshes, int n, const tsvpp_remap *remaps, int border_y,
              int border_u, int border_v, RoiPlan &pl) {
    const auto cell_ok = [](int l) { return l >= MESH_LOG2_MIN && l <= MESH_LOG2_MAX; };
    return coord_plan(
        p, n_frames, frames, meshes && remaps && n_meshes > 0, n, border_y, border_u, border_v, TSVPP_MAX_MESHES, M_BILINEAR, pl,
        [&](int i) { return remap_index_ok(remaps[i], n_frames, n_meshes); },
        [&] {
            for (int m = 0; m < n_meshes; m++) {
                // (a cell size outside the range has no column count to hold a pitch against: its answer is TSVPP_UNSUPPORTED, below)
                if (meshes[m].pitch & 7) return true;
                if (cell_ok(meshes[m].log2_cw) && meshes[m].pitch != 0 && (long)meshes[m].pitch < 8L * mesh_points(p->dst_width, meshes[m].log2_cw)) return true;
                if (meshes[m].lds_bytes < 0) return true;
            }
            return false;
        },
        [&] {
            for (int m = 0; m < n_meshes; m++)
                if (!cell_ok(meshes[m].log2_cw) || !cell_ok(meshes[m].log2_ch)) return true;
            return false;
        });
}

// One spec check for both tensor paths. The caller has the plan's status already (it wins); what is left is about the spec and about what the tensor stores cover.
int tensor_spec_status(const tsvpp_params *p, const tsvpp_tensor_spec *spec) {
    if (!p || !spec) return TSVPP_ERROR;
    const int used = p->fourcc == TSVPP_Y800 ? 1 : 3; // channels the format reads mean / scale of (a fourcc outside the list: all three, then rule 3)
    for (int c = 0; c < used; c++)
        if (!std::isfinite(spec->mean[c]) || !std::isfinite(spec->scale[c]) || spec->scale[c] == 0.0f) return TSVPP_ERROR;
    if (spec->dtype != TSVPP_F32 && spec->dtype != TSVPP_F16 && spec->dtype != TSVPP_BF16) return TSVPP_UNSUPPORTED;
    if (p->normalization == 0) return TSVPP_UNSUPPORTED; // the contract is stated on q = k / 255
    if (p->fourcc == TSVPP_Y800) return TSVPP_OK;
    if (p->fourcc != TSVPP_RGB24 && p->fourcc != TSVPP_BGR24) return TSVPP_UNSUPPORTED;
    return p->planes == TSVPP_PLANAR ? TSVPP_OK : TSVPP_UNSUPPORTED; // merged half-precision output: out of scope
}

} // namespace tsvpp

extern "C" {

size_t tsvpp_tensor_bytes(const tsvpp_params *p, const tsvpp_tensor_spec *spec) {
    if (tensor_spec_status(p, spec) != TSVPP_OK) return 0;
    if (p->dst_width <= 0 || p->dst_height <= 0 || ((p->dst_width | p->dst_height) & 1)) return 0;
    const size_t elems = (size_t)(p->fourcc == TSVPP_Y800 ? 1 : 3) * (size_t)p->dst_width * (size_t)p->dst_height;
    if (elems * sizeof(float) >= ((size_t)1 << 32)) return 0; // the plans' limit, which is stated on fp32
    return elems * tensor_elem_bytes(spec->dtype);
}

size_t tsvpp_rois_sized_bytes(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int dst_width, int dst_height) {
    if (!p || p->dst_width || p->dst_height || p->crop_left || p->crop_top || p->crop_right || p->crop_bottom) return 0;
    if (dst_width <= 0 || dst_height <= 0 || ((dst_width | dst_height) & 1)) return 0;
    RoiPlan pl;
    size_t bytes;
    if (tile_output_flavour(p, false, pl) != TSVPP_OK) return 0;
    if (!spec) return tile_output_size(p, dst_width, dst_height, TSVPP_MAX_ROIS_SIZED, bytes) == TSVPP_OK ? bytes : 0;
    if (tensor_spec_status(p, spec) != TSVPP_OK) return 0; // (normalization != 0 from here on: `bytes` is the fp32 size the plan's limit is stated on)
    if (tile_output_size(p, dst_width, dst_height, TSVPP_MAX_ROIS_SIZED, bytes) != TSVPP_OK) return 0;
    return bytes / sizeof(float) * tensor_elem_bytes(spec->dtype);
}

float tsvpp_channels(int fourcc) {
    if (fourcc == TSVPP_Y800) return 1.0f;
    if (fourcc == TSVPP_UYVY) return 2.0f;
    if (fourcc == TSVPP_NV12) return 1.5f;
    return 3.0f;
}

int tsvpp_out_dims(const tsvpp_params *p, int in_width, int in_height, int *out_width, int *out_height) {
    Plan pl;
    int sts = make_plan(p, in_width, in_height, pl);
    if (sts != TSVPP_OK) return sts;
    if (out_width) *out_width = pl.dst_w;
    if (out_height) *out_height = pl.dst_h;
    return TSVPP_OK;
}

size_t tsvpp_out_bytes(const tsvpp_params *p, int in_width, int in_height) {
    Plan pl;
    if (make_plan(p, in_width, in_height, pl) != TSVPP_OK) return 0;
    return pl.out_bytes;
}

} // extern "C"
