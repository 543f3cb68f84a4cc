// tsvpp_host.h -- private to the host side of the C ABI (tsvpp_*.cpp): the records those files share and the few functions that cross between them.
//   tsvpp_plan.cpp   request -> Plan / RoiPlan (no HIP runtime call)
//   tsvpp_area.cpp   AREA weight tables, their device cache, the AREA fields of a launch descriptor
//   tsvpp_api.cpp    contexts, streams, knobs, the conversion itself and its replay cache, tsvpp_describe
//   tsvpp_table.cpp  persistent frame tables
//   tsvpp_tiles.h    what the tile paths below share (templates): the launch fill, the staging budgets, the convert and describe skeletons; and what the four
//                    coordinate paths share beyond that (CoordRequest: request fields, border, record and launch fill, the pair of launchers)
//   tsvpp_rois.cpp   regions of interest (both entry points: NEAREST / BILINEAR / BICUBIC and AREA)
//   tsvpp_rois_sized.cpp regions of interest, each to its own output size (a skeleton of its own: the boxes of a call are split by store class)
//   tsvpp_letterbox.cpp  aspect-preserving resize into a padded canvas
//   tsvpp_letterbox_area.cpp  the same with AREA: weight rows generated per tile, from a jump start
//   tsvpp_warp.cpp   affine warps        } the coordinate paths: one path with a different source coordinate.  Each file holds its record's geometry, its
//   tsvpp_persp.cpp  homographies        } footprint function or LDS hint, its labels, its entry points and its host-only helpers; the request skeleton they
//   tsvpp_remap.cpp  coordinate maps     } share is coord_plan (tsvpp_plan.cpp)
//   tsvpp_mesh.cpp   control-grid warps  }
// (the tensor entry points -- fp16 / bf16 / fp32 with mean and scale -- live with the path they extend: tsvpp_rois.cpp, tsvpp_letterbox.cpp, tsvpp_warp.cpp, ...)
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "tsvpp.h"
#include "vpp_kernels.h"
#include "vpp_axis.h"

namespace tsvpp {

// What the kernel selection needs to know about the AREA weight table of one axis: derived from the scale alone, on the host (area_axis).
struct AreaAxis {
    int rows = 0, taps = 0;
    int nk = 0;               // taps4 = 4 * nk
    int ones_end = 0;         // taps 1 .. ones_end - 1 weigh exactly 1.0f in every row (the streaming kernel multiplies nothing there)
    bool dyadic = false;      // an integer form exists: every weight is k / 2^shift and taps <= 8
    int shift = -1;
    int uniform_sum = 0;      // > 0: every row of the integer table has this weight sum
};
// ... and the table itself on a device (get_area_table; the dry-run area_desc fills in stand-ins)
struct AreaTable : AreaAxis {
    float *dev = nullptr;
    AreaQRow *qdev = nullptr; // integer form, only if `dyadic` (and its upload succeeded)
    float *dev4 = nullptr;    // the float rows zero-padded to a multiple of four taps
    std::shared_ptr<std::vector<float>> host4; // host copy of dev4 (divisor tables of the float AREA kernels)
};

struct Plan {
    Mode mode = M_NONE;
    OutKind out = O_U8_MERGED;
    int off_x = 0, off_y = 0; // crop origin
    int src_w = 0, src_h = 0; // logical source after crop
    int dst_w = 0, dst_h = 0;
    float xr = 1.f, yr = 1.f;
    int swap_rb = 0;
    size_t out_bytes = 0;
    int point_kind = PK_NONE;
    int wx_zero = 0, wy_zero = 0; // BILINEAR: every weight of that axis is zero (and not of both: that is point_kind)
    int w_dyadic = 0;
    int fourcc = TSVPP_RGB24;
    bool f32 = false;
};

// The request of tsvpp_convert_rois / tsvpp_describe_rois and of their AREA counterparts, checked and resolved on the host alone.
struct RoiPlan {
    Mode mode = M_NONE; // M_AREA_DOWN: the AREA entry point -- every box chooses between the down-scale and the up-scale rule (roi_area_mode, vpp_rois.h)
    OutKind out = O_U8_MERGED;
    int dst_w = 0, dst_h = 0, swap_rb = 0;
    size_t out_bytes = 0;
    int down = 0, taps_x = 0, taps_y = 0; // AREA: boxes on the down-scale path, their largest tap counts
};

// An int that tsvpp_set_option / tsvpp_enable_markers may write while conversions on other threads read it (include/tsvpp.h: options may be set beside
// conversions).  Relaxed atomic accesses -- plain loads and stores on x86: the replay hit pays nothing for them -- and copyable, so that Knobs stays plain data.
// A writer stores the value FIRST and moves tsvpp_ctx::epoch afterwards; a conversion loads the epoch (acquire) before it reads any option, so a launch is never
// remembered under an epoch newer than the values it was built from.
struct OptInt {
    std::atomic<int> v;
    OptInt(int x = 0) : v(x) {}
    OptInt(const OptInt &o) : v(o.load()) {}
    OptInt &operator=(const OptInt &o) { store(o.load()); return *this; }
    OptInt &operator=(int x) { store(x); return *this; }
    operator int() const { return load(); }
    int load() const { return v.load(std::memory_order_relaxed); }
    void store(int x) { v.store(x, std::memory_order_relaxed); }
};

// Everything of a context that the launch descriptor is filled from (fill_desc): the tuning knobs (read_env_knobs) and the two options the API sets that
// travel in the descriptor.  Plain data: tsvpp_describe makes one of its own, without a context.  A knob that travels in the descriptor has its LaunchDesc
// member's name; kKnobs (tsvpp_api.cpp) is the one place that says which environment variable sets it and where it goes.
struct Knobs {
    tsvpp_coeffs coeffs;                // tsvpp_set_coeffs (a quiescent context only: include/tsvpp.h)
    OptInt color_g;                     // TSVPP_OPT_COLOR_G_TERM
    int force_gather = 0;               // TSVPP_FORCE_GATHER=1: always use the global-gather kernel (A/B, tests)
    int nt_stores = -1, tile_order = 0, shape_tx = 0, shape_ty = 0; // TSVPP_NT (0 plain, 1 nt, 2 sc1; -1 = per kernel), TSVPP_TILE_ORDER, TSVPP_SHAPE=tx,ty
    int num_cus = 256;                  // compute units of the device (tsvpp_create reads it; 256 without a device)
    // dyadic AREA reads straight from global memory from this ratio on (both axes); below it the LDS kernel wins
    // (measured after its VGPR fix: 2x 501 k vs 368 k fps, 3x 743 k vs 621 k, 4x 162 k vs 251 k)
    float area_direct_min = 3.5f;   // TSVPP_AREA_DIRECT_MIN
    float area_direct_fmin = 2.0f;  // the same for non-dyadic weights (a constant since round 3)
    int bicubic_int_pref = 1;       // TSVPP_BICUBIC_INT: integer kernels for dyadic weights (1: + the streaming kernel at 3 : 2 / 2 : 1, 2: the LDS kernel only, 0: none)
    int bil_int_pref = 1;           // TSVPP_BILINEAR_INT: integer thread tile of the 2x2-tap kernel for dyadic weights
    int area_box_pref = 1;          // TSVPP_AREA_BOX: contiguous-run box kernel for integer ratios >= 4
    int area2_pref = 1;             // float-weight AREA at 2 x 2 .. 3 x 3 taps on its own LDS kernel
    int lds_budget_kb = 40;         // TSVPP_LDS_KB: LDS KiB a staged workgroup may use (four workgroups per CU; tests: a budget nothing fits)
    int bil_win_pref = 1;           // window form of the float 2x2-tap thread tile where it measured faster (ratios 1 .. 1.45)
    int u8_xchg = 1;                // 16-byte stores for uint8 merged outputs through an in-wave LDS exchange
    int area_divtab = 1;            // TSVPP_AREA_DIVTAB: host-built divisor table for the float AREA kernels
    int area_cols_rows = 0;         // TSVPP_AREA_COLS_ROWS: tile height of the column-per-lane AREA kernel (8 | 32; 0: by tap count and launch size)
    int tail_shift = 1;             // TSVPP_TAIL_SHIFT: outputs 4 k + 2 columns wide end in a shifted tile column instead of a row tail and its second launch (0: the two-column tail launch of rounds 1-3, A/B)
    int area_cols_pref = 1;         // TSVPP_AREA_COLS
    int rpt_pref = 0;               // TSVPP_RPT: row pairs per thread, 0 = per kernel (launch_fused)
    int dma = 1;                    // TSVPP_DMA=0 selects the register-staged path
    int r32_pref = 1;               // TSVPP_R32: streaming kernel for BILINEAR at exactly 3 : 2 with uint8 outputs
    int bicubic_cols_pref = 1;      // TSVPP_BICUBIC_COLS: wave-per-tile BICUBIC kernel (1: what the integer kernel does not take, 2: every BICUBIC request, 0: off)
    int area_stream_pref = 1;       // TSVPP_AREA_STREAM: float-weight AREA with the source rows streamed through a wave-private LDS ring (vpp_area_stream.hip)
    int as_rows = 0;                // its tile height: automatic (4)
    int as_min_taps = 40;           // ... from this many taps (rx * ry) per value on (measured cross-over)
    int bc_rows = 0;                // TSVPP_BICUBIC_ROWS: its tile height (8 / 16 / 24 / 32; 0 = automatic)
    int bc_dma_pref = 1;            // TSVPP_BICUBIC_DMA: its source rows through a wave-private LDS-DMA ring (0: per-lane loads)
    int bil_rows_pref = 1;          // TSVPP_BILINEAR_ROWS: BILINEAR at sparse ratios with the tapped rows as LDS-DMA row segments (vpp_bilinear_rows.hip; 1: ratio product >= 12, 2: wherever it applies, 0: byte gathers)
    int bc_u8x_pref = 1;            // TSVPP_BICUBIC_U8X: uint8 outputs of the wave-per-tile BICUBIC kernel through the 8 x 4 output side of the streaming kernels
    int point_rn_pref = 1;          // TSVPP_POINT_RN: streaming point sampler at exact integer ratios 3 / 4 / 5 (vpp_point_rn.hip; 0: the LDS point kernel)
    int br_waves = 0;               // TSVPP_BILINEAR_ROWS_WAVES: its waves per workgroup (1 / 2 / 4; 0 = automatic: launch_fused chooses)
    int geo_pref = 1;               // TSVPP_GEO: host-built geometry tables for the 2x2-tap kernel's window tiles (1: where measured to win, 2: wherever they apply)
    int replay = 1;                 // TSVPP_REPLAY=0 (debug knob): every call runs the full selection
    int debug = 0;                  // TSVPP_DEBUG_KNOBS=1, the gate itself: every conversion keeps its launch record for tsvpp_debug_last_launch
    Knobs() { tsvpp_default_coeffs(&coeffs); }
};

} // namespace tsvpp

struct tsvpp_ctx {
    int device = 0;
    std::vector<std::pair<std::string, hipStream_t>> streams;
    std::vector<hipStream_t> streams2; // TSVPP_OPT_INPUTS_READY: a consumer's second stream (created on first use), same index as `streams`
    std::vector<uint8_t> turn;         // ... and which of the two its next conversion takes
    std::mutex stream_mu;
    tsvpp::Knobs knobs;
    std::map<uint32_t, tsvpp::AreaTable> area; // keyed by the bit pattern of the float scale
    std::map<uint64_t, float *> area_div; // divisor tables, keyed by both scales' bit patterns
    tsvpp::GeoCache *geo = nullptr; // device copies of the geometry tables (Knobs::geo_pref), one set per (request geometry, tile shape)
    std::mutex area_mu;
    // NV12 intermediates of the two-pass formats (UYVY / YUV444 with a resize): one grow-only slot per stream.  A slot's
    // mutex is held while BOTH passes of a call are enqueued, so calls that share a stream (typically NULL) cannot
    // interleave their passes on the shared buffer; a buffer that is outgrown is retired, not freed -- work already
    // enqueued may still use it and hipFree would synchronise the device -- and released in tsvpp_destroy.
    struct ScratchSlot {
        std::mutex mu;
        uint8_t *buf = nullptr;
        size_t bytes = 0;
    };
    std::map<void *, std::unique_ptr<ScratchSlot>> scratch;
    std::vector<uint8_t *> retired;
    std::mutex scratch_mu;
    tsvpp::OptInt markers; // tsvpp_enable_markers: roctx ranges around every conversion (the reference's NVTX ranges)
    tsvpp::OptInt inputs_ready; // TSVPP_OPT_INPUTS_READY: fused launches do not wait for earlier work on their stream (include/tsvpp.h)
    // Replay cache (convert_impl): a thread keeps the finished launches of its last requests, keyed by this context's id and epoch.  The epoch moves whenever
    // something a finished launch descriptor depends on changes or may be freed: tsvpp_set_coeffs, tsvpp_set_option, tsvpp_enable_markers, tsvpp_trim.
    uint64_t id = 0;
    std::atomic<uint64_t> epoch{ 1 };
    tsvpp::OptInt unsafe_coeffs; // TSVPP_OPT_UNSAFE_COEFFS: tsvpp_set_coeffs accepts a block that differs from the defaults
    std::set<struct tsvpp_table *> tables; // live frame tables: released with the context if the caller destroys it first
    std::mutex tables_mu;
};

namespace tsvpp {

// Selects the context's device for the duration of one API call and restores the caller's on exit (as torch's
// CUDAGuard does): a VideoProcessor bound to device k must not change the calling thread's current device.
struct DeviceGuard {
    int prev = -1, status = TSVPP_OK;
    bool switched = false;
    explicit DeviceGuard(const tsvpp_ctx *ctx) {
        hipError_t e = hipGetDevice(&prev);
        if (e != hipSuccess) { status = (int)e; return; }
        if (prev != ctx->device) {
            e = hipSetDevice(ctx->device);
            if (e != hipSuccess) { status = (int)e; return; }
            switched = true;
        }
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// roctx ranges (the reference brackets Convert with NVTX ranges: include/Common.h:72-105, src/VideoProcessor.cpp:95).
// The tracer library is looked up at run time (tsvpp_api.cpp), so libtsvpp.so carries no link-time dependency on it.
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    Roctx();
};
const Roctx &roctx();
struct RangeGuard {
    bool on;
    RangeGuard(bool enabled, const char *label) : on(enabled && roctx().push) {
        if (on) roctx().push(label);
    }
    ~RangeGuard() {
        if (on) roctx().pop();
    }
};

// Device-resident columns of a tsvpp_table, already advanced to the run's first entry (null: the pointer triples travel in the kernarg segment).
struct TableCols {
    const uint64_t *y = nullptr, *uv = nullptr, *out = nullptr;
};

// ---- rules about a request that more than one file applies (inline: the replay hit of tsvpp_api.cpp runs them per conversion) --------------------------
inline int pitch_or_width(int pitch, int width) { return pitch ? pitch : width; } // an unset pitch means the width (reference fallback)

// crop = pointer arithmetic (reference src/Crop.cu:10-18: luma at (left + j, top + i), chroma
// row top/2 + i/2, chroma byte (j & ~1) + left -- an odd `left` therefore swaps U and V,
// exactly as it does in the reference)
struct CropOff { size_t y, uv; };
inline CropOff plane_offsets(int left, int top, int pitch_y, int pitch_uv) {
    return CropOff{ (size_t)top * (size_t)pitch_y + (size_t)left, (size_t)(top / 2) * (size_t)pitch_uv + (size_t)left };
}
inline CropOff crop_offsets(const Plan &pl, int pitch_y, int pitch_uv) { return plane_offsets(pl.off_x, pl.off_y, pitch_y, pitch_uv); }

// The source limit (include/tsvpp.h: TSVPP_SOURCE_SPAN_LIMIT): a region of w x h luma pixels as the kernels see it from the plane addresses advanced to its
// origin -- the crop box, a ROI box, or the whole frame.  (w, h > 0 and even, pitches >= w: the callers have checked.)  The kernels' offsets are unsigned 32-bit
// products (profiles/addressing_limits.txt), the chunked ones counted from up to 15 bytes below the address.
inline bool plane_span_ok(int rows, int pitch, int row_bytes) { return (uint64_t)(rows - 1) * (uint64_t)pitch + (uint64_t)row_bytes < TSVPP_SOURCE_SPAN_LIMIT; }
inline int source_span_status(int w, int h, int pitch_y, int pitch_uv) {
    return plane_span_ok(h, pitch_y, w) && plane_span_ok(h >> 1, pitch_uv, w) ? TSVPP_OK : TSVPP_UNSUPPORTED;
}

// LaunchDesc::in_aligned4 for one frame: `y` / `uv` are its crop-adjusted plane addresses (the bare crop offsets where the frame itself is taken as aligned)
inline bool planes_aligned4(int pitch_y, int pitch_uv, uintptr_t y, uintptr_t uv) { return pitch_y % 4 == 0 && pitch_uv % 4 == 0 && y % 4 == 0 && uv % 4 == 0; }

// Vector-store kernels need 16-byte aligned outputs (else: the element-wise gather kernel); decided per launch group, so one odd pointer does not push a whole
// call onto the element-wise kernel.
inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
inline bool outs_aligned16(void *const *outs, int n) {
    bool vec = true;
    for (int i = 0; i < n; i++) vec = vec && aligned16(outs[i]);
    return vec;
}

// The per-frame checks of a conversion: every pointer set, one geometry, one pair of pitches -- and on the way the alignment class of the call: `aligned4`
// (planes_aligned4 of every frame) and `vec` (every output 16-byte aligned).
inline int check_frames(int n, const tsvpp_nv12 *in, void *const *outs, int w, int h, int pitch_y, int pitch_uv, size_t y_off, size_t uv_off, bool &aligned4, bool &vec) {
    aligned4 = vec = true;
    for (int f = 0; f < n; f++) {
        if (!in[f].y || !in[f].uv || !outs[f]) return TSVPP_ERROR;
        if (in[f].width != w || in[f].height != h) return TSVPP_UNSUPPORTED;
        if (pitch_or_width(in[f].pitch_y, in[f].width) != pitch_y) return TSVPP_UNSUPPORTED;
        if (pitch_or_width(in[f].pitch_uv, in[f].width) != pitch_uv) return TSVPP_UNSUPPORTED;
        aligned4 = aligned4 && planes_aligned4(pitch_y, pitch_uv, (uintptr_t)(in[f].y + y_off), (uintptr_t)(in[f].uv + uv_off));
        vec = vec && aligned16(outs[f]);
    }
    return TSVPP_OK;
}

// What tsvpp_describe, tsvpp_describe_rois and tsvpp_debug_last_launch call a mode and an output flavour (the ROI API uses the first O_COUNT flavours).
inline constexpr const char *mode_names[M_COUNT] = { "none", "nearest", "bilinear", "bicubic", "area_down", "area_up" };
inline constexpr const char *out_names[O_COUNT_ALL] = { "u8_planar", "u8_merged", "f32_planar", "f32_merged", "nv12_u8", "nv12_f32", "y800_u8", "y800_f32", "hsv_f32", "uyvy_u8", "yuv444_u8", "uyvy_f32" };

// ---- functions that cross files ----------------------------------------------------------------------------------------------------------------------
// tsvpp_plan.cpp
int make_plan(const tsvpp_params *p, int in_w, int in_h, Plan &pl);
// (tsvpp_convert* / tsvpp_describe, after make_plan) the rules about the source planes: TSVPP_ERROR for a pitch below the frame's width, TSVPP_UNSUPPORTED for a
// plane span at or above TSVPP_SOURCE_SPAN_LIMIT as seen from the plan's source origin
int plan_source_status(const Plan &pl, int in_w, int pitch_y, int pitch_uv);
int rois_plan(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois, RoiPlan &pl, bool area = false);
// (tsvpp_convert_rois_sized / tsvpp_describe_rois_sized; RoiPlan: dst_w x dst_h stay 0, the sizes are the boxes')
int rois_sized_plan(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi_sized *rois, RoiPlan &pl);
// (tsvpp_convert_letterbox / tsvpp_describe_letterbox; RoiPlan: the canvas is its dst_w x dst_h).  letterbox_rect_of: frame k's rectangle, the caller's or the default
int letterbox_plan(const tsvpp_params *p, int n, const tsvpp_nv12 *in, const tsvpp_rect *rects, int pad_y, int pad_u, int pad_v, RoiPlan &pl);
tsvpp_rect letterbox_rect_of(const tsvpp_nv12 *in, const tsvpp_rect *rects, int k, int dst_w, int dst_h);
// (tsvpp_convert_letterbox_area / tsvpp_describe_letterbox_area; RoiPlan: mode is M_AREA_DOWN -- every frame chooses its rule --, down / taps_x / taps_y as rois_plan's)
int letterbox_area_plan(const tsvpp_params *p, int n, const tsvpp_nv12 *in, const tsvpp_rect *rects, int pad_y, int pad_u, int pad_v, RoiPlan &pl);
// (tsvpp_convert_warp / tsvpp_describe_warp; RoiPlan: mode is M_BILINEAR).  The border is (-1, -1, -1), replicate, or three components 0..255
int warp_plan(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_warps, const tsvpp_warp *warps, int border_y, int border_u, int border_v, RoiPlan &pl,
              Mode filter = M_BILINEAR); // (filter: the one resize type the entry point samples with -- M_BICUBIC for tsvpp_convert_warp_bicubic)
// (tsvpp_convert_perspective / tsvpp_describe_perspective) warp_plan's rules in warp_plan's order, then the horizon rule (include/tsvpp.h)
int persp_plan(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n, const tsvpp_persp *persps, int border_y, int border_u, int border_v, RoiPlan &pl,
               Mode filter = M_BILINEAR);
// (tsvpp_convert_remap / tsvpp_describe_remap) warp_plan's rules in warp_plan's order without the matrix rules, with the maps' (include/tsvpp.h); `xy` is not read
int remap_plan(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_maps, const tsvpp_map *maps, int n, const tsvpp_remap *remaps, int border_y,
               int border_u, int border_v, RoiPlan &pl);
// (tsvpp_convert_mesh / tsvpp_describe_mesh) remap_plan's rules in remap_plan's order with the meshes' rules where the maps' are (include/tsvpp.h); `xy` is not read
int mesh_plan(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_meshes, const tsvpp_mesh *meshes, int n, const tsvpp_remap *remaps, int border_y,
              int border_u, int border_v, RoiPlan &pl);
// (the tensor entry points of both paths) the status of a (params, spec) pair whose plan was accepted: rules 2 and 3 of include/tsvpp.h, in that order
int tensor_spec_status(const tsvpp_params *p, const tsvpp_tensor_spec *spec);
inline size_t tensor_elem_bytes(int dtype) { return dtype == TSVPP_F32 ? 4 : 2; }
// every output aligned to its element
inline bool outs_aligned_to(void *const *outs, int n, size_t elem) {
    for (int i = 0; i < n; i++)
        if ((uintptr_t)outs[i] % elem) return false;
    return true;
}
// out= of the tensor describe calls: `luma_only` for Y800
inline const char *tensor_out_name(int dtype, bool luma_only) {
    if (dtype == TSVPP_F16) return luma_only ? "f16_y800" : "f16_planar";
    if (dtype == TSVPP_BF16) return luma_only ? "bf16_y800" : "bf16_planar";
    return luma_only ? "f32n_y800" : "f32n_planar";
}
// tsvpp_area.cpp: the AREA down-scale fields of a descriptor (nothing for any other mode), out of the context's tables or -- a dry run -- with stand-in pointers
int area_desc(tsvpp_ctx *ctx, const Plan &pl, hipStream_t stream, LaunchDesc &d);
int area_desc(const Knobs &kn, const Plan &pl, LaunchDesc &d);
// tsvpp_api.cpp
void read_env_knobs(Knobs &kn, bool report = false);
int convert_impl(tsvpp_ctx *ctx, int n, const tsvpp_nv12 *in, const tsvpp_params *p, void *const *outs, void *stream, const TableCols &tab);
void clear_last_launch(); // tsvpp_debug_last_launch reports fused launches only: no stale record survives another kind of conversion
// tsvpp_table.cpp
void ctx_release_tables(tsvpp_ctx *ctx);

} // namespace tsvpp
