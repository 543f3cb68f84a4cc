// tsvpp_api.cpp -- host side of the C ABI declared in include/tsvpp.h: contexts, the conversion itself, its dry runs.
//
// Holds what the reference keeps in `class VideoProcessor` (include/VideoProcessor.h:120-149): the per-consumer stream pool and the conversion
// (convert_impl), with the replay of a thread's recent launches in front of it.  No per-frame allocation, free or synchronisation.
// The rest of the host side: tsvpp_plan.cpp (request -> plan), tsvpp_area.cpp (AREA tables), tsvpp_table.cpp (frame tables), tsvpp_rois.cpp (regions of interest).
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "tsvpp_host.h"

using namespace tsvpp;

namespace tsvpp {
thread_local LaunchRecord *g_launch_rec = nullptr;
thread_local bool g_build_declined = false;

// The tracer library is looked up at run time -- rocprofv3's SDK flavour first, the legacy roctracer one second.
Roctx::Roctx() {
    for (const char *name : { "librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4" }) {
        void *h = dlopen(name, RTLD_LAZY | RTLD_GLOBAL);
        if (!h) continue;
        push = (int (*)(const char *))dlsym(h, "roctxRangePushA");
        pop = (int (*)())dlsym(h, "roctxRangePop");
        if (push && pop) return;
        push = nullptr;
        pop = nullptr;
    }
}
const Roctx &roctx() {
    static const Roctx r;
    return r;
}
} // namespace tsvpp

namespace {

// Tuning knobs (profiling / A-B only), read once per context -- and ONLY when TSVPP_DEBUG_KNOBS=1 (round 6, VERDICT r05 #8: until then a release library silently
// obeyed 25 environment variables).  A context created under TSVPP_DEBUG_KNOBS=1 names every knob that differs from its default on stderr, once; a TSVPP_* knob that is
// set WITHOUT the gate is reported once per process and ignored.
// One row per knob: the environment variable that sets it (null: a constant, or set by other means) and the LaunchDesc member it travels in (null: the host
// alone reads it).  read_env_knobs and fill_desc both walk the table, so a knob that has its row is read and forwarded.
template <class T> struct KnobRow {
    const char *env;
    T Knobs::*knob;
    T LaunchDesc::*desc;
};
#define FWD(ENV, NAME) { ENV, &Knobs::NAME, &LaunchDesc::NAME } // a knob that travels under its own name
#define HOST(ENV, NAME) { ENV, &Knobs::NAME, nullptr }
const KnobRow<int> kKnobs[] = {
    FWD("TSVPP_FORCE_GATHER", force_gather), FWD("TSVPP_NT", nt_stores), FWD("TSVPP_DMA", dma), FWD("TSVPP_GEO", geo_pref), FWD("TSVPP_R32", r32_pref),
    FWD("TSVPP_RPT", rpt_pref), FWD("TSVPP_BICUBIC_INT", bicubic_int_pref), FWD("TSVPP_BICUBIC_COLS", bicubic_cols_pref), FWD("TSVPP_BILINEAR_ROWS", bil_rows_pref),
    FWD("TSVPP_BICUBIC_U8X", bc_u8x_pref), FWD("TSVPP_POINT_RN", point_rn_pref), FWD("TSVPP_LDS_KB", lds_budget_kb), FWD("TSVPP_BILINEAR_ROWS_WAVES", br_waves),
    FWD("TSVPP_BICUBIC_ROWS", bc_rows), FWD("TSVPP_AREA_STREAM", area_stream_pref), FWD("TSVPP_BICUBIC_DMA", bc_dma_pref), FWD("TSVPP_AREA_BOX", area_box_pref),
    FWD("TSVPP_BILINEAR_INT", bil_int_pref), HOST("TSVPP_AREA_DIVTAB", area_divtab), FWD("TSVPP_AREA_COLS", area_cols_pref),
    HOST("TSVPP_TAIL_SHIFT", tail_shift), // (travels as LaunchDesc::last_col0: fill_desc)
    FWD("TSVPP_AREA_COLS_ROWS", area_cols_rows), FWD("TSVPP_TILE_ORDER", tile_order), HOST("TSVPP_REPLAY", replay),
    HOST(nullptr, debug), // (the gate TSVPP_DEBUG_KNOBS itself sets it: read_env_knobs)
    FWD(nullptr, shape_tx), FWD(nullptr, shape_ty), // TSVPP_SHAPE=tx,ty sets both (read_env_knobs)
    FWD(nullptr, bil_win_pref), FWD(nullptr, u8_xchg), FWD(nullptr, area2_pref), FWD(nullptr, as_rows), FWD(nullptr, as_min_taps), // constants
};
const KnobRow<float> kFloatKnobs[] = { FWD("TSVPP_AREA_DIRECT_MIN", area_direct_min), FWD(nullptr, area_direct_fmin) };
#undef FWD
#undef HOST

// The part of the launch descriptor that depends only on the request and the knobs.
void fill_desc(const Knobs &kn, GeoCache *geo, const Plan &pl, int pitch_y, int pitch_uv, LaunchDesc &d) {
    std::memset(&d, 0, sizeof(d));
    d.src_w = pl.src_w;
    d.src_h = pl.src_h;
    d.pitch_y = pitch_y;
    d.pitch_uv = pitch_uv;
    d.dst_w = pl.dst_w;
    d.dst_h = pl.dst_h;
    d.xr = pl.xr;
    d.yr = pl.yr;
    d.swap_rb = pl.swap_rb;
    d.point_kind = pl.point_kind;
    d.wx_zero = pl.wx_zero;
    d.wy_zero = pl.wy_zero;
    d.w_dyadic = pl.w_dyadic;
    for (const KnobRow<int> &k : kKnobs)
        if (k.desc) d.*(k.desc) = kn.*(k.knob);
    for (const KnobRow<float> &k : kFloatKnobs) d.*(k.desc) = kn.*(k.knob);
    d.last_col0 = kn.tail_shift ? 0 : -1; // (launch_fused decides; < 0 = not allowed)
    d.k = kn.coeffs;
    d.color_g = kn.color_g;
    d.num_cus = kn.num_cus;
    d.geo_cache = geo;
}

} // namespace

// `report`: name the knobs that took effect on stderr (tsvpp_create; the dry runs of tsvpp_describe / tsvpp_describe_rois stay silent)
void tsvpp::read_env_knobs(Knobs &kn, bool report) {
    const char *gate = std::getenv("TSVPP_DEBUG_KNOBS");
    const bool on = gate && std::atoi(gate) != 0;
    std::string seen;
    auto env = [&](const char *name) { // the variable's value if it is set (and noted), else null
        const char *e = name ? std::getenv(name) : nullptr;
        if (e) seen += std::string(seen.empty() ? "" : " ") + name + "=" + e;
        return e;
    };
    kn.debug = on ? 1 : 0;
    for (const KnobRow<int> &k : kKnobs)
        if (const char *e = env(k.env))
            if (on) kn.*(k.knob) = std::atoi(e);
    for (const KnobRow<float> &k : kFloatKnobs)
        if (const char *e = env(k.env))
            if (on) kn.*(k.knob) = (float)std::atof(e);
    if (const char *e = env("TSVPP_SHAPE"))
        if (on) std::sscanf(e, "%d,%d", &kn.shape_tx, &kn.shape_ty);
    if (seen.empty()) return;
    if (on) {
        if (report) std::fprintf(stderr, "tsvpp: TSVPP_DEBUG_KNOBS=1, this context runs with %s (profiling / A-B settings: parity statements assume the defaults)\n", seen.c_str());
    } else {
        static std::atomic<bool> told{ false };
        if (!told.exchange(true)) std::fprintf(stderr, "tsvpp: ignoring %s (debug knobs are honoured only under TSVPP_DEBUG_KNOBS=1)\n", seen.c_str());
    }
}

namespace {

// The scratch slot of a stream, created on first use; `need` bytes are guaranteed after grow() (caller holds slot->mu).
tsvpp_ctx::ScratchSlot *scratch_slot(tsvpp_ctx *ctx, void *stream) {
    std::lock_guard<std::mutex> lk(ctx->scratch_mu);
    auto &slot = ctx->scratch[stream];
    if (!slot) slot.reset(new tsvpp_ctx::ScratchSlot());
    return slot.get();
}
int scratch_grow(tsvpp_ctx *ctx, tsvpp_ctx::ScratchSlot *slot, size_t need) {
    if (slot->bytes >= need) return TSVPP_OK;
    uint8_t *fresh = nullptr;
    hipError_t e = hipMalloc((void **)&fresh, need);
    if (e != hipSuccess) {
        (void)hipGetLastError(); // reported here: a launcher's `return hipGetLastError()` later on this thread must not find it
        return (int)e;
    }
    if (slot->buf) {
        std::lock_guard<std::mutex> lk(ctx->scratch_mu);
        ctx->retired.push_back(slot->buf);
    }
    slot->buf = fresh;
    slot->bytes = need;
    return TSVPP_OK;
}
size_t scratch_frame_bytes(const Plan &pl) { return (((size_t)pl.dst_w * pl.dst_h * 3 / 2) + 255) & ~(size_t)255; }
// Bytes one frame of this request moves, roughly: the output + the source rows its sampler taps (a point sampler at vertical ratio r reads every r-th row,
// the 2-tap kernels two of every r, BICUBIC four: C4's 4K -> 720p point sample 6.9 MB where the ROI formula says 15.2; PMC: 6.91 MB).  Only used to decide whether a
// launch is small enough to overlap its predecessor (TSVPP_BARRIER_FREE_MAX_BYTES).
size_t plan_moved_bytes(const Plan &pl) {
    double rows = 1.0;
    if (pl.yr > 1.0f) {
        if (pl.mode == M_NEAREST || pl.point_kind != PK_NONE) rows = 1.0 / pl.yr;
        else if (pl.mode == M_BILINEAR || pl.mode == M_AREA_UP) rows = 2.0 / pl.yr;
        else if (pl.mode == M_BICUBIC) rows = 4.0 / pl.yr;
    }
    if (rows > 1.0) rows = 1.0;
    return pl.out_bytes + (size_t)((double)pl.src_w * pl.src_h * 1.5 * rows);
}

bool needs_scratch(const Plan &pl) { return (pl.fourcc == TSVPP_UYVY || pl.fourcc == TSVPP_YUV444) && pl.mode != M_NONE; }

// A by-value frame table of n frames (only the first n triples and the three ext / off pairs are ever read).
inline void fill_frames(FrameTable &t, const tsvpp_nv12 *in, void *const *outs, int n, size_t y_off, size_t uv_off) {
    t.y.ext = nullptr; t.y.off = 0;
    t.uv.ext = nullptr; t.uv.off = 0;
    t.out.ext = nullptr; t.out.off = 0;
    for (int f = 0; f < n; f++) {
        t.y[f] = in[f].y + y_off;
        t.uv[f] = in[f].uv + uv_off;
        t.out[f] = outs[f];
    }
}

OutKind single_pass_kind(const Plan &pl) { return pl.fourcc == TSVPP_UYVY ? (pl.f32 ? O_UYVY_F32 : O_UYVY_U8) : O_YUV444_U8; }
// UYVY / YUV444 (uint8; UYVY also fp32) behind a resize: does the streaming kernel take it (exact 3 : 2 or 2 : 1, BILINEAR / AREA / NEAREST, dword-aligned planes,
// width % 8 == 0, height % 4 == 0, 16-byte aligned outputs)?  Asked of launch_fused itself, as a dry run: one set of conditions.
bool single_pass_format(const Plan &pl, OutKind kind, const LaunchDesc &d, int n, bool vec, hipStream_t stream) {
    if ((pl.fourcc != TSVPP_UYVY && pl.fourcc != TSVPP_YUV444) || (pl.f32 && pl.fourcc != TSVPP_UYVY) || pl.mode == M_NONE || !vec) return false; // (fp32: UYVY only, round 6)
    LaunchDesc dd = d;
    dd.n_frames = n < TSVPP_MAX_BATCH ? (n > 0 ? n : 1) : TSVPP_MAX_BATCH;
    FrameTable t = {};
    LaunchInfo info = {};
    return launch_fused(pl.mode, kind, true, dd, t, stream, &info) == hipSuccess;
}

// The decisions of a request beyond its plan, taken once for a conversion, for tsvpp_describe and for the dry run of tsvpp_prepare_batch.  `d` comes from
// fill_desc (+ area_desc) and leaves with in_aligned4 and the store override set.
// Formats other than RGB24/BGR24: the reference feeds its other colour kernels with
// the resized NV12; here pass 1 (only if there is a resize) writes that intermediate with the
// fused kernel, pass 2 converts it.  Crop alone needs no pass 1: it is pointer arithmetic.
// ... unless the streaming 3 : 2 / 2 : 1 kernel takes the request: it writes UYVY / YUV444 (uint8) itself, in one pass (vpp_bilinear_r32.hip)
struct Resolved {
    bool two_pass;    // UYVY / YUV444 as a second pass (launch_format) over NV12, not out of the streaming kernel in one
    bool pass1;       // a fused launch runs (not for crop + format conversion: the second pass alone)
    OutKind out_kind; // its output flavour
};
Resolved resolve_request(const Plan &pl, LaunchDesc &d, int n, bool aligned4, bool vec, hipStream_t stream) {
    d.in_aligned4 = aligned4 ? 1 : 0;
    const OutKind kind1 = single_pass_kind(pl);
    const bool single = single_pass_format(pl, kind1, d, n, vec, stream);
    const bool two_pass = (pl.fourcc == TSVPP_UYVY || pl.fourcc == TSVPP_YUV444) && !single;
    if (two_pass && d.nt_stores < 0) d.nt_stores = 0; // the intermediate is read back at once: keep it in L2 / MALL
    return Resolved{ two_pass, !(two_pass && pl.mode == M_NONE), single ? kind1 : pl.out };
}

// ---- replay of a thread's recent launches (round 6) ---------------------------------------------------------------------------------------------------
// A conversion of ONE frame is host-bound: ~3.3 us of runtime per launch (tools/launch_cost.hip: 3.5 us with this library's 3.7 KiB kernarg segment, 2.65 with a
// 16-byte one) plus what this file adds -- make_plan, fill_desc, launch_fused's selection, the table caches' mutexes and map lookups.  The latter is the same work for
// every frame a consumer converts, so a thread keeps the FINISHED launches (host function, grid, final LaunchDesc) of its last eight requests and replays one when
// the request, the frame geometry, the alignment class of the pointers, the context and its epoch all match.  Only single-launch requests are kept (no second
// pass, no row-tail launch, no frame table, at most TSVPP_MAX_BATCH frames); TSVPP_REPLAY=0 disables it (the GPU suite is replayed both ways).
// A hit is convert_impl -> try_replay -> check_frames -> DeviceGuard -> launch: all of it in this file or inline in tsvpp_host.h.
struct ReplayEntry {
    uint64_t ctx_id = 0, epoch = 0, stamp = 0;
    tsvpp_params p = {};
    int w = 0, h = 0, py = 0, puv = 0, n = 0;
    bool aligned4 = false, vec = false;
    size_t y_off = 0, uv_off = 0;
    LaunchRecord rec;
};
constexpr int kReplayEntries = 8;
constexpr int kReplayMiss = -1000;
thread_local ReplayEntry g_replay[kReplayEntries];
thread_local uint64_t g_replay_clock = 0;
// tsvpp_debug_last_launch: the record of this thread's last conversion, if it ran in a context created under TSVPP_DEBUG_KNOBS=1 -- a replay slot's (replayed or
// just remembered) or a copy of a record that is not replayable (several launches, a second pass, a frame table); null otherwise.  Every conversion clears it first.
// What that costs every conversion: two thread-local pointer stores, three int stores into the launch record, and in each launcher one thread-local load
// (describe_only) -- the record itself is only armed where the replay cache arms it anyway, or in a debug context.
thread_local const LaunchRecord *g_last_launch = nullptr;
thread_local LaunchRecord g_last_copy;
struct RecordArm { // points launch_fused's launches at `rec` for the lifetime of this object
    explicit RecordArm(LaunchRecord *rec) { g_launch_rec = rec; }
    ~RecordArm() { g_launch_rec = nullptr; }
};

int try_replay(tsvpp_ctx *ctx, int n, const tsvpp_nv12 *in, const tsvpp_params *p, void *const *outs, void *stream) {
    const uint64_t epoch = ctx->epoch.load(std::memory_order_acquire); // (a plain load on x86)
    const int py = pitch_or_width(in[0].pitch_y, in[0].width), puv = pitch_or_width(in[0].pitch_uv, in[0].width);
    bool classed = false, aligned4 = false, vec = false; // alignment class of THIS call, computed once (every entry of one request has the same crop offsets)
    for (int k = 0; k < kReplayEntries; k++) {
        ReplayEntry &e = g_replay[k];
        if (e.ctx_id != ctx->id || e.epoch != epoch || e.n != n || e.w != in[0].width || e.h != in[0].height || e.py != py || e.puv != puv ||
            std::memcmp(&e.p, p, sizeof(*p)) != 0)
            continue;
        if (!classed) {
            const int sts = check_frames(n, in, outs, in[0].width, in[0].height, py, puv, e.y_off, e.uv_off, aligned4, vec);
            if (sts != TSVPP_OK) return sts;
            classed = true;
        }
        if (e.aligned4 != aligned4 || e.vec != vec) continue;
        DeviceGuard guard(ctx);
        if (guard.status != TSVPP_OK) return guard.status;
        FrameTable t;
        fill_frames(t, in, outs, n, e.y_off, e.uv_off);
        void *args[2] = { (void *)&e.rec.d, (void *)&t };
        const hipError_t err = e.rec.d.any_order
                                   ? hipExtLaunchKernel(e.rec.fn, e.rec.grid, e.rec.block, args, e.rec.lds, (hipStream_t)stream, nullptr, nullptr, hipExtAnyOrderLaunch)
                                   : hipLaunchKernel(e.rec.fn, e.rec.grid, e.rec.block, args, e.rec.lds, (hipStream_t)stream);
        e.stamp = ++g_replay_clock;
        if (err == hipSuccess && ctx->knobs.debug) g_last_launch = &e.rec;
        return (int)err;
    }
    return kReplayMiss;
}

const LaunchRecord *remember_launch(const tsvpp_ctx *ctx, uint64_t epoch, int n, const tsvpp_nv12 *in, const tsvpp_params *p, int py, int puv, bool aligned4, bool vec, size_t y_off,
                     size_t uv_off, const LaunchRecord &rec) {
    ReplayEntry *slot = &g_replay[0];
    for (ReplayEntry &e : g_replay)
        if (e.stamp < slot->stamp) slot = &e;
    slot->ctx_id = ctx->id;
    slot->epoch = epoch;
    slot->stamp = ++g_replay_clock;
    slot->p = *p;
    slot->w = in[0].width;
    slot->h = in[0].height;
    slot->py = py;
    slot->puv = puv;
    slot->n = n;
    slot->aligned4 = aligned4;
    slot->vec = vec;
    slot->y_off = y_off;
    slot->uv_off = uv_off;
    slot->rec = rec;
    return &slot->rec;
}

// Index of the consumer's pool slot (claiming a free one for a new name), or -1 (caller holds stream_mu).
int consumer_slot(tsvpp_ctx *ctx, const char *name) {
    for (size_t i = 0; i < ctx->streams.size(); i++) {
        auto &s = ctx->streams[i];
        if (s.first == name) return (int)i;
        if (s.first == "empty") {
            s.first = name;
            return (int)i;
        }
    }
    return -1;
}

// The answer of tsvpp_describe / tsvpp_debug_last_launch: one line of key=value pairs.
void format_selection(char *buf, size_t buf_len, int mode, int out, int src_w, int src_h, int dst_w, int dst_h, const LaunchInfo &info, int frames, int pass2) {
    char kname[128]; // the launcher's spelling without blanks: one token per key=value pair
    size_t kn = 0;
    for (const char *c = info.kernel ? info.kernel : "(unnamed)"; *c && kn + 1 < sizeof(kname); c++)
        if (*c != ' ') kname[kn++] = *c;
    kname[kn] = 0;
    std::snprintf(buf, buf_len, "mode=%s out=%s src=%dx%d dst=%dx%d kernel=%s shape=%dx%d rpt=%d dma=%d lds=%d grid=%d tiles=%dx%d frames=%d tail=%d geo=%d nt=%d staged=%d in4=%d%s",
                  mode_names[mode], out_names[out], src_w, src_h, dst_w, dst_h, kname, info.tx, info.ty, info.rpt, info.dma, info.lds_bytes, info.grid, info.tiles_x,
                  info.tiles_y, frames, info.tail, info.geo, info.nt, info.staged, info.in4,
                  pass2 ? (pass2 == TSVPP_UYVY ? " pass2=fmt_uyvy" : " pass2=fmt_yuv444") : "");
}

} // namespace

void tsvpp::clear_last_launch() { g_last_launch = nullptr; }

// tsvpp_convert_batch and tsvpp_convert_table: `in` / `outs` are HOST arrays of the n frames (a table's pinned mirror for the latter).
int tsvpp::convert_impl(tsvpp_ctx *ctx, int n, const tsvpp_nv12 *in, const tsvpp_params *p, void *const *outs, void *stream, const TableCols &tab) {
    g_last_launch = nullptr; // (tsvpp_debug_last_launch: no stale record survives a conversion that records none)
    if (!ctx || !in || !p || !outs || n < 0) return TSVPP_ERROR;
    if (n == 0) return TSVPP_OK;
    g_build_declined = false;
    // The epoch first, every option after it (OptInt, tsvpp_host.h).  tsvpp_set_option stores the value before it moves the epoch, so a launch built from newer
    // options than `epoch0` stands for is remembered under an epoch that is already past -- never replayed -- and one built from older options cannot be.
    const uint64_t epoch0 = ctx->epoch.load(std::memory_order_acquire);
    const bool replayable = ctx->knobs.replay && tab.y == nullptr && n <= TSVPP_MAX_BATCH && !ctx->markers;
    if (replayable) { // the same request as one of this thread's recent ones: its finished launch again, with this call's frame pointers
        const int r = try_replay(ctx, n, in, p, outs, stream);
        if (r != kReplayMiss) return r;
    }
    Plan pl;
    int sts = make_plan(p, in[0].width, in[0].height, pl);
    if (sts != TSVPP_OK) return sts;
    const int pitch_y = pitch_or_width(in[0].pitch_y, in[0].width), pitch_uv = pitch_or_width(in[0].pitch_uv, in[0].width);
    sts = plan_source_status(pl, in[0].width, pitch_y, pitch_uv);
    if (sts != TSVPP_OK) return sts;
    // dst_w is even; when it is 4 k + 2 launch_fused shifts the launch's last tile column to the frame's right edge (or, where it cannot, the
    // vector-store kernels skip the two-column tail of every row and a tiny element-wise launch converts it); rows then start 8 bytes / 2 bytes
    // off the vector alignment, which global stores tolerate.
    // (alignment is decided per launch group of TSVPP_MAX_BATCH frames below: one odd pointer does not push the
    // whole batch onto the element-wise kernel)
    const CropOff off = crop_offsets(pl, pitch_y, pitch_uv);
    bool aligned4, all_vec;
    sts = check_frames(n, in, outs, in[0].width, in[0].height, pitch_y, pitch_uv, off.y, off.uv, aligned4, all_vec);
    if (sts != TSVPP_OK) return sts;
    DeviceGuard guard(ctx);
    if (guard.status != TSVPP_OK) return guard.status;
    char label[96] = "";
    const bool markers = ctx->markers != 0; // read once: a concurrent tsvpp_enable_markers cannot push an unformatted label
    if (markers)
        std::snprintf(label, sizeof(label), "tsvpp_convert n=%d %dx%d->%dx%d mode=%d fourcc=%d stream=%p", n, pl.src_w, pl.src_h, pl.dst_w, pl.dst_h,
                      (int)pl.mode, pl.fourcc, stream);
    RangeGuard range(markers, label);

    LaunchDesc d;
    fill_desc(ctx->knobs, ctx->geo, pl, pitch_y, pitch_uv, d);
    sts = area_desc(ctx, pl, (hipStream_t)stream, d);
    if (sts != TSVPP_OK) return sts;
    const Resolved rq = resolve_request(pl, d, n, aligned4, all_vec, (hipStream_t)stream);
    uint8_t *scratch = nullptr;
    size_t frame_scratch = 0;
    std::unique_lock<std::mutex> scratch_lock; // held until both passes of this call are enqueued
    if (needs_scratch(pl) && rq.two_pass) {
        frame_scratch = scratch_frame_bytes(pl);
        tsvpp_ctx::ScratchSlot *slot = scratch_slot(ctx, stream);
        scratch_lock = std::unique_lock<std::mutex>(slot->mu);
        // sized by tsvpp_prepare_batch: then this is a no-op; otherwise the first call for a (size, n) pays one hipMalloc
        sts = scratch_grow(ctx, slot, frame_scratch * (size_t)n);
        if (sts != TSVPP_OK) return sts;
        scratch = slot->buf;
    }
    // Frames per launch: TSVPP_MAX_BATCH with the pointer triples in the kernarg segment; out of a device-resident table (single-pass requests) up to
    // TSVPP_MAX_TABLE_LAUNCH, less where the grid would outgrow 2^31 threads (the smallest tile any kernel uses is 64 x 4 output pixels per workgroup of 256).
    const bool from_table = tab.y != nullptr && !rq.two_pass;
    // TSVPP_OPT_INPUTS_READY: never out of a table (tsvpp_table_set's upload is enqueued on this stream: the launch must wait for it), never for the two-pass
    // formats (pass 1 writes the stream's scratch buffer, which the previous call's pass 2 may still be reading)
    // ... and only for launches small enough to gain from starting beside their predecessor: measured on the headline (profiles/r06_curve_values.txt, one consumer on two
    // streams) 1 / 2 / 4 frames per launch 0.367 / 0.573 / 0.661 -> 0.410 / 0.583 / 0.682 of the roofline, but 8 frames (113 MB) 0.719 -> 0.682
    const int inputs_ready = ctx->inputs_ready; // read once
    d.any_order = ((inputs_ready == 1 || inputs_ready == 2) && tab.y == nullptr && !rq.two_pass &&
                   (size_t)n * plan_moved_bytes(pl) <= TSVPP_BARRIER_FREE_MAX_BYTES) ? 1 : 0;
    int max_launch = TSVPP_MAX_BATCH;
    if (from_table) {
        const long wg_per_frame = (long)((pl.dst_w + 63) / 64) * ((pl.dst_h + 3) / 4);
        long cap = ((1L << 31) / 256) / (wg_per_frame > 0 ? wg_per_frame : 1);
        if (cap > TSVPP_MAX_TABLE_LAUNCH) cap = TSVPP_MAX_TABLE_LAUNCH;
        if (cap > TSVPP_MAX_BATCH) max_launch = (int)cap;
    }
    const bool to_scratch = rq.two_pass && pl.mode != M_NONE; // pass 1 writes the resized NV12 intermediate, pass 2 reads it
    for (int base = 0; base < n; base += max_launch) {
        const int cnt = (n - base < max_launch) ? n - base : max_launch;
        FrameTable t = {};
        if (from_table) {
            t.y.ext = (const uint8_t *const *)(tab.y + base);
            t.y.off = (int64_t)off.y;
            t.uv.ext = (const uint8_t *const *)(tab.uv + base);
            t.uv.off = (int64_t)off.uv;
            t.out.ext = (void *const *)(tab.out + base);
            t.out.off = 0;
        } else {
            fill_frames(t, in + base, outs + base, cnt, off.y, off.uv);
            if (to_scratch)
                for (int f = 0; f < cnt; f++) t.out[f] = scratch + (size_t)(base + f) * frame_scratch;
        }
        d.n_frames = cnt;
        const bool vec = rq.two_pass || outs_aligned16(outs + base, cnt); // (scratch frames are 256-byte aligned)
        if (rq.pass1) {
            LaunchRecord rec;
            rec.mode = pl.mode;
            rec.out = rq.out_kind;
            rec.pass2 = rq.two_pass ? pl.fourcc : 0;
            const bool keep = replayable && !rq.two_pass && n <= max_launch; // one launch group, one pass
            hipError_t e;
            {
                RecordArm arm((keep || ctx->knobs.debug) ? &rec : nullptr);
                e = launch_fused(pl.mode, rq.out_kind, vec, d, t, (hipStream_t)stream);
            }
            if (e != hipSuccess) {
                g_last_launch = nullptr; // (an earlier launch group's record does not describe a failed conversion)
                return (int)e;
            }
            // (a launch that fell back because a capturing stream kept a table from being built is right for this call and wrong to remember: the next ordinary
            // call builds the table)
            if (keep && rec.count == 1 && rec.fn && !g_build_declined) {
                const LaunchRecord *kept = remember_launch(ctx, epoch0, n, in, p, pitch_y, pitch_uv, aligned4, vec, off.y, off.uv, rec);
                if (ctx->knobs.debug) g_last_launch = kept;
            } else if (ctx->knobs.debug && rec.count > 0) { // (count == 0: nothing was launched, and rec.d was never written)
                g_last_copy = rec;
                g_last_launch = &g_last_copy;
            } else {
                g_last_launch = nullptr;
            }
        } else if (ctx->knobs.debug) { // crop + format conversion: the second pass alone
            g_last_copy = LaunchRecord();
            g_last_copy.name = "(none)";
            g_last_copy.mode = pl.mode;
            g_last_copy.out = rq.out_kind;
            g_last_copy.pass2 = pl.fourcc;
            g_last_copy.d.in_aligned4 = aligned4 ? 1 : 0;
            g_last_copy.d.n_frames = cnt;
            g_last_launch = &g_last_copy;
        }
        if (rq.two_pass) {
            int fpy = pitch_y, fpuv = pitch_uv;
            if (to_scratch) { // resized intermediate: tight, pitch = width (as the reference's)
                for (int f = 0; f < cnt; f++) {
                    t.y[f] = scratch + (size_t)(base + f) * frame_scratch;
                    t.uv[f] = t.y[f] + (size_t)pl.dst_w * pl.dst_h;
                    t.out[f] = outs[base + f];
                }
                fpy = fpuv = pl.dst_w;
            }
            hipError_t e = launch_format(pl.fourcc, pl.f32, t, cnt, fpy, fpuv, pl.dst_w, pl.dst_h, (hipStream_t)stream);
            if (e != hipSuccess) {
                g_last_launch = nullptr;
                return (int)e;
            }
        }
    }
    return TSVPP_OK;
}

extern "C" {

void tsvpp_default_coeffs(tsvpp_coeffs *k) {
    if (!k) return;
    k->y_scale = 1.163999557f;
    k->v_to_r = 1.5959997177f;
    k->u_to_b = 2.017999649f;
    k->v_to_g = -0.812999725f;
    k->u_to_g = -0.390999794f;
    k->round_bias = 0.5f;
    k->y_offset = 16.0f;
    k->c_offset = 128.0f;
}

int tsvpp_create(int device, int max_consumers, tsvpp_ctx **out_ctx) {
    if (!out_ctx || max_consumers < 0) return TSVPP_ERROR;
    *out_ctx = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess) return (int)e;
    if (device < 0 || device >= count) return (int)hipErrorInvalidDevice;
    tsvpp_ctx *ctx = new tsvpp_ctx();
    static std::atomic<uint64_t> next_id{ 1 };
    ctx->id = next_id.fetch_add(1);
    ctx->device = device;
    DeviceGuard guard(ctx);
    if (guard.status != TSVPP_OK) {
        delete ctx;
        return guard.status;
    }
    read_env_knobs(ctx->knobs, true);
    ctx->geo = geo_cache_create();
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ctx->knobs.num_cus = prop.multiProcessorCount;
    }
    for (int i = 0; i < max_consumers; i++) {
        hipStream_t s = nullptr;
        e = hipStreamCreate(&s); // blocking stream, as the reference (src/VideoProcessor.cpp:86)
        if (e != hipSuccess) {
            (void)hipGetLastError();
            for (auto &st : ctx->streams)
                if (st.second) (void)hipStreamDestroy(st.second);
            geo_cache_destroy(ctx->geo);
            delete ctx;
            return (int)e;
        }
        ctx->streams.emplace_back(std::string("empty"), s);
    }
    ctx->streams2.assign(ctx->streams.size(), nullptr);
    ctx->turn.assign(ctx->streams.size(), 0);
    *out_ctx = ctx;
    return TSVPP_OK;
}

void tsvpp_destroy(tsvpp_ctx *ctx) {
    if (!ctx) return;
    {
        DeviceGuard guard(ctx);
        ctx_release_tables(ctx);
        for (auto &s : ctx->streams)
            if (s.second) (void)hipStreamDestroy(s.second);
        for (hipStream_t s : ctx->streams2)
            if (s) (void)hipStreamDestroy(s);
        for (auto &sc : ctx->scratch)
            if (sc.second && sc.second->buf) (void)hipFree(sc.second->buf);
        for (uint8_t *b : ctx->retired) (void)hipFree(b);
        for (auto &a : ctx->area) {
            if (a.second.dev) (void)hipFree(a.second.dev);
            if (a.second.qdev) (void)hipFree(a.second.qdev);
            if (a.second.dev4) (void)hipFree(a.second.dev4);
        }
        for (auto &a : ctx->area_div)
            if (a.second) (void)hipFree(a.second);
        geo_cache_destroy(ctx->geo);
        ctx->geo = nullptr;
    }
    delete ctx;
}

int tsvpp_consumer_stream(tsvpp_ctx *ctx, const char *name, void **out_stream) {
    if (!ctx || !name || !out_stream) return TSVPP_ERROR;
    std::lock_guard<std::mutex> lk(ctx->stream_mu);
    const int i = consumer_slot(ctx, name);
    *out_stream = i < 0 ? nullptr : (void *)ctx->streams[(size_t)i].second;
    return i < 0 ? TSVPP_ERROR : TSVPP_OK; // pool exhausted (reference src/VideoProcessor.cpp:100-103)
}

int tsvpp_consumer_next_stream(tsvpp_ctx *ctx, const char *name, size_t launch_bytes, void **out_stream) {
    if (!ctx || !name || !out_stream) return TSVPP_ERROR;
    *out_stream = nullptr;
    std::lock_guard<std::mutex> lk(ctx->stream_mu);
    const int i = consumer_slot(ctx, name);
    if (i < 0) return TSVPP_ERROR; // pool exhausted (reference src/VideoProcessor.cpp:100-103)
    const int inputs_ready = ctx->inputs_ready;
    if (!(inputs_ready == 1 || inputs_ready == 3) || launch_bytes > TSVPP_OVERLAP_MAX_BYTES) { // (large launches do not overlap: see the header)
        *out_stream = (void *)ctx->streams[(size_t)i].second;
        return TSVPP_OK;
    }
    if (!ctx->streams2[(size_t)i]) {
        DeviceGuard guard(ctx);
        if (guard.status != TSVPP_OK) return guard.status;
        hipStream_t s = nullptr;
        const hipError_t e = hipStreamCreate(&s); // blocking, as the pool's first stream
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return (int)e;
        }
        ctx->streams2[(size_t)i] = s;
    }
    const uint8_t t = ctx->turn[(size_t)i];
    ctx->turn[(size_t)i] = t ^ 1;
    *out_stream = (void *)(t ? ctx->streams2[(size_t)i] : ctx->streams[(size_t)i].second);
    return TSVPP_OK;
}

int tsvpp_consumer_synchronize(tsvpp_ctx *ctx, const char *name) {
    if (!ctx || !name) return TSVPP_ERROR;
    hipStream_t a = nullptr, b = nullptr;
    {
        std::lock_guard<std::mutex> lk(ctx->stream_mu);
        int i = -1;
        for (size_t k = 0; k < ctx->streams.size(); k++)
            if (ctx->streams[k].first == name) i = (int)k;
        if (i < 0) return TSVPP_ERROR; // no such consumer
        a = ctx->streams[(size_t)i].second;
        b = ctx->streams2[(size_t)i];
    }
    DeviceGuard guard(ctx);
    if (guard.status != TSVPP_OK) return guard.status;
    hipError_t e = hipStreamSynchronize(a);
    if (e == hipSuccess && b) e = hipStreamSynchronize(b);
    return (int)e;
}

int tsvpp_prepare_batch(tsvpp_ctx *ctx, const tsvpp_params *p, int in_width, int in_height, int n_frames, void *stream) {
    if (!ctx || n_frames < 0) return TSVPP_ERROR;
    Plan pl;
    int sts = make_plan(p, in_width, in_height, pl);
    if (sts != TSVPP_OK) return sts;
    DeviceGuard guard(ctx);
    if (guard.status != TSVPP_OK) return guard.status;
    LaunchDesc d;
    const int pitch = (in_width + 255) & ~255;
    fill_desc(ctx->knobs, ctx->geo, pl, pitch, pitch, d);
    sts = area_desc(ctx, pl, (hipStream_t)stream, d);
    if (sts != TSVPP_OK) return sts;
    if (needs_scratch(pl) && n_frames > 0) { // the NV12 intermediate of UYVY / YUV444 behind a resize
        tsvpp_ctx::ScratchSlot *slot = scratch_slot(ctx, stream);
        std::lock_guard<std::mutex> lk(slot->mu);
        sts = scratch_grow(ctx, slot, scratch_frame_bytes(pl) * (size_t)n_frames);
        if (sts != TSVPP_OK) return sts;
    }
    if (((pl.mode == M_BILINEAR || pl.mode == M_AREA_UP) && ctx->knobs.geo_pref) || (pl.mode == M_BICUBIC && ctx->knobs.bicubic_cols_pref)) {
        // geometry tables of the 2x2-tap kernel: a dry run of the launch chooses the tile shape and builds them.  They do not
        // depend on the pitches (only their use does: multiples of 16) nor on the batch size beyond the tile shape -- a
        // conversion that ends up with another shape builds its own set on first use.
        const int total = n_frames > 0 ? n_frames : 1;
        // (the outputs are unknown: UYVY / YUV444 are prepared as the two passes they may need -- pass 1 reads tables, the single-pass kernel none)
        const Resolved rq = resolve_request(pl, d, total, true, false, (hipStream_t)stream);
        d.geo_build = 1;
        FrameTable t = {};
        // the launch groups tsvpp_convert_batch forms: full groups of TSVPP_MAX_BATCH frames, then the remainder; and, for more frames than that, the groups
        // tsvpp_convert_table forms (up to TSVPP_MAX_TABLE_LAUNCH per launch; a launch the grid limit caps lower builds its tables on first use)
        const int groups[4] = { total >= TSVPP_MAX_BATCH ? TSVPP_MAX_BATCH : 0, total % TSVPP_MAX_BATCH,
                                total > TSVPP_MAX_BATCH ? (total < TSVPP_MAX_TABLE_LAUNCH ? total : TSVPP_MAX_TABLE_LAUNCH) : 0,
                                total > TSVPP_MAX_TABLE_LAUNCH ? total % TSVPP_MAX_TABLE_LAUNCH : 0 };
        for (int cnt : groups) {
            if (cnt == 0) continue;
            d.n_frames = cnt;
            LaunchInfo info = {};
            hipError_t e = launch_fused(pl.mode, rq.out_kind, true, d, t, (hipStream_t)stream, &info);
            if (e != hipSuccess) return (int)e;
        }
    }
    return sts;
}

int tsvpp_prepare(tsvpp_ctx *ctx, const tsvpp_params *p, int in_width, int in_height) {
    return tsvpp_prepare_batch(ctx, p, in_width, in_height, 0, nullptr);
}

int tsvpp_enable_markers(tsvpp_ctx *ctx, int on) {
    if (!ctx) return TSVPP_ERROR;
    if (on && !roctx().push) return TSVPP_UNSUPPORTED; // no roctx library on this machine
    ctx->markers = on ? 1 : 0;
    ctx->epoch.fetch_add(1);
    return TSVPP_OK;
}

int tsvpp_convert_batch(tsvpp_ctx *ctx, int n, const tsvpp_nv12 *in, const tsvpp_params *p, void *const *outs, void *stream) {
    return convert_impl(ctx, n, in, p, outs, stream, TableCols());
}

int tsvpp_convert(tsvpp_ctx *ctx, const tsvpp_nv12 *in, const tsvpp_params *p, void *out, void *stream) {
    void *outs[1] = { out };
    return tsvpp_convert_batch(ctx, 1, in, p, outs, stream);
}

int tsvpp_trim(tsvpp_ctx *ctx, size_t *released_bytes) {
    if (released_bytes) *released_bytes = 0;
    if (!ctx) return TSVPP_ERROR;
    DeviceGuard guard(ctx);
    if (guard.status != TSVPP_OK) return guard.status;
    ctx->epoch.fetch_add(1); // replay records may hold the addresses of retired table sets
    size_t n = geo_cache_trim(ctx->geo);
    {
        std::lock_guard<std::mutex> lk(ctx->scratch_mu);
        for (uint8_t *b : ctx->retired) (void)hipFree(b); // outgrown NV12 scratch buffers of the two-pass formats (their sizes are not tracked: not counted)
        ctx->retired.clear();
    }
    if (released_bytes) *released_bytes = n;
    return TSVPP_OK;
}

int tsvpp_set_option(tsvpp_ctx *ctx, int option, int value) {
    if (!ctx) return TSVPP_ERROR;
    switch (option) {
    case TSVPP_OPT_UNSAFE_COEFFS:
        ctx->unsafe_coeffs = value ? 1 : 0;
        return TSVPP_OK;
    case TSVPP_OPT_COLOR_G_TERM:
        if (value < 0 || value > 2) return TSVPP_ERROR;
        ctx->knobs.color_g = value;
        ctx->epoch.fetch_add(1);
        return TSVPP_OK;
    case TSVPP_OPT_INPUTS_READY:
        if (value < 0 || value > 3) return TSVPP_ERROR;
        ctx->inputs_ready = value;
        ctx->epoch.fetch_add(1);
        return TSVPP_OK;
    default: return TSVPP_UNSUPPORTED;
    }
}

int tsvpp_get_option(const tsvpp_ctx *ctx, int option, int *value) {
    if (!ctx || !value) return TSVPP_ERROR;
    switch (option) {
    case TSVPP_OPT_INPUTS_READY: *value = ctx->inputs_ready; return TSVPP_OK;
    case TSVPP_OPT_COLOR_G_TERM: *value = ctx->knobs.color_g; return TSVPP_OK;
    case TSVPP_OPT_UNSAFE_COEFFS: *value = ctx->unsafe_coeffs; return TSVPP_OK;
    default: return TSVPP_UNSUPPORTED;
    }
}

int tsvpp_get_coeffs(const tsvpp_ctx *ctx, tsvpp_coeffs *out) {
    if (!ctx || !out) return TSVPP_ERROR;
    *out = ctx->knobs.coeffs;
    return TSVPP_OK;
}

int tsvpp_set_coeffs(tsvpp_ctx *ctx, const tsvpp_coeffs *in) {
    if (!ctx || !in) return TSVPP_ERROR;
    // Every parity statement of this library is about the reference's literals (reference src/ColorConversion.cu:23-36).  A block that differs from them -- by a bit --
    // is refused unless the caller has said it wants one; the multi-GPU broadcast sets the block it verified against the defaults, which passes.
    tsvpp_coeffs def;
    tsvpp_default_coeffs(&def);
    if (std::memcmp(&def, in, sizeof(def)) != 0 && !ctx->unsafe_coeffs) return TSVPP_UNSUPPORTED;
    ctx->knobs.coeffs = *in;
    ctx->epoch.fetch_add(1);
    return TSVPP_OK;
}

int tsvpp_describe(const tsvpp_params *p, int in_width, int in_height, int pitch_y, int pitch_uv, int n_frames, int aligned_outputs, char *buf,
                   size_t buf_len) {
    if (!p || !buf || buf_len == 0) return TSVPP_ERROR;
    buf[0] = 0;
    Plan pl;
    int sts = make_plan(p, in_width, in_height, pl);
    if (sts != TSVPP_OK) return sts;
    pitch_y = pitch_or_width(pitch_y, in_width);
    pitch_uv = pitch_or_width(pitch_uv, in_width);
    if (n_frames < 1) return TSVPP_ERROR;
    sts = plan_source_status(pl, in_width, pitch_y, pitch_uv);
    if (sts != TSVPP_OK) return sts;
    Knobs kn; // no context: no device, no streams
    read_env_knobs(kn);
    LaunchDesc d;
    fill_desc(kn, nullptr, pl, pitch_y, pitch_uv, d);
    sts = area_desc(kn, pl, d);
    if (sts != TSVPP_OK) return sts;
    // frame pointers are assumed 256-byte aligned; the crop origin decides the rest
    const CropOff off = crop_offsets(pl, pitch_y, pitch_uv);
    const Resolved rq = resolve_request(pl, d, n_frames, planes_aligned4(pitch_y, pitch_uv, off.y, off.uv), aligned_outputs != 0, nullptr);
    d.n_frames = n_frames < TSVPP_MAX_BATCH ? n_frames : TSVPP_MAX_BATCH;
    LaunchInfo info = {};
    info.kernel = "(none)";
    info.in4 = d.in_aligned4;
    if (rq.pass1) {
        FrameTable t = {};
        hipError_t e = launch_fused(pl.mode, rq.out_kind, aligned_outputs != 0 || rq.two_pass, d, t, nullptr, &info);
        if (e != hipSuccess) return (int)e;
    }
    format_selection(buf, buf_len, pl.mode, rq.out_kind, pl.src_w, pl.src_h, pl.dst_w, pl.dst_h, info, d.n_frames, rq.two_pass ? pl.fourcc : 0);
    return TSVPP_OK;
}

int tsvpp_debug_last_launch(char *buf, size_t buf_len) {
    if (!buf || buf_len == 0) return TSVPP_ERROR;
    buf[0] = 0;
    const char *gate = std::getenv("TSVPP_DEBUG_KNOBS");
    if (!gate || std::atoi(gate) == 0) return TSVPP_UNSUPPORTED;
    const LaunchRecord *r = g_last_launch;
    if (!r) return TSVPP_ERROR;
    // the fields tsvpp_describe reports, read off the launch as it went out: the FINAL descriptor of the first launch; a second launch is the row tail
    const LaunchDesc &d = r->d;
    LaunchInfo info = {};
    info.kernel = r->name;
    info.tx = d.tx;
    info.ty = d.ty;
    info.rpt = d.rpt;
    info.dma = d.dma;
    info.staged = r->staged;
    info.lds_bytes = (int)r->lds; // (dynamic LDS only: tsvpp_describe adds the static exchange slabs of some kernels)
    info.grid = (int)r->grid.x;
    info.tiles_x = d.tiles_x;
    info.tiles_y = d.tiles_y;
    info.tail = d.last_col0 > 0 ? 2 : (r->count > 1 ? 1 : 0);
    info.geo = d.geo;
    info.nt = d.nt_stores;
    info.in4 = d.in_aligned4;
    format_selection(buf, buf_len, r->mode, r->out, d.src_w, d.src_h, d.dst_w, d.dst_h, info, d.n_frames, r->pass2);
    return TSVPP_OK;
}

const char *tsvpp_strerror(int status) {
    switch (status) {
    case TSVPP_OK: return "ok";
    case TSVPP_REPEAT: return "VREADER_REPEAT: repeat the request";
    case TSVPP_UNSUPPORTED: return "VREADER_UNSUPPORTED: unsupported parameters (odd size, unknown FourCC/resize type, mixed batch geometry)";
    case TSVPP_ERROR: return "VREADER_ERROR: invalid argument or consumer pool exhausted";
    default: break;
    }
    if (status > 0) return hipGetErrorString((hipError_t)status);
    return "unknown status";
}

const char *tsvpp_version(void) { return "tsvpp 0.3.0 gfx950"; }

} // extern "C"
