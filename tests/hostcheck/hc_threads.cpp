// hc_threads.cpp -- host check under ThreadSanitizer (and once more under AddressSanitizer): eight threads do, for a fixed number of iterations, what
// include/tsvpp.h and cpp/VideoProcessor.h allow concurrently, on the stub runtime (stub_hip.cpp).
//   every thread   is a named consumer of ONE shared context (tsvpp_consumer_next_stream / tsvpp_consumer_synchronize) and converts a rotating set of twelve
//                  distinct requests -- more than the eight entries of a thread's replay cache, so it evicts;
//                  creates and destroys a context and a frame table of its own now and then;
//                  calls VideoProcessor::Convert / Release on one shared object ("Convert and Release may be called from several threads on one object").
//   threads 0, 1   tsvpp_table_set disjoint entry ranges of one shared table ("tsvpp_table_set calls are serialised against each other")
//   threads 2, 3   tsvpp_convert_table other ranges of it, set before the threads start (the same entries from two threads would be "the caller's race")
//   thread 7       instead of converting: tsvpp_set_option (inputs-ready 0 / 1 / 2, the green-term option), tsvpp_enable_markers and tsvpp_trim in a loop
//                  ("tsvpp_set_option ... may be called while other threads convert through the same context"; nothing ever runs on the stub, so every point is
//                  quiescent in tsvpp_trim's sense: no launch is in flight on a device)
//   before them    one thread holds more results of VideoProcessor::Convert than the processor used to remember, then releases every one
//   between joins  tsvpp_set_coeffs ("needs a QUIESCENT context"): only the main thread, only while no other thread exists.
// usage: hc_threads [iterations per thread, default 300].  Exit status 0 only without a failed assertion and without a stub violation; a sanitizer report ends
// the process with the sanitizer's own status.
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "VideoProcessor.h"
#include "hc_common.h"

namespace {

constexpr int kThreads = 8;

struct Request {
    int w, h, pitch, dw, dh, rt, fcc, planes, norm;
};
// twelve: dyadic BILINEAR on uint8 (geometry tables), BICUBIC (column tables), AREA with integer and float weights (weight and divisor tables), the streaming
// ratios, UYVY behind a resize (two passes, the per-stream scratch slot), no resize at all
const Request kRequests[12] = {
    { 640, 360, 640, 512, 288, TSVPP_BILINEAR, TSVPP_RGB24, TSVPP_PLANAR, 0 }, { 640, 360, 640, 512, 288, TSVPP_BILINEAR, TSVPP_BGR24, TSVPP_MERGED, 1 },
    { 640, 360, 656, 300, 300, TSVPP_BICUBIC, TSVPP_RGB24, TSVPP_PLANAR, 1 },  { 640, 360, 640, 426, 240, TSVPP_BICUBIC, TSVPP_RGB24, TSVPP_MERGED, 0 },
    { 640, 360, 640, 256, 144, TSVPP_AREA, TSVPP_RGB24, TSVPP_PLANAR, 1 },     { 640, 360, 640, 160, 90, TSVPP_AREA, TSVPP_BGR24, TSVPP_MERGED, 0 },
    { 640, 360, 640, 320, 180, TSVPP_BILINEAR, TSVPP_RGB24, TSVPP_PLANAR, 1 }, { 640, 360, 704, 480, 270, TSVPP_BILINEAR, TSVPP_UYVY, TSVPP_PLANAR, 0 },
    { 640, 360, 640, 0, 0, TSVPP_NEAREST, TSVPP_RGB24, TSVPP_MERGED, 0 },      { 640, 360, 640, 1280, 720, TSVPP_BILINEAR, TSVPP_Y800, TSVPP_PLANAR, 1 },
    { 320, 240, 320, 224, 224, TSVPP_NEAREST, TSVPP_RGB24, TSVPP_PLANAR, 1 },  { 640, 360, 640, 854, 480, TSVPP_AREA, TSVPP_YUV444, TSVPP_PLANAR, 0 },
};

tsvpp_params params_of(const Request &r) {
    tsvpp_params p = {};
    p.dst_width = r.dw;
    p.dst_height = r.dh;
    p.resize_type = r.rt;
    p.fourcc = r.fcc;
    p.planes = r.planes;
    p.normalization = r.norm;
    return p;
}

struct Shared {
    tsvpp_ctx *ctx = nullptr;
    tsvpp_table *table = nullptr; // 64 entries of 640 x 360
    VideoProcessor *vpp = nullptr;
    uint8_t *y = nullptr, *uv = nullptr, *out = nullptr; // planes and an output every call shares: nothing is ever executed
    int iterations = 300;
};

void worker(const Shared &sh, int id) {
    const std::string name = "consumer" + std::to_string(id);
    tsvpp_nv12 frames[16];
    void *outs[16];
    for (int i = 0; i < 16; i++) {
        frames[i] = tsvpp_nv12{ sh.y, sh.uv, 640, 640, 640, 360 };
        outs[i] = sh.out;
    }
    const tsvpp_params table_p = params_of(kRequests[0]);
    for (int it = 0; it < sh.iterations; it++) {
        hc_stub_clear_launches();
        void *stream = nullptr;
        HC_CHECK(tsvpp_consumer_next_stream(sh.ctx, name.c_str(), 0, &stream) == TSVPP_OK && stream, "consumer_next_stream of %s", name.c_str());
        if (id == 7) { // the one thread that changes the context under the others
            HC_CHECK(tsvpp_set_option(sh.ctx, TSVPP_OPT_INPUTS_READY, it % 3) == TSVPP_OK, "set_option inputs-ready");
            HC_CHECK(tsvpp_set_option(sh.ctx, TSVPP_OPT_COLOR_G_TERM, (it / 3) % 3) == TSVPP_OK, "set_option green term");
            const int m = tsvpp_enable_markers(sh.ctx, it & 1);
            HC_CHECK(m == TSVPP_OK || m == TSVPP_UNSUPPORTED, "enable_markers: %d", m);
            int v = -1;
            HC_CHECK(tsvpp_get_option(sh.ctx, TSVPP_OPT_COLOR_G_TERM, &v) == TSVPP_OK && v == (it / 3) % 3, "get_option reads back what this thread set");
            if (it % 8 == 0) HC_CHECK(tsvpp_trim(sh.ctx, nullptr) == TSVPP_OK, "trim");
        } else {
            for (int k = 0; k < 3; k++) { // three of the twelve per iteration: every request comes round again after four
                const Request &r = kRequests[(3 * it + k + id) % 12];
                const tsvpp_nv12 in = { sh.y, sh.uv, r.pitch, r.pitch, r.w, r.h };
                const tsvpp_params p = params_of(r);
                HC_CHECK(tsvpp_convert(sh.ctx, &in, &p, sh.out, stream) == TSVPP_OK, "thread %d converts request %d", id, (3 * it + k + id) % 12);
            }
            HC_CHECK(hc_stub_launch_count() >= 3, "three conversions launched %zu kernels", hc_stub_launch_count());
        }
        if (id < 2) HC_CHECK(tsvpp_table_set(sh.table, 16 * id + it % 8, 8, frames, outs, stream) == TSVPP_OK, "table_set of thread %d", id);
        if (id == 2 || id == 3) HC_CHECK(tsvpp_convert_table(sh.ctx, sh.table, 16 * id, 16, &table_p, stream) == TSVPP_OK, "convert_table of thread %d", id);
        if (it % 16 == 15) HC_CHECK(tsvpp_consumer_synchronize(sh.ctx, name.c_str()) == TSVPP_OK, "consumer_synchronize of %s", name.c_str());
        if (it % 32 == id) { // a context and a table of this thread's own, meanwhile (on the stub's second device: the device guard switches and restores)
            tsvpp_ctx *own = nullptr;
            tsvpp_table *tab = nullptr;
            HC_CHECK(tsvpp_create(1, 2, &own) == TSVPP_OK && own, "a context of thread %d's own", id);
            HC_CHECK(tsvpp_table_create(own, 16, &tab) == TSVPP_OK && tab, "a table of thread %d's own", id);
            void *s = nullptr;
            HC_CHECK(tsvpp_consumer_stream(own, "own", &s) == TSVPP_OK, "its stream");
            HC_CHECK(tsvpp_table_set(tab, 0, 16, frames, outs, s) == TSVPP_OK, "its table_set");
            HC_CHECK(tsvpp_convert_table(own, tab, 3, 9, &table_p, s) == TSVPP_OK, "its convert_table");
            const Request &r = kRequests[it % 12];
            const tsvpp_nv12 in = { sh.y, sh.uv, r.pitch, r.pitch, r.w, r.h };
            const tsvpp_params p = params_of(r);
            HC_CHECK(tsvpp_convert(own, &in, &p, sh.out, s) == TSVPP_OK, "its convert");
            HC_CHECK(hc::current_device() == 0, "the calling thread's device is left as it was");
            if (it & 32) { // either order of destruction is legal
                tsvpp_table_destroy(tab);
                tsvpp_destroy(own);
            } else {
                tsvpp_destroy(own);
                tsvpp_table_destroy(tab);
            }
        }
        { // the adapter: one object, every thread its own consumer
            AVFrame in, out;
            in.data[0] = sh.y;
            in.data[1] = sh.uv;
            in.linesize[0] = in.linesize[1] = 640;
            in.width = 640;
            in.height = 360;
            FrameParameters fp(ResizeOptions(320 + 32 * (it % 3), 180), ColorOptions(it & 1 ? FourCC::BGR24 : FourCC::RGB24));
            fp.resize.type = ResizeType::BILINEAR;
            HC_CHECK(sh.vpp->Convert(&in, &out, fp, name) == VREADER_OK && out.opaque, "VideoProcessor::Convert on thread %d", id);
            if (out.opaque) HC_CHECK(sh.vpp->Release(out.opaque, (hipStream_t)stream) == VREADER_OK, "VideoProcessor::Release on thread %d", id);
        }
    }
    hc_stub_clear_launches();
}

// cpp/VideoProcessor.h: "a result is never forgotten while its caller may still Release() it, however many Converts lie in between" -- more results than the 65536
// entries at which the processor used to forget all of them are held at once, then every one is released
void results_are_never_forgotten(const Shared &sh) {
    constexpr int kHeld = 65536 + 64;
    std::vector<void *> held;
    held.reserve(kHeld);
    FrameParameters fp(ResizeOptions(2, 2), ColorOptions(FourCC::RGB24)); // 12 bytes a result
    int converted = 0, released = 0;
    for (int i = 0; i < kHeld; i++) {
        AVFrame in, out;
        in.data[0] = sh.y;
        in.data[1] = sh.uv;
        in.linesize[0] = in.linesize[1] = 64;
        in.width = 64;
        in.height = 36;
        if (sh.vpp->Convert(&in, &out, fp, "holder") == VREADER_OK && out.opaque) converted++, held.push_back(out.opaque);
    }
    HC_CHECK(converted == kHeld, "%d of %d conversions", converted, kHeld);
    for (void *p : held) released += sh.vpp->Release(p, nullptr) == VREADER_OK;
    HC_CHECK(released == converted, "Release took back %d of the %d results that were held at once: the others had been forgotten", released, converted);
    int foreign = 0;
    HC_CHECK(sh.vpp->Release(&foreign, nullptr) == VREADER_ERROR && sh.vpp->Release(held[0], nullptr) == VREADER_ERROR,
             "a pointer Convert did not hand out, and one released twice, are still VREADER_ERROR");
}

void run_threads(const Shared &sh) {
    std::vector<std::thread> threads;
    for (int id = 0; id < kThreads; id++) threads.emplace_back(worker, std::cref(sh), id);
    for (std::thread &t : threads) t.join();
}

} // namespace

int main(int argc, char **argv) {
    Shared sh;
    if (argc > 1) sh.iterations = std::atoi(argv[1]);
    const auto t0 = std::chrono::steady_clock::now();
    sh.y = hc::dev_alloc(4096);
    sh.uv = hc::dev_alloc(4096);
    sh.out = hc::dev_alloc(4096);
    HC_CHECK(tsvpp_create(0, kThreads, &sh.ctx) == TSVPP_OK && sh.ctx, "the shared context");
    HC_CHECK(tsvpp_table_create(sh.ctx, 64, &sh.table) == TSVPP_OK && sh.table, "the shared table");
    if (!sh.ctx || !sh.table) return 3;
    {
        tsvpp_nv12 frames[64];
        void *outs[64];
        for (int i = 0; i < 64; i++) {
            frames[i] = tsvpp_nv12{ sh.y, sh.uv, 640, 640, 640, 360 };
            outs[i] = sh.out;
        }
        HC_CHECK(tsvpp_table_set(sh.table, 0, 64, frames, outs, nullptr) == TSVPP_OK, "every entry of the shared table, before the threads start");
    }
    VideoProcessor vpp;
    HC_CHECK(vpp.Init(nullptr, kThreads + 1, false, 0) == VREADER_OK, "VideoProcessor::Init");
    sh.vpp = &vpp;
    results_are_never_forgotten(sh);

    tsvpp_coeffs k;
    tsvpp_default_coeffs(&k);
    for (int phase = 0; phase < 2; phase++) {
        HC_CHECK(tsvpp_set_coeffs(sh.ctx, &k) == TSVPP_OK, "set_coeffs between joins (phase %d)", phase); // the context is quiescent: no other thread exists
        run_threads(sh);
    }
    HC_CHECK(hc_stub_total_launches() >= (long)2 * (kThreads - 1) * sh.iterations * 3, "%ld launches in all", hc_stub_total_launches());

    vpp.Close();
    tsvpp_table_destroy(sh.table);
    tsvpp_destroy(sh.ctx);
    (void)hipFree(sh.y);
    (void)hipFree(sh.uv);
    (void)hipFree(sh.out);
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::fprintf(stderr, "hc_threads: %d threads x 2 phases x %d iterations in %.2f s\n", kThreads, sh.iterations, secs);
    return hc::verdict("hc_threads");
}
