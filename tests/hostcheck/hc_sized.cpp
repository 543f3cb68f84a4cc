// hc_sized.cpp -- host check, single thread (AddressSanitizer + UndefinedBehaviorSanitizer): tsvpp_convert_rois_sized / tsvpp_describe_rois_sized, their tensor
// forms and tsvpp_rois_sized_tile on the stub runtime (stub_hip.cpp).  Launches are recorded and range-checked by the stub, never executed.
// usage: hc_sized <request file>   -- written by tests/test_hostcheck_sized_cpu.py from tests/rois_sized_util.py (the seeded requests of the CPU test), one per line:
//   sized resize_type fourcc planes normalization dtype mean*3 scale*3 n_frames {w h pitch} n {frame left top right bottom dst_w dst_h aligned}
// (dtype -1: the plain form; floats travel as the eight hex digits of their bits; `aligned`: where the box's output lies in the "mixed" placement)
// Every request goes through describe (outputs aligned / not) and convert with all outputs aligned, none, and mixed -- the two-class split --, then once on a
// capturing stream and once with the next allocation failing: the path allocates nothing, so both succeed.  The launches the stub saw are the described ones:
// their number, ceil(n_vec / 48) + ceil(n_el / 48), the first grid, the sum of all grids = the sum of the boxes' tile counts, 128 threads, always in order.
// Exit status 0 only without a failed assertion, a stub violation, or anything the stub still holds at the end.
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "hc_common.h"

namespace {

struct Tokens {
    std::vector<std::string> t;
    size_t at = 0;
    explicit Tokens(const std::string &l) {
        std::istringstream in(l);
        std::string w;
        while (in >> w) t.push_back(w);
    }
    const std::string &word() {
        if (at >= t.size()) {
            std::fprintf(stderr, "hc_sized: line too short\n");
            std::exit(3);
        }
        return t[at++];
    }
    int i() { return (int)std::strtol(word().c_str(), nullptr, 10); }
    float f() {
        const uint32_t bits = (uint32_t)std::strtoul(word().c_str(), nullptr, 16);
        float v;
        std::memcpy(&v, &bits, 4);
        return v;
    }
};

long tiles_of(const tsvpp_roi_sized &r) { return (long)((r.dst_width + 31) / 32) * ((r.dst_height + 31) / 32); }
bool narrow(const tsvpp_roi_sized &r) { return (r.dst_width & 3) != 0 && r.dst_width < 32; }

struct Request {
    tsvpp_params p = {};
    tsvpp_tensor_spec spec = {};
    bool tensor = false;
    std::vector<tsvpp_nv12> frames;
    std::vector<tsvpp_roi_sized> rois;
    std::vector<int> mixed; // per box: aligned in the mixed placement
    std::vector<uint8_t *> blocks;
    uint8_t *out = nullptr;
    std::vector<size_t> offs; // of every output in `out`, 256-byte aligned
    size_t esz = 1;

    int describe(int aligned, char *buf, size_t len) const {
        return tensor ? tsvpp_describe_rois_sized_tensor(&p, &spec, (int)frames.size(), frames.data(), (int)rois.size(), rois.data(), aligned, buf, len)
                      : tsvpp_describe_rois_sized(&p, (int)frames.size(), frames.data(), (int)rois.size(), rois.data(), aligned, buf, len);
    }
    int convert(tsvpp_ctx *ctx, void *const *outs, void *stream) const {
        return tensor ? tsvpp_convert_rois_sized_tensor(ctx, (int)frames.size(), frames.data(), (int)rois.size(), rois.data(), &p, &spec, outs, stream)
                      : tsvpp_convert_rois_sized(ctx, (int)frames.size(), frames.data(), (int)rois.size(), rois.data(), &p, outs, stream);
    }
    // placement 0: every output 16-byte aligned; 1: every output one element past a boundary; 2: as `mixed` says
    std::vector<void *> outs(int placement) const {
        std::vector<void *> o;
        for (size_t i = 0; i < rois.size(); i++) o.push_back(out + offs[i] + ((placement == 0 || (placement == 2 && mixed[i])) ? 0 : esz));
        return o;
    }
    ~Request() {
        for (uint8_t *b : blocks) (void)hipFree(b);
        if (out) (void)hipFree(out);
    }
};

// what the stub saw of one convert call against the split the header states
void check_launches(const Request &r, const std::vector<void *> &outs, const char *what, int captured) {
    long n_vec = 0, n_el = 0, all_tiles = 0, first = 0;
    for (size_t i = 0; i < r.rois.size(); i++) {
        const bool vec = ((uintptr_t)outs[i] & 15) == 0 && !narrow(r.rois[i]);
        (vec ? n_vec : n_el)++;
        all_tiles += tiles_of(r.rois[i]);
    }
    long taken = 0; // the first launch: the first 48 boxes of the vector class, or of the other if there is none
    for (size_t i = 0; i < r.rois.size() && taken < TSVPP_MAX_ROIS_SIZED; i++) {
        const bool vec = ((uintptr_t)outs[i] & 15) == 0 && !narrow(r.rois[i]);
        if (vec == (n_vec > 0)) first += tiles_of(r.rois[i]), taken++;
    }
    const long want = (n_vec + TSVPP_MAX_ROIS_SIZED - 1) / TSVPP_MAX_ROIS_SIZED + (n_el + TSVPP_MAX_ROIS_SIZED - 1) / TSVPP_MAX_ROIS_SIZED;
    HC_CHECK((long)hc_stub_launch_count() == want, "%s: %zu launches for %ld vector and %ld element-wise boxes, expected %ld", what, hc_stub_launch_count(), n_vec, n_el, want);
    long grids = 0;
    for (size_t l = 0; l < hc_stub_launch_count(); l++) {
        const HcLaunch &k = *hc_stub_launch(l);
        grids += k.grid[0];
        HC_CHECK(k.block[0] == 128 && k.block[1] == 1 && k.grid[1] == 1 && !k.any_order && !k.refused && k.captured == captured,
                 "%s: launch %zu: block %u x %u, grid y %u, any_order %d, refused %d, captured %d", what, l, k.block[0], k.block[1], k.grid[1], k.any_order, k.refused, k.captured);
        HC_CHECK(std::string(k.name).find("vpp_rois_sized_kernel") != std::string::npos, "%s: launch %zu is %s", what, l, k.name);
    }
    HC_CHECK(grids == all_tiles, "%s: the grids sum to %ld, the boxes' tiles to %ld", what, grids, all_tiles);
    if (hc_stub_launch_count()) HC_CHECK((long)hc_stub_launch(0)->grid[0] == first, "%s: the first grid is %u, expected %ld", what, hc_stub_launch(0)->grid[0], first);
}

void run(tsvpp_ctx *ctx, void *stream, Tokens &k, const char *text) {
    Request r;
    r.p.resize_type = k.i(), r.p.fourcc = k.i(), r.p.planes = k.i(), r.p.normalization = k.i();
    r.spec.dtype = k.i();
    for (float &m : r.spec.mean) m = k.f();
    for (float &s : r.spec.scale) s = k.f();
    r.tensor = r.spec.dtype >= 0;
    r.esz = r.tensor ? (r.spec.dtype == TSVPP_F32 ? 4 : 2) : (r.p.normalization ? 4 : 1);
    const int n_frames = k.i();
    for (int f = 0; f < n_frames; f++) {
        const int w = k.i(), h = k.i(), pitch = k.i();
        uint8_t *y = hc::dev_alloc((size_t)h * pitch), *uv = hc::dev_alloc((size_t)(h / 2) * pitch);
        r.blocks.push_back(y), r.blocks.push_back(uv);
        r.frames.push_back(tsvpp_nv12{ y, uv, pitch, pitch, w, h });
    }
    const int n = k.i();
    size_t total = 0;
    for (int i = 0; i < n; i++) {
        tsvpp_roi_sized b = {};
        b.frame = k.i(), b.left = k.i(), b.top = k.i(), b.right = k.i(), b.bottom = k.i(), b.dst_width = k.i(), b.dst_height = k.i();
        r.rois.push_back(b);
        r.mixed.push_back(k.i());
        const size_t bytes = tsvpp_rois_sized_bytes(&r.p, r.tensor ? &r.spec : nullptr, b.dst_width, b.dst_height);
        HC_CHECK(bytes > 0, "rois_sized_bytes of box %d: %s", i, text);
        r.offs.push_back(total);
        total += (bytes + 16 + 255) & ~(size_t)255;
    }
    r.out = hc::dev_alloc(total);

    char desc1[512] = "", desc0[512] = "";
    const int d1 = r.describe(1, desc1, sizeof(desc1)), d0 = r.describe(0, desc0, sizeof(desc0));
    HC_CHECK(d1 == TSVPP_OK && d0 == TSVPP_OK, "describe answers %d / %d: %.200s", d1, d0, text);
    if (d1 != TSVPP_OK || d0 != TSVPP_OK) return;
    HC_CHECK(hc::value_of(desc1, "dst") == "var" && hc::number_of(desc1, "rois") == n && hc::number_of(desc0, "vec") == 0 && hc::number_of(desc1, "limit") == TSVPP_MAX_ROIS_SIZED,
             "describe line: %s", desc1);
    const long held = hc_stub_live();
    for (int placement = 0; placement < 3; placement++) {
        const std::vector<void *> outs = r.outs(placement);
        hc_stub_clear_launches();
        const int cs = r.convert(ctx, outs.data(), stream);
        HC_CHECK(cs == TSVPP_OK, "convert, placement %d: %d (%s): %.200s", placement, cs, tsvpp_strerror(cs), text);
        if (cs != TSVPP_OK) continue;
        check_launches(r, outs, placement == 0 ? "aligned" : placement == 1 ? "unaligned" : "mixed", 0);
        if (placement < 2) { // the launches that went out are the described ones
            const char *d = placement == 0 ? desc1 : desc0;
            HC_CHECK((long)hc_stub_launch_count() == hc::number_of(d, "launches") && (long)hc_stub_launch(0)->grid[0] == hc::number_of(d, "grid"),
                     "launched %zu with a first grid of %u, described %s", hc_stub_launch_count(), hc_stub_launch(0)->grid[0], d);
            const long extra = hc::number_of(d, "lds") - (long)hc_stub_launch(0)->lds; // describe adds the static exchange slab of the kernel's store side
            HC_CHECK(extra == 0 || extra == 3072 || extra == 12288, "the first launch has %zu bytes of dynamic LDS, described %s", hc_stub_launch(0)->lds, d);
        }
        // the lookup on the request's first launch: every workgroup has a tile of a box of the request, one past the grid has none
        int32_t t5[5];
        const unsigned grid = hc_stub_launch(0)->grid[0];
        long sum = 0;
        for (unsigned wg = 0; wg < grid && placement < 2; wg++) {
            const int ts = tsvpp_rois_sized_tile(&r.p, n_frames, r.frames.data(), n, r.rois.data(), placement == 0, wg, t5);
            HC_CHECK(ts == TSVPP_OK && t5[0] >= 0 && t5[0] < n && t5[3] >= 0 && t5[3] < r.rois[(size_t)t5[0]].dst_width && t5[4] < r.rois[(size_t)t5[0]].dst_height,
                     "rois_sized_tile(%u): %d", wg, ts);
            sum += t5[0];
        }
        (void)sum;
        if (placement < 2) HC_CHECK(tsvpp_rois_sized_tile(&r.p, n_frames, r.frames.data(), n, r.rois.data(), placement == 0, grid, t5) == TSVPP_ERROR, "wg = grid");
    }
    // on a capturing stream: no allocation, no copy, no synchronisation -- the stub would answer each with the capture error
    const std::vector<void *> mixed = r.outs(2);
    hc_stub_set_capturing((hipStream_t)stream, 1);
    hc_stub_clear_launches();
    const int cap = r.convert(ctx, mixed.data(), stream);
    hc_stub_set_capturing((hipStream_t)stream, 0);
    HC_CHECK(cap == TSVPP_OK, "convert on a capturing stream: %d (%s)", cap, tsvpp_strerror(cap));
    if (cap == TSVPP_OK) check_launches(r, mixed, "capturing", 1);
    // with the next allocation failing: there is none to fail
    hc_stub_fail_alloc_after(1);
    hc_stub_clear_launches();
    const int oom = r.convert(ctx, mixed.data(), stream);
    hc_stub_fail_alloc_after(0);
    HC_CHECK(oom == TSVPP_OK, "convert with the next allocation failing: %d (%s): the path allocates", oom, tsvpp_strerror(oom));
    HC_CHECK(hc_stub_live() == held, "the conversions left %ld blocks, streams or events of the stub's behind", hc_stub_live() - held);
    HC_CHECK(hc::current_device() == 0, "the thread ends on device %d", hc::current_device());
    // refusals on the live context
    std::vector<void *> hole = mixed;
    hole[hole.size() / 2] = nullptr;
    HC_CHECK(r.convert(ctx, hole.data(), stream) == TSVPP_ERROR && r.convert(nullptr, mixed.data(), stream) == TSVPP_ERROR && r.convert(ctx, nullptr, stream) == TSVPP_ERROR,
             "a null output, a null context, null outs");
    r.p.dst_width = r.rois[0].dst_width, r.p.dst_height = r.rois[0].dst_height;
    hc_stub_clear_launches();
    HC_CHECK(r.convert(ctx, mixed.data(), stream) == TSVPP_ERROR && r.describe(1, desc1, sizeof(desc1)) == TSVPP_ERROR && hc_stub_launch_count() == 0, "non-zero p->dst_* is TSVPP_ERROR");
}

} // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: hc_sized <request file>\n");
        return 2;
    }
    std::ifstream file(argv[1]);
    if (!file) {
        std::fprintf(stderr, "hc_sized: cannot read %s\n", argv[1]);
        return 2;
    }
    tsvpp_ctx *ctx = nullptr;
    void *stream = nullptr;
    HC_CHECK(tsvpp_create(1, 1, &ctx) == TSVPP_OK && ctx, "tsvpp_create on the stub's second device");
    if (!ctx) return 3;
    HC_CHECK(tsvpp_consumer_stream(ctx, "sized", &stream) == TSVPP_OK && stream, "the consumer's stream");
    int count = 0, tensors = 0;
    std::string line;
    while (std::getline(file, line)) {
        if (line.empty() || line[0] == '#') continue;
        Tokens k(line);
        HC_CHECK(k.word() == "sized", "unknown request kind");
        run(ctx, stream, k, line.c_str());
        count++;
        tensors += line.find(" -1 ") == std::string::npos ? 1 : 0;
    }
    std::fprintf(stderr, "hc_sized: %d requests, %d of them tensor forms\n", count, tensors);
    HC_CHECK(count >= 20 && tensors >= 1, "the request file holds the seeded requests and a tensor form");
    tsvpp_destroy(ctx);
    return hc::verdict("hc_sized");
}
