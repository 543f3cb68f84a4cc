// hc_rois_p010.cpp -- host check, single thread (AddressSanitizer + UndefinedBehaviorSanitizer): tsvpp_convert_rois_p010 and VideoProcessor::ConvertRoisP010 on the
// stub runtime (stub_hip.cpp), which records launches and never executes them.  Only what needs a live context: 65 boxes and 65 frames as two launches, eager and
// on a capturing stream; the host array of 65 frames refused (this file's operator new); a plane address that holds no 16-bit words; the adapter's two methods.
#include <new>
#include "VideoProcessor.h"
#include "hc_common.h"

static size_t g_refuse_new = 0; // armed: operator new refuses a request of exactly this size
void *operator new(size_t n) {
    if (n == g_refuse_new) throw std::bad_alloc();
    if (void *p = std::malloc(n ? n : 1)) return p;
    throw std::bad_alloc();
}
void operator delete(void *p) noexcept { std::free(p); }
void operator delete(void *p, size_t) noexcept { std::free(p); }

// 65 boxes spread over `n_frames` frames of 64 x 32 at a pitch of 144 bytes
static void run(tsvpp_ctx *ctx, void *stream, int n_frames, int dst_w, int dst_h, int type, int planes, bool tensor, const char *what) {
    const int n = TSVPP_MAX_ROIS_P010 + 1;
    tsvpp_params p = { 0, 0, 0, 0, dst_w, dst_h, type, TSVPP_RGB24, planes, tensor };
    tsvpp_tensor_spec spec = { TSVPP_F16, { 0.485f, 0.456f, 0.406f }, { 4.0f, 4.5f, 5.0f } };
    const tsvpp_tensor_spec *sp = tensor ? &spec : nullptr;
    const size_t stride = ((size_t)3 * dst_w * dst_h * (tensor ? 2 : 1) + 255) & ~(size_t)255;
    uint8_t *const src = hc::dev_alloc((size_t)n_frames * 48 * 144), *const dst = hc::dev_alloc(stride * n);
    std::vector<tsvpp_p010> frames;
    std::vector<AVFrame> av(n_frames);
    std::vector<AVFrame *> in;
    std::vector<tsvpp_roi> rois;
    std::vector<void *> outs;
    for (int k = 0; k < n_frames; k++) {
        frames.push_back(tsvpp_p010{ (const uint16_t *)(src + k * 48 * 144), (const uint16_t *)(src + (k * 48 + 32) * 144), 144, 144, 64, 32 });
        av[k].data[0] = (uint8_t *)frames[k].y, av[k].data[1] = (uint8_t *)frames[k].uv, av[k].linesize[0] = av[k].linesize[1] = 144, av[k].width = 64, av[k].height = 32;
        in.push_back(&av[k]);
    }
    for (int k = 0; k < n; k++) rois.push_back(tsvpp_roi{ k % n_frames, 2 * (k % 8), 2 * (k % 4), 32 + 2 * (k % 8), 24 }), outs.push_back(dst + k * stride);
    const auto convert = [&](void *const *o) { return tsvpp_convert_rois_p010(ctx, n_frames, frames.data(), n, rois.data(), &p, sp, o, stream); };
    for (int leg = 0; leg < 2; leg++) { // eager, then capturing: an allocation, a copy or a synchronisation would fail the capture
        hc_stub_set_capturing((hipStream_t)stream, leg);
        hc_stub_clear_launches();
        const int cs = convert(outs.data());
        hc_stub_set_capturing((hipStream_t)stream, 0);
        HC_CHECK(cs == TSVPP_OK && hc_stub_launch_count() == 2 && hc_stub_launch(0)->captured == leg && hc_stub_launch(1)->captured == leg && !hc_stub_launch(1)->refused,
                 "%s, leg %d: status %d, %zu launches", what, leg, cs, hc_stub_launch_count());
    }
    hc_stub_clear_launches();
    if (n_frames > TSVPP_MAX_ROIS_P010) { // the host array of the frames' byte-plane view cannot be had
        char buf[512];
        g_refuse_new = n_frames * sizeof(tsvpp_nv12);
        const int c = convert(outs.data()), d = tsvpp_describe_rois_p010(&p, sp, n_frames, frames.data(), n, rois.data(), 1, buf, sizeof(buf));
        g_refuse_new = 0;
        HC_CHECK(c == TSVPP_ERROR && d == TSVPP_ERROR, "%s: the host array refused: convert %d, describe %d", what, c, d);
    }
    frames[0].uv = (const uint16_t *)((const uint8_t *)frames[0].uv + 1);
    HC_CHECK(convert(outs.data()) == TSVPP_ERROR && hc_stub_launch_count() == 0, "%s: a plane pointer that is not 2-byte aligned", what);
    // the adapter launches as often as the entry point, and answers a refusal in the reference's convention
    VideoProcessor vpp;
    HC_CHECK(vpp.Init(nullptr, 2, false, 0) == VREADER_OK, "VideoProcessor::Init");
    FrameParameters fp(ResizeOptions(dst_w, dst_h), ColorOptions((FourCC)TSVPP_RGB24));
    fp.resize.type = (ResizeType)type, fp.color.planesPos = (Planes)planes, fp.color.normalization = tensor;
    const auto adapter = [&] {
        hc_stub_clear_launches();
        return tensor ? vpp.ConvertRoisP010(in.data(), n_frames, rois.data(), n, outs.data(), fp, sp, "hc") : vpp.ConvertRoisP010(in.data(), n_frames, rois.data(), n, outs.data(), fp, "hc");
    };
    HC_CHECK(adapter() == VREADER_OK && hc_stub_launch_count() == 2, "%s: ConvertRoisP010, %zu launches", what, hc_stub_launch_count());
    fp.resize.type = ResizeType::BICUBIC;
    HC_CHECK(adapter() == VREADER_UNSUPPORTED && hc_stub_launch_count() == 0, "%s: the adapter refuses BICUBIC", what);
    vpp.Close();
    (void)hipFree(src), (void)hipFree(dst);
}

int main() {
    tsvpp_ctx *ctx = nullptr;
    void *stream = nullptr;
    HC_CHECK(tsvpp_create(1, 1, &ctx) == TSVPP_OK && ctx, "tsvpp_create on the stub's second device");
    if (!ctx) return 3;
    HC_CHECK(tsvpp_consumer_stream(ctx, "rois_p010", &stream) == TSVPP_OK && stream, "the consumer's stream");
    run(ctx, stream, 2, 66, 34, TSVPP_BILINEAR, TSVPP_MERGED, false, "65 boxes of two frames, uint8 merged");
    run(ctx, stream, TSVPP_MAX_ROIS_P010 + 1, 32, 32, TSVPP_NEAREST, TSVPP_PLANAR, true, "65 frames, fp16 tensor");
    tsvpp_destroy(ctx);
    return hc::verdict("hc_rois_p010");
}
