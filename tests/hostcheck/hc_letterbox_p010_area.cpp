// hc_letterbox_p010_area.cpp -- host check, single thread (AddressSanitizer + UndefinedBehaviorSanitizer): tsvpp_convert_letterbox_p010_area and
// VideoProcessor::ConvertLetterboxP010Area on the stub runtime (stub_hip.cpp), which records launches and never executes them.  Only what needs a live context:
// 33 frames of mixed ratios as two launches, eager and on a capturing stream, with the grid and the dynamic LDS the describe call names; a plane address that
// holds no 16-bit words; the adapter's two methods and its refusal; and tsvpp_box_p010_plane on a heap buffer that is exactly as long as its sizes say.
#include "VideoProcessor.h"
#include "hc_common.h"

// 33 frames at a pitch of 1040 bytes: 512 x 64 (ratios 16 and 2), 192 x 192 (6) and 34 x 34 in turn, into rectangles of 32 x 32 in canvases of 66 x 34
static void run(tsvpp_ctx *ctx, void *stream, int planes, bool tensor, const char *what) {
    const int n = TSVPP_MAX_LETTERBOX_P010 + 1, pitch = 1040, W[3] = { 512, 192, 34 }, H[3] = { 64, 192, 34 };
    tsvpp_params p = { 0, 0, 0, 0, 66, 34, TSVPP_AREA, TSVPP_RGB24, planes, tensor };
    tsvpp_tensor_spec spec = { TSVPP_F16, { 0.485f, 0.456f, 0.406f }, { 4.0f, 4.5f, 5.0f } };
    const tsvpp_tensor_spec *sp = tensor ? &spec : nullptr;
    const size_t stride = ((size_t)3 * 66 * 34 * (tensor ? 2 : 1) + 255) & ~(size_t)255, frame_bytes = (size_t)(192 + 96) * pitch;
    uint8_t *const src = hc::dev_alloc(frame_bytes * n), *const dst = hc::dev_alloc(stride * n);
    std::vector<tsvpp_p010> frames;
    std::vector<AVFrame> av(n);
    std::vector<AVFrame *> in;
    std::vector<tsvpp_rect> rects;
    std::vector<void *> outs;
    for (int k = 0; k < n; k++) {
        frames.push_back(tsvpp_p010{ (const uint16_t *)(src + k * frame_bytes), (const uint16_t *)(src + k * frame_bytes + 192 * pitch), pitch, pitch, W[k % 3], H[k % 3] });
        av[k].data[0] = (uint8_t *)frames[k].y, av[k].data[1] = (uint8_t *)frames[k].uv, av[k].linesize[0] = av[k].linesize[1] = pitch, av[k].width = W[k % 3], av[k].height = H[k % 3];
        in.push_back(&av[k]);
        rects.push_back(tsvpp_rect{ 2 * (k % 16), 2, 32, 32 });
        outs.push_back(dst + k * stride);
    }
    char line[512];
    int grid = 0, lds = 0;
    HC_CHECK(tsvpp_describe_letterbox_p010_area(&p, sp, n, frames.data(), rects.data(), 1, line, sizeof(line)) == TSVPP_OK, "%s: describe", what);
    const char *g = strstr(line, " grid="), *l = strstr(line, " lds=");
    HC_CHECK(g && l && strstr(line, " launches=2 ") && strstr(line, " taps=16x6 "), "%s: %s", what, line);
    if (g && l) grid = atoi(g + 6), lds = atoi(l + 5);
    const auto convert = [&] { return tsvpp_convert_letterbox_p010_area(ctx, n, frames.data(), &p, sp, rects.data(), 64, 512, 512, outs.data(), stream); };
    for (int leg = 0; leg < 2; leg++) { // eager, then capturing: an allocation, a copy or a synchronisation would fail the capture
        hc_stub_set_capturing((hipStream_t)stream, leg);
        hc_stub_clear_launches();
        const int cs = convert();
        hc_stub_set_capturing((hipStream_t)stream, 0);
        HC_CHECK(cs == TSVPP_OK && hc_stub_launch_count() == 2 && hc_stub_launch(0)->captured == leg && hc_stub_launch(1)->captured == leg && !hc_stub_launch(1)->refused,
                 "%s, leg %d: status %d, %zu launches", what, leg, cs, hc_stub_launch_count());
        if (hc_stub_launch_count() == 2)
            HC_CHECK((int)hc_stub_launch(0)->grid[0] == grid && hc_stub_launch(1)->grid[0] == 3 * 2 && hc_stub_launch(0)->lds + (planes == TSVPP_MERGED ? 256 * 12 : 0) == (size_t)lds,
                     "%s, leg %d: grid %u, lds %zu against %s", what, leg, hc_stub_launch(0)->grid[0], hc_stub_launch(0)->lds, line);
    }
    hc_stub_clear_launches();
    frames[0].y = (const uint16_t *)((const uint8_t *)frames[0].y + 1);
    HC_CHECK(convert() == TSVPP_ERROR && hc_stub_launch_count() == 0, "%s: a plane pointer that is not 2-byte aligned", what);
    // the adapter launches as often as the entry point, and answers a refusal in the reference's convention
    VideoProcessor vpp;
    HC_CHECK(vpp.Init(nullptr, 2, false, 0) == VREADER_OK, "VideoProcessor::Init");
    FrameParameters fp(ResizeOptions(66, 34), ColorOptions((FourCC)TSVPP_RGB24));
    fp.resize.type = ResizeType::AREA, fp.color.planesPos = (Planes)planes, fp.color.normalization = tensor;
    const auto adapter = [&] {
        hc_stub_clear_launches();
        return tensor ? vpp.ConvertLetterboxP010Area(in.data(), n, rects.data(), 64, 512, 512, outs.data(), fp, sp, "hc") : vpp.ConvertLetterboxP010Area(in.data(), n, rects.data(), 64, 512, 512, outs.data(), fp, "hc");
    };
    HC_CHECK(adapter() == VREADER_OK && hc_stub_launch_count() == 2, "%s: ConvertLetterboxP010Area, %zu launches", what, hc_stub_launch_count());
    fp.resize.type = ResizeType::BILINEAR;
    HC_CHECK(adapter() == VREADER_UNSUPPORTED && hc_stub_launch_count() == 0, "%s: the adapter refuses BILINEAR", what);
    vpp.Close();
    (void)hipFree(src), (void)hipFree(dst);
}

int main() {
    tsvpp_ctx *ctx = nullptr;
    void *stream = nullptr;
    HC_CHECK(tsvpp_create(1, 1, &ctx) == TSVPP_OK && ctx, "tsvpp_create on the stub's second device");
    if (!ctx) return 3;
    HC_CHECK(tsvpp_consumer_stream(ctx, "letterbox_p010_area", &stream) == TSVPP_OK && stream, "the consumer's stream");
    run(ctx, stream, TSVPP_MERGED, false, "33 frames, uint8 merged");
    run(ctx, stream, TSVPP_PLANAR, true, "33 frames, fp16 tensor");
    tsvpp_destroy(ctx);
    // the host form of the contract reads and writes exactly src_w x src_h and dst_w x dst_h samples; a flat plane comes back flat
    std::vector<uint16_t> s((size_t)50 * 38, 1023), d((size_t)32 * 30, 0);
    HC_CHECK(tsvpp_box_p010_plane(s.data(), 50, 38, d.data(), 32, 30) == TSVPP_OK && d.front() == 1023 && d.back() == 1023, "tsvpp_box_p010_plane 50 x 38 -> 32 x 30");
    HC_CHECK(tsvpp_box_p010_plane(s.data(), 16386, 2, d.data(), 32, 2) == TSVPP_UNSUPPORTED && tsvpp_box_p010_plane(nullptr, 2, 2, d.data(), 2, 2) == TSVPP_ERROR, "tsvpp_box_p010_plane refusals");
    return hc::verdict("hc_letterbox_p010_area");
}
