// vpp_letterbox -- letterboxes a few NV12 frames into canvases of one size through the C++ class (VideoProcessor::ConvertLetterbox) and prints a CRC-32 per canvas
// (the zlib / IEEE 802.3 one: reflected 0xEDB88320, as Python's zlib.crc32); tests/test_cpp_letterbox_gpu.py compares each with the CRC of the expected canvas.
//   vpp_letterbox [--dtype f16|bf16|f32] [--mean a,b,c] [--scale a,b,c] DW DH TYPE FOURCC PLANES NORM PADY PADU PADV  frame.nv12 W H PITCH [frame.nv12 W H PITCH ...]
// --dtype / --mean / --scale: through the ConvertLetterbox overload that takes a tsvpp_tensor_spec (tests/test_cpp_tensor_gpu.py); without them the output is byte
// for byte what it was.
// A file holds H rows of PITCH bytes of luma, then H / 2 rows of PITCH bytes of chroma.  Every frame gets the default rectangle (tsvpp_letterbox_rect).  Prints
// "<index> <crc> <bytes> <left> <top> <width> <height>" per canvas; exit code 0 = converted.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "VideoProcessor.h"
#include "tensor_flags.h"

static uint32_t crc32_zlib(const uint8_t *buf, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) {
        c ^= buf[i];
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : (c >> 1);
    }
    return c ^ 0xFFFFFFFFu;
}

int main(int argc, char **argv) {
    tsvpp_tensor_spec spec;
    const bool tensor = tensor_flags(argc, argv, spec);
    if (argc < 14 || (argc - 10) % 4 != 0) {
        fprintf(stderr, "usage: vpp_letterbox " TENSOR_FLAGS_USAGE " DW DH TYPE FOURCC PLANES NORM PADY PADU PADV frame.nv12 W H PITCH [frame.nv12 W H PITCH ...]\n");
        return 200;
    }
    const int DW = atoi(argv[1]), DH = atoi(argv[2]), type = atoi(argv[3]);
    const int fcc = atoi(argv[4]), planes = atoi(argv[5]), norm = atoi(argv[6]);
    const int padY = atoi(argv[7]), padU = atoi(argv[8]), padV = atoi(argv[9]);
    const int n = (argc - 10) / 4;
    std::vector<AVFrame *> inputs;
    std::vector<uint8_t *> planesDev;
    for (int k = 0; k < n; k++) {
        const char *path = argv[10 + 4 * k];
        const int W = atoi(argv[11 + 4 * k]), H = atoi(argv[12 + 4 * k]), P = atoi(argv[13 + 4 * k]);
        std::vector<uint8_t> host((size_t)P * H * 3 / 2);
        FILE *f = fopen(path, "rb");
        if (!f || fread(host.data(), 1, host.size(), f) != host.size()) { fprintf(stderr, "cannot read %s\n", path); return 201; }
        fclose(f);
        uint8_t *dY = nullptr, *dUV = nullptr;
        if (hipMalloc(&dY, (size_t)P * H) != hipSuccess || hipMalloc(&dUV, (size_t)P * H / 2) != hipSuccess) return 202;
        (void)hipMemcpy(dY, host.data(), (size_t)P * H, hipMemcpyHostToDevice);
        (void)hipMemcpy(dUV, host.data() + (size_t)P * H, (size_t)P * H / 2, hipMemcpyHostToDevice);
        AVFrame *input = av_frame_alloc();
        input->data[0] = dY;
        input->data[1] = dUV;
        input->linesize[0] = input->linesize[1] = P;
        input->width = W;
        input->height = H;
        inputs.push_back(input);
        planesDev.push_back(dY);
        planesDev.push_back(dUV);
    }

    VideoProcessor vpp;
    if (vpp.Init(std::make_shared<Logger>()) != 0) return 203;
    ColorOptions color((FourCC)fcc);
    color.planesPos = (Planes)planes;
    color.normalization = norm != 0;
    ResizeOptions resize(DW, DH);
    resize.type = (ResizeType)type;
    FrameParameters options(resize, color);
    size_t bytes = (size_t)(channelsByFourCC((FourCC)fcc) * (float)DW) * (size_t)DH * (norm ? sizeof(float) : 1);
    if (tensor) {
        const tsvpp_params flat{ 0, 0, 0, 0, DW, DH, type, fcc, planes, norm };
        bytes = tsvpp_tensor_bytes(&flat, &spec);
        if (bytes == 0) return 205; // a (parameters, spec) pair the tensor entry points refuse
    }
    const size_t stride = (bytes + 255) & ~(size_t)255;
    uint8_t *dOut = nullptr;
    if (hipMalloc(&dOut, stride * (size_t)n) != hipSuccess) return 204;
    std::vector<void *> outs((size_t)n);
    for (int k = 0; k < n; k++) outs[(size_t)k] = dOut + (size_t)k * stride;
    const int sts = tensor ? vpp.ConvertLetterbox(inputs.data(), n, nullptr, padY, padU, padV, outs.data(), options, &spec, "letterbox")
                           : vpp.ConvertLetterbox(inputs.data(), n, nullptr, padY, padU, padV, outs.data(), options, "letterbox");
    if (sts != 0) return 210;
    if (tsvpp_consumer_synchronize(vpp.context(), "letterbox") != 0) return 211; // the conversion is asynchronous, on the consumer's stream
    std::vector<uint8_t> result(bytes);
    for (int k = 0; k < n; k++) {
        if (hipMemcpy(result.data(), outs[(size_t)k], bytes, hipMemcpyDeviceToHost) != hipSuccess) return 212;
        tsvpp_rect r = {};
        if (tsvpp_letterbox_rect(inputs[(size_t)k]->width, inputs[(size_t)k]->height, DW, DH, &r) != 0) return 213;
        printf("%d %u %zu %d %d %d %d\n", k, crc32_zlib(result.data(), bytes), bytes, r.left, r.top, r.width, r.height);
    }
    // a rectangle outside the canvas is refused with the reference's status convention, and nothing is launched
    const tsvpp_rect bad{ 0, 0, DW + 2, 2 };
    const int refused = tensor ? vpp.ConvertLetterbox(inputs.data(), 1, &bad, padY, padU, padV, outs.data(), options, &spec, "letterbox")
                               : vpp.ConvertLetterbox(inputs.data(), 1, &bad, padY, padU, padV, outs.data(), options, "letterbox");
    if (refused != VREADER_ERROR) return 214;
    for (AVFrame *f : inputs) av_frame_free(&f);
    vpp.Close();
    (void)hipFree(dOut);
    for (uint8_t *p : planesDev) (void)hipFree(p);
    return 0;
}
