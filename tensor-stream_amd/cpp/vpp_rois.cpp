// vpp_rois -- converts a handful of boxes of one NV12 frame through the C++ class (VideoProcessor::ConvertRois) and prints a CRC-32 per box
// (libavutil's AV_CRC_32_IEEE, as vpp_goldens computes it); tests/test_cpp_rois_gpu.py compares each with the oracle's.
//   vpp_rois [--area] [--dtype f16|bf16|f32] [--mean a,b,c] [--scale a,b,c] frame.nv12 W H PITCH  DW DH TYPE  FOURCC PLANES NORM  L T R B [L T R B ...]
// --area: through VideoProcessor::ConvertRoisArea (TYPE must then be 3, AREA; tests/test_cpp_rois_area_gpu.py).
// --dtype / --mean / --scale: through the ConvertRois overload that takes a tsvpp_tensor_spec (any TYPE; tests/test_cpp_tensor_gpu.py); without them the
// output is byte for byte what it was.
// The file holds H rows of PITCH bytes of luma, then H / 2 rows of PITCH bytes of chroma.  Prints "<index> <crc> <bytes>" per box; exit code 0 = converted.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "VideoProcessor.h"
#include "tensor_flags.h"

static uint32_t crc32_av(const uint8_t *buf, size_t n) {
    uint32_t c = __builtin_bswap32(0xFFFFFFFFu);
    for (size_t i = 0; i < n; i++) {
        c ^= (uint32_t)buf[i] << 24;
        for (int k = 0; k < 8; k++) c = (c & 0x80000000u) ? (c << 1) ^ 0x04C11DB7u : (c << 1);
    }
    return __builtin_bswap32(c);
}

int main(int argc, char **argv) {
    const bool area = argc > 1 && strcmp(argv[1], "--area") == 0;
    if (area) {
        argv++;
        argc--;
    }
    tsvpp_tensor_spec spec;
    const bool tensor = tensor_flags(argc, argv, spec);
    if (argc < 15 || (argc - 11) % 4 != 0) { fprintf(stderr, "usage: vpp_rois [--area] " TENSOR_FLAGS_USAGE " frame.nv12 W H PITCH DW DH TYPE FOURCC PLANES NORM L T R B [L T R B ...]\n"); return 200; }
    const int W = atoi(argv[2]), H = atoi(argv[3]), P = atoi(argv[4]);
    const int DW = atoi(argv[5]), DH = atoi(argv[6]), type = atoi(argv[7]);
    const int fcc = atoi(argv[8]), planes = atoi(argv[9]), norm = atoi(argv[10]);
    std::vector<tsvpp_roi> rois;
    for (int a = 11; a + 3 < argc; a += 4) rois.push_back(tsvpp_roi{ 0, atoi(argv[a]), atoi(argv[a + 1]), atoi(argv[a + 2]), atoi(argv[a + 3]) });
    std::vector<uint8_t> host((size_t)P * H * 3 / 2);
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(host.data(), 1, host.size(), f) != host.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 201; }
    fclose(f);
    uint8_t *dY = nullptr, *dUV = nullptr;
    if (hipMalloc(&dY, (size_t)P * H) != hipSuccess || hipMalloc(&dUV, (size_t)P * H / 2) != hipSuccess) return 202;
    (void)hipMemcpy(dY, host.data(), (size_t)P * H, hipMemcpyHostToDevice);
    (void)hipMemcpy(dUV, host.data() + (size_t)P * H, (size_t)P * H / 2, hipMemcpyHostToDevice);

    VideoProcessor vpp;
    if (vpp.Init(std::make_shared<Logger>()) != 0) return 203;
    AVFrame *input = av_frame_alloc();
    input->data[0] = dY;
    input->data[1] = dUV;
    input->linesize[0] = input->linesize[1] = P;
    input->width = W;
    input->height = H;
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
    if (hipMalloc(&dOut, stride * rois.size()) != hipSuccess) return 204;
    std::vector<void *> outs(rois.size());
    for (size_t i = 0; i < rois.size(); i++) outs[i] = dOut + i * stride;
    AVFrame *inputs[1] = { input };
    const int sts = tensor ? vpp.ConvertRois(inputs, 1, rois.data(), (int)rois.size(), outs.data(), options, &spec, "rois")
                    : area ? vpp.ConvertRoisArea(inputs, 1, rois.data(), (int)rois.size(), outs.data(), options, "rois")
                           : vpp.ConvertRois(inputs, 1, rois.data(), (int)rois.size(), outs.data(), options, "rois");
    if (sts != 0) return 210;
    if (tsvpp_consumer_synchronize(vpp.context(), "rois") != 0) return 211; // the conversion is asynchronous, on the consumer's stream
    std::vector<uint8_t> result(bytes);
    for (size_t i = 0; i < rois.size(); i++) {
        if (hipMemcpy(result.data(), outs[i], bytes, hipMemcpyDeviceToHost) != hipSuccess) return 212;
        printf("%zu %u %zu\n", i, crc32_av(result.data(), bytes), bytes);
    }
    // a box outside its frame is refused with the reference's status convention, and nothing is launched
    tsvpp_roi bad{ 0, 0, 0, W + 2, 2 };
    void *one[1] = { dOut };
    const int refused = tensor ? vpp.ConvertRois(inputs, 1, &bad, 1, one, options, &spec, "rois")
                        : area ? vpp.ConvertRoisArea(inputs, 1, &bad, 1, one, options, "rois")
                               : vpp.ConvertRois(inputs, 1, &bad, 1, one, options, "rois");
    if (refused != VREADER_ERROR) return 213;
    av_frame_free(&input);
    vpp.Close();
    (void)hipFree(dOut);
    (void)hipFree(dY);
    (void)hipFree(dUV);
    return 0;
}
