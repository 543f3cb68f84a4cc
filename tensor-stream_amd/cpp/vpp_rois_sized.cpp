// vpp_rois_sized -- converts a handful of boxes of one NV12 frame, each to its own output size, through the C++ class (VideoProcessor::ConvertRoisSized) and
// prints a CRC-32 per box (libavutil's AV_CRC_32_IEEE, as vpp_goldens computes it); tests/test_cpp_rois_sized_gpu.py compares each with the oracle's.
//   vpp_rois_sized [--dtype f16|bf16|f32] [--mean a,b,c] [--scale a,b,c] frame.nv12 W H PITCH  TYPE  FOURCC PLANES NORM  L T R B DW DH [L T R B DW DH ...]
// --dtype / --mean / --scale: through the ConvertRoisSized overload that takes a tsvpp_tensor_spec.
// The file holds H rows of PITCH bytes of luma, then H / 2 rows of PITCH bytes of chroma.  Prints "<index> <crc> <bytes>" per box; exit code 0 = converted, and
// the refused request behind it was refused.
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
    tsvpp_tensor_spec spec;
    const bool tensor = tensor_flags(argc, argv, spec);
    if (argc < 15 || (argc - 9) % 6 != 0) { fprintf(stderr, "usage: vpp_rois_sized " TENSOR_FLAGS_USAGE " frame.nv12 W H PITCH TYPE FOURCC PLANES NORM L T R B DW DH [L T R B DW DH ...]\n"); return 200; }
    const int W = atoi(argv[2]), H = atoi(argv[3]), P = atoi(argv[4]);
    const int type = atoi(argv[5]), fcc = atoi(argv[6]), planes = atoi(argv[7]), norm = atoi(argv[8]);
    std::vector<tsvpp_roi_sized> rois;
    for (int a = 9; a + 5 < argc; a += 6)
        rois.push_back(tsvpp_roi_sized{ 0, atoi(argv[a]), atoi(argv[a + 1]), atoi(argv[a + 2]), atoi(argv[a + 3]), atoi(argv[a + 4]), atoi(argv[a + 5]) });
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
    ResizeOptions resize(0, 0); // the sizes are the boxes'
    resize.type = (ResizeType)type;
    FrameParameters options(resize, color);
    const tsvpp_params flat{ 0, 0, 0, 0, 0, 0, type, fcc, planes, norm };
    std::vector<size_t> bytes(rois.size()), offs(rois.size());
    size_t total = 0;
    for (size_t i = 0; i < rois.size(); i++) {
        bytes[i] = tsvpp_rois_sized_bytes(&flat, tensor ? &spec : nullptr, rois[i].dst_width, rois[i].dst_height);
        if (bytes[i] == 0) return 205; // a request the entry points refuse
        offs[i] = total;
        total += (bytes[i] + 255) & ~(size_t)255;
    }
    uint8_t *dOut = nullptr;
    if (hipMalloc(&dOut, total) != hipSuccess) return 204;
    std::vector<void *> outs(rois.size());
    for (size_t i = 0; i < rois.size(); i++) outs[i] = dOut + offs[i];
    AVFrame *inputs[1] = { input };
    const int sts = tensor ? vpp.ConvertRoisSized(inputs, 1, rois.data(), (int)rois.size(), outs.data(), options, &spec, "rois")
                           : vpp.ConvertRoisSized(inputs, 1, rois.data(), (int)rois.size(), outs.data(), options, "rois");
    if (sts != 0) return 210;
    if (tsvpp_consumer_synchronize(vpp.context(), "rois") != 0) return 211; // the conversion is asynchronous, on the consumer's stream
    std::vector<uint8_t> result;
    for (size_t i = 0; i < rois.size(); i++) {
        result.resize(bytes[i]);
        if (hipMemcpy(result.data(), outs[i], bytes[i], hipMemcpyDeviceToHost) != hipSuccess) return 212;
        printf("%zu %u %zu\n", i, crc32_av(result.data(), bytes[i]), bytes[i]);
    }
    // a request that sets the parameters' own output size is refused with the reference's status convention, and nothing is launched
    ResizeOptions sized(rois[0].dst_width, rois[0].dst_height);
    sized.type = (ResizeType)type;
    FrameParameters wrong(sized, color);
    const int refused = tensor ? vpp.ConvertRoisSized(inputs, 1, rois.data(), 1, outs.data(), wrong, &spec, "rois")
                               : vpp.ConvertRoisSized(inputs, 1, rois.data(), 1, outs.data(), wrong, "rois");
    if (refused != VREADER_ERROR) return 213;
    av_frame_free(&input);
    vpp.Close();
    (void)hipFree(dOut);
    (void)hipFree(dY);
    (void)hipFree(dUV);
    return 0;
}
