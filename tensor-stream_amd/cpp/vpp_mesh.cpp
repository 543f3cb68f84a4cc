// vpp_mesh -- samples one NV12 frame through a handful of warp meshes with the C++ class (VideoProcessor::ConvertMesh) and prints a CRC-32 per output (the
// zlib / IEEE 802.3 one: reflected 0xEDB88320, as Python's zlib.crc32); tests/test_cpp_mesh_gpu.py compares each with the CRC of the expected output.
//   vpp_mesh [--dtype f16|bf16|f32] [--mean a,b,c] [--scale a,b,c] DW DH FOURCC PLANES NORM BY BU BV frame.nv12 W H PITCH LOG2_CW LOG2_CH  mesh.f32 [mesh.f32 ...]
// --dtype / --mean / --scale: through the ConvertMesh overload that takes a tsvpp_tensor_spec.  BY BU BV: the border sample, or -1 -1 -1 to replicate the edge.
// A mesh file is raw fp32: tsvpp_mesh_dims' rows of cols (x, y) control points, tight.  The frame file holds H rows of PITCH bytes of luma, then H / 2 rows of
// PITCH bytes of chroma.  Output k samples the frame through mesh k.  Prints "<index> <crc> <bytes>" per output; exit code 0 = converted.
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
    if (argc < 16) {
        fprintf(stderr, "usage: vpp_mesh " TENSOR_FLAGS_USAGE " DW DH FOURCC PLANES NORM BY BU BV frame.nv12 W H PITCH LOG2_CW LOG2_CH mesh.f32 [mesh.f32 ...]\n");
        return 200;
    }
    const int DW = atoi(argv[1]), DH = atoi(argv[2]), fcc = atoi(argv[3]), planes = atoi(argv[4]), norm = atoi(argv[5]);
    const int bY = atoi(argv[6]), bU = atoi(argv[7]), bV = atoi(argv[8]);
    const char *path = argv[9];
    const int W = atoi(argv[10]), H = atoi(argv[11]), P = atoi(argv[12]);
    const int lcw = atoi(argv[13]), lch = atoi(argv[14]);
    const int n = argc - 15;
    int cols = 0, rows = 0;
    if (DW <= 0 || DH <= 0 || W <= 0 || H <= 0 || P < W || tsvpp_mesh_dims(DW, DH, lcw, lch, &cols, &rows) != 0) return 200;
    std::vector<uint8_t> host((size_t)P * H * 3 / 2);
    FILE *f = fopen(path, "rb");
    if (!f || fread(host.data(), 1, host.size(), f) != host.size()) { fprintf(stderr, "cannot read %s\n", path); return 201; }
    fclose(f);
    uint8_t *dY = nullptr, *dUV = nullptr;
    if (hipMalloc(&dY, (size_t)P * H) != hipSuccess || hipMalloc(&dUV, (size_t)P * H / 2) != hipSuccess) return 202;
    (void)hipMemcpy(dY, host.data(), (size_t)P * H, hipMemcpyHostToDevice);
    (void)hipMemcpy(dUV, host.data() + (size_t)P * H, (size_t)P * H / 2, hipMemcpyHostToDevice);
    // the meshes: one device allocation, mesh k at k * map_bytes (a multiple of 8)
    const size_t map_bytes = (size_t)cols * rows * 2 * sizeof(float);
    std::vector<uint8_t> map_host(map_bytes);
    uint8_t *dMaps = nullptr;
    if (hipMalloc(&dMaps, map_bytes * (size_t)n) != hipSuccess) return 202;
    std::vector<tsvpp_mesh> maps((size_t)n);
    std::vector<tsvpp_remap> remaps((size_t)n);
    for (int k = 0; k < n; k++) {
        FILE *m = fopen(argv[15 + k], "rb");
        if (!m || fread(map_host.data(), 1, map_bytes, m) != map_bytes) { fprintf(stderr, "cannot read %s\n", argv[15 + k]); return 201; }
        fclose(m);
        (void)hipMemcpy(dMaps + (size_t)k * map_bytes, map_host.data(), map_bytes, hipMemcpyHostToDevice);
        maps[(size_t)k] = tsvpp_mesh{ (const float *)(dMaps + (size_t)k * map_bytes), 0, lcw, lch, 0 };
        remaps[(size_t)k] = tsvpp_remap{ 0, k };
    }
    AVFrame *input = av_frame_alloc();
    input->data[0] = dY;
    input->data[1] = dUV;
    input->linesize[0] = input->linesize[1] = P;
    input->width = W;
    input->height = H;
    AVFrame *inputs[1] = { input };

    VideoProcessor vpp;
    if (vpp.Init(std::make_shared<Logger>()) != 0) return 203;
    ColorOptions color((FourCC)fcc);
    color.planesPos = (Planes)planes;
    color.normalization = norm != 0;
    ResizeOptions resize(DW, DH);
    resize.type = (ResizeType)TSVPP_BILINEAR;
    FrameParameters options(resize, color);
    size_t bytes = (size_t)(channelsByFourCC((FourCC)fcc) * (float)DW) * (size_t)DH * (norm ? sizeof(float) : 1);
    if (tensor) {
        const tsvpp_params flat{ 0, 0, 0, 0, DW, DH, TSVPP_BILINEAR, fcc, planes, norm };
        bytes = tsvpp_tensor_bytes(&flat, &spec);
        if (bytes == 0) return 205; // a (parameters, spec) pair the tensor entry points refuse
    }
    const size_t stride = (bytes + 255) & ~(size_t)255;
    uint8_t *dOut = nullptr;
    if (hipMalloc(&dOut, stride * (size_t)n) != hipSuccess) return 204;
    std::vector<void *> outs((size_t)n);
    for (int k = 0; k < n; k++) outs[(size_t)k] = dOut + (size_t)k * stride;
    const int sts = tensor ? vpp.ConvertMesh(inputs, 1, maps.data(), n, remaps.data(), n, bY, bU, bV, outs.data(), options, &spec, "mesh")
                           : vpp.ConvertMesh(inputs, 1, maps.data(), n, remaps.data(), n, bY, bU, bV, outs.data(), options, "mesh");
    if (sts != 0) return 210;
    if (tsvpp_consumer_synchronize(vpp.context(), "mesh") != 0) return 211; // the conversion is asynchronous, on the consumer's stream
    std::vector<uint8_t> result(bytes);
    for (int k = 0; k < n; k++) {
        if (hipMemcpy(result.data(), outs[(size_t)k], bytes, hipMemcpyDeviceToHost) != hipSuccess) return 212;
        printf("%d %u %zu\n", k, crc32_zlib(result.data(), bytes), bytes);
    }
    // a mesh index that was not given is refused with the reference's status convention, and nothing is launched
    const tsvpp_remap bad = { 0, n };
    const int refused = tensor ? vpp.ConvertMesh(inputs, 1, maps.data(), n, &bad, 1, bY, bU, bV, outs.data(), options, &spec, "mesh")
                               : vpp.ConvertMesh(inputs, 1, maps.data(), n, &bad, 1, bY, bU, bV, outs.data(), options, "mesh");
    if (refused != VREADER_ERROR) return 214;
    av_frame_free(&input);
    vpp.Close();
    (void)hipFree(dOut);
    (void)hipFree(dMaps);
    (void)hipFree(dY);
    (void)hipFree(dUV);
    return 0;
}
