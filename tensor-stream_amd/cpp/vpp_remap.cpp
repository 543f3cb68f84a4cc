// vpp_remap -- samples one NV12 frame through a handful of coordinate maps with the C++ class (VideoProcessor::ConvertRemap) and prints a CRC-32 per output (the
// zlib / IEEE 802.3 one: reflected 0xEDB88320, as Python's zlib.crc32); tests/test_cpp_remap_gpu.py compares each with the CRC of the expected output.
//   vpp_remap [--dtype f16|bf16|f32] [--mean a,b,c] [--scale a,b,c] DW DH FOURCC PLANES NORM BY BU BV frame.nv12 W H PITCH  map.f32 [map.f32 ...]
// --dtype / --mean / --scale: through the ConvertRemap overload that takes a tsvpp_tensor_spec.  BY BU BV: the border sample, or -1 -1 -1 to replicate the edge.
// A map file is raw fp32: DH rows of DW (x, y) pairs, tight.  The frame file holds H rows of PITCH bytes of luma, then H / 2 rows of PITCH bytes of chroma.
// Output k samples the frame through map k.  Prints "<index> <crc> <bytes>" per output; exit code 0 = converted.
#include "check_common.h"

int main(int argc, char **argv) {
    tsvpp_tensor_spec spec;
    const bool tensor = tensor_flags(argc, argv, spec);
    if (argc < 14) {
        fprintf(stderr, "usage: vpp_remap " TENSOR_FLAGS_USAGE " DW DH FOURCC PLANES NORM BY BU BV frame.nv12 W H PITCH map.f32 [map.f32 ...]\n");
        return 200;
    }
    const int DW = atoi(argv[1]), DH = atoi(argv[2]), fcc = atoi(argv[3]), planes = atoi(argv[4]), norm = atoi(argv[5]);
    const int bY = atoi(argv[6]), bU = atoi(argv[7]), bV = atoi(argv[8]);
    const char *path = argv[9];
    const int W = atoi(argv[10]), H = atoi(argv[11]), P = atoi(argv[12]);
    const int n = argc - 13;
    if (DW <= 0 || DH <= 0 || W <= 0 || H <= 0 || P < W) return 200;
    uint8_t *dY = nullptr, *dUV = nullptr;
    if (int sts = load_nv12(path, H, P, dY, dUV)) return sts;
    // the maps: one device allocation, map k at k * map_bytes (a multiple of 8)
    const size_t map_bytes = (size_t)DW * DH * 2 * sizeof(float);
    std::vector<uint8_t> map_host(map_bytes);
    uint8_t *dMaps = nullptr;
    if (hipMalloc(&dMaps, map_bytes * (size_t)n) != hipSuccess) return 202;
    std::vector<tsvpp_map> maps((size_t)n);
    std::vector<tsvpp_remap> remaps((size_t)n);
    for (int k = 0; k < n; k++) {
        if (!read_file(argv[13 + k], map_host.data(), map_bytes)) return 201;
        (void)hipMemcpy(dMaps + (size_t)k * map_bytes, map_host.data(), map_bytes, hipMemcpyHostToDevice);
        maps[(size_t)k] = tsvpp_map{ (const float *)(dMaps + (size_t)k * map_bytes), 0, 0 };
        remaps[(size_t)k] = tsvpp_remap{ 0, k };
    }
    AVFrame *input = nv12_frame(dY, dUV, W, H, P);
    AVFrame *inputs[1] = { input };

    VideoProcessor vpp;
    if (vpp.Init(std::make_shared<Logger>()) != 0) return 203;
    FrameParameters options = frame_parameters(DW, DH, TSVPP_BILINEAR, fcc, planes, norm);
    size_t bytes = 0;
    if (int sts = output_bytes(DW, DH, TSVPP_BILINEAR, fcc, planes, norm, tensor ? &spec : nullptr, bytes)) return sts;
    OutputArena arena;
    if (int sts = arena.carve((size_t)n, bytes)) return sts;
    const int sts = tensor ? vpp.ConvertRemap(inputs, 1, maps.data(), n, remaps.data(), n, bY, bU, bV, arena.outs.data(), options, &spec, "remap")
                           : vpp.ConvertRemap(inputs, 1, maps.data(), n, remaps.data(), n, bY, bU, bV, arena.outs.data(), options, "remap");
    if (sts != 0) return 210;
    if (int failed = print_outputs(vpp, "remap", arena, crc32_zlib)) return failed;
    // a map index that was not given is refused with the reference's status convention, and nothing is launched
    const tsvpp_remap bad = { 0, n };
    const int refused = tensor ? vpp.ConvertRemap(inputs, 1, maps.data(), n, &bad, 1, bY, bU, bV, arena.outs.data(), options, &spec, "remap")
                               : vpp.ConvertRemap(inputs, 1, maps.data(), n, &bad, 1, bY, bU, bV, arena.outs.data(), options, "remap");
    if (refused != VREADER_ERROR) return 214;
    av_frame_free(&input);
    vpp.Close();
    arena.release();
    (void)hipFree(dMaps);
    (void)hipFree(dY);
    (void)hipFree(dUV);
    return 0;
}
