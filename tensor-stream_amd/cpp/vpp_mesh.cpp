// vpp_mesh -- samples one NV12 frame through a handful of warp meshes with the C++ class (VideoProcessor::ConvertMesh) and prints a CRC-32 per output (the
// zlib / IEEE 802.3 one: reflected 0xEDB88320, as Python's zlib.crc32); tests/test_cpp_mesh_gpu.py compares each with the CRC of the expected output.
//   vpp_mesh [--dtype f16|bf16|f32] [--mean a,b,c] [--scale a,b,c] DW DH FOURCC PLANES NORM BY BU BV frame.nv12 W H PITCH LOG2_CW LOG2_CH  mesh.f32 [mesh.f32 ...]
// --dtype / --mean / --scale: through the ConvertMesh overload that takes a tsvpp_tensor_spec.  BY BU BV: the border sample, or -1 -1 -1 to replicate the edge.
// A mesh file is raw fp32: tsvpp_mesh_dims' rows of cols (x, y) control points, tight.  The frame file holds H rows of PITCH bytes of luma, then H / 2 rows of
// PITCH bytes of chroma.  Output k samples the frame through mesh k.  Prints "<index> <crc> <bytes>" per output; exit code 0 = converted.
#include "check_common.h"

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
    uint8_t *dY = nullptr, *dUV = nullptr;
    if (int sts = load_nv12(path, H, P, dY, dUV)) return sts;
    // the meshes: one device allocation, mesh k at k * map_bytes (a multiple of 8)
    const size_t map_bytes = (size_t)cols * rows * 2 * sizeof(float);
    std::vector<uint8_t> map_host(map_bytes);
    uint8_t *dMaps = nullptr;
    if (hipMalloc(&dMaps, map_bytes * (size_t)n) != hipSuccess) return 202;
    std::vector<tsvpp_mesh> maps((size_t)n);
    std::vector<tsvpp_remap> remaps((size_t)n);
    for (int k = 0; k < n; k++) {
        if (!read_file(argv[15 + k], map_host.data(), map_bytes)) return 201;
        (void)hipMemcpy(dMaps + (size_t)k * map_bytes, map_host.data(), map_bytes, hipMemcpyHostToDevice);
        maps[(size_t)k] = tsvpp_mesh{ (const float *)(dMaps + (size_t)k * map_bytes), 0, lcw, lch, 0 };
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
    const int sts = tensor ? vpp.ConvertMesh(inputs, 1, maps.data(), n, remaps.data(), n, bY, bU, bV, arena.outs.data(), options, &spec, "mesh")
                           : vpp.ConvertMesh(inputs, 1, maps.data(), n, remaps.data(), n, bY, bU, bV, arena.outs.data(), options, "mesh");
    if (sts != 0) return 210;
    if (int failed = print_outputs(vpp, "mesh", arena, crc32_zlib)) return failed;
    // a mesh index that was not given is refused with the reference's status convention, and nothing is launched
    const tsvpp_remap bad = { 0, n };
    const int refused = tensor ? vpp.ConvertMesh(inputs, 1, maps.data(), n, &bad, 1, bY, bU, bV, arena.outs.data(), options, &spec, "mesh")
                               : vpp.ConvertMesh(inputs, 1, maps.data(), n, &bad, 1, bY, bU, bV, arena.outs.data(), options, "mesh");
    if (refused != VREADER_ERROR) return 214;
    av_frame_free(&input);
    vpp.Close();
    arena.release();
    (void)hipFree(dMaps);
    (void)hipFree(dY);
    (void)hipFree(dUV);
    return 0;
}
