// vpp_warp -- samples a handful of affine warps out of one NV12 frame through the C++ class (VideoProcessor::ConvertWarp) and prints a CRC-32 per output (the
// zlib / IEEE 802.3 one: reflected 0xEDB88320, as Python's zlib.crc32); tests/test_cpp_warp_gpu.py compares each with the CRC of the expected output.
//   vpp_warp [--bicubic] [--dtype f16|bf16|f32] [--mean a,b,c] [--scale a,b,c] DW DH FOURCC PLANES NORM BY BU BV frame.nv12 W H PITCH  m0 m1 m2 m3 m4 m5 [m0 ... m5 ...]
// --bicubic: through VideoProcessor::ConvertWarpBicubic (BICUBIC in place of BILINEAR; tests/test_cpp_warp_bicubic_gpu.py).
// --dtype / --mean / --scale: through the ConvertWarp overload that takes a tsvpp_tensor_spec.  BY BU BV: the border sample, or -1 -1 -1 to replicate the edge.
// The matrix entries are read with strtod (C99 hexadecimal floats keep every bit) and must be float values.  The file holds H rows of PITCH bytes of luma, then
// H / 2 rows of PITCH bytes of chroma.  Prints "<index> <crc> <bytes>" per output; exit code 0 = converted.
#include "check_common.h"

int main(int argc, char **argv) {
    const bool cubic = argc > 1 && strcmp(argv[1], "--bicubic") == 0;
    if (cubic) {
        argv++;
        argc--;
    }
    tsvpp_tensor_spec spec;
    const bool tensor = tensor_flags(argc, argv, spec);
    if (argc < 19 || (argc - 13) % 6 != 0) {
        fprintf(stderr, "usage: vpp_warp [--bicubic] " TENSOR_FLAGS_USAGE " DW DH FOURCC PLANES NORM BY BU BV frame.nv12 W H PITCH m0 m1 m2 m3 m4 m5 [m0 ... m5 ...]\n");
        return 200;
    }
    const int DW = atoi(argv[1]), DH = atoi(argv[2]), fcc = atoi(argv[3]), planes = atoi(argv[4]), norm = atoi(argv[5]);
    const int bY = atoi(argv[6]), bU = atoi(argv[7]), bV = atoi(argv[8]);
    const char *path = argv[9];
    const int W = atoi(argv[10]), H = atoi(argv[11]), P = atoi(argv[12]);
    std::vector<tsvpp_warp> warps;
    for (int a = 13; a + 5 < argc; a += 6) {
        tsvpp_warp w = {};
        for (int k = 0; k < 6; k++) w.m[k] = (float)strtod(argv[a + k], nullptr);
        warps.push_back(w);
    }
    const int n = (int)warps.size();
    uint8_t *dY = nullptr, *dUV = nullptr;
    if (int sts = load_nv12(path, H, P, dY, dUV)) return sts;
    AVFrame *input = nv12_frame(dY, dUV, W, H, P);
    AVFrame *inputs[1] = { input };

    VideoProcessor vpp;
    if (vpp.Init(std::make_shared<Logger>()) != 0) return 203;
    const int type = cubic ? TSVPP_BICUBIC : TSVPP_BILINEAR;
    FrameParameters options = frame_parameters(DW, DH, type, fcc, planes, norm);
    size_t bytes = 0;
    if (int sts = output_bytes(DW, DH, type, fcc, planes, norm, tensor ? &spec : nullptr, bytes)) return sts;
    OutputArena arena;
    if (int sts = arena.carve((size_t)n, bytes)) return sts;
    // the four forms: BILINEAR or --bicubic, plain or with the tensor spec (the BICUBIC method's spec may be null)
    const auto convert = [&](const tsvpp_warp *items, int cnt) {
        if (cubic) return vpp.ConvertWarpBicubic(inputs, 1, items, cnt, bY, bU, bV, arena.outs.data(), options, tensor ? &spec : nullptr, "warp");
        return tensor ? vpp.ConvertWarp(inputs, 1, items, cnt, bY, bU, bV, arena.outs.data(), options, &spec, "warp")
                      : vpp.ConvertWarp(inputs, 1, items, cnt, bY, bU, bV, arena.outs.data(), options, "warp");
    };
    const int sts = convert(warps.data(), n);
    if (sts != 0) return 210;
    if (int failed = print_outputs(vpp, "warp", arena, crc32_zlib)) return failed;
    // a matrix of another frame than the one given is refused with the reference's status convention, and nothing is launched
    tsvpp_warp bad = warps[0];
    bad.frame = 1;
    const int refused = convert(&bad, 1);
    if (refused != VREADER_ERROR) return 214;
    av_frame_free(&input);
    vpp.Close();
    arena.release();
    (void)hipFree(dY);
    (void)hipFree(dUV);
    return 0;
}
