// vpp_rois -- converts a handful of boxes of one NV12 frame through the C++ class (VideoProcessor::ConvertRois) and prints a CRC-32 per box
// (libavutil's AV_CRC_32_IEEE, as vpp_goldens computes it); tests/test_cpp_rois_gpu.py compares each with the oracle's.
//   vpp_rois [--area] [--dtype f16|bf16|f32] [--mean a,b,c] [--scale a,b,c] frame.nv12 W H PITCH  DW DH TYPE  FOURCC PLANES NORM  L T R B [L T R B ...]
// --area: through VideoProcessor::ConvertRoisArea (TYPE must then be 3, AREA; tests/test_cpp_rois_area_gpu.py).
// --dtype / --mean / --scale: through the ConvertRois overload that takes a tsvpp_tensor_spec (any TYPE; tests/test_cpp_tensor_gpu.py); without them the
// output is byte for byte what it was.
// The file holds H rows of PITCH bytes of luma, then H / 2 rows of PITCH bytes of chroma.  Prints "<index> <crc> <bytes>" per box; exit code 0 = converted.
#include "check_common.h"

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
    uint8_t *dY = nullptr, *dUV = nullptr;
    if (int sts = load_nv12(argv[1], H, P, dY, dUV)) return sts;

    VideoProcessor vpp;
    if (vpp.Init(std::make_shared<Logger>()) != 0) return 203;
    AVFrame *input = nv12_frame(dY, dUV, W, H, P);
    FrameParameters options = frame_parameters(DW, DH, type, fcc, planes, norm);
    size_t bytes = 0;
    if (int sts = output_bytes(DW, DH, type, fcc, planes, norm, tensor ? &spec : nullptr, bytes)) return sts;
    OutputArena arena;
    if (int sts = arena.carve(rois.size(), bytes)) return sts;
    AVFrame *inputs[1] = { input };
    const int sts = tensor ? vpp.ConvertRois(inputs, 1, rois.data(), (int)rois.size(), arena.outs.data(), options, &spec, "rois")
                    : area ? vpp.ConvertRoisArea(inputs, 1, rois.data(), (int)rois.size(), arena.outs.data(), options, "rois")
                           : vpp.ConvertRois(inputs, 1, rois.data(), (int)rois.size(), arena.outs.data(), options, "rois");
    if (sts != 0) return 210;
    if (int failed = print_outputs(vpp, "rois", arena, crc32_av)) return failed;
    // a box outside its frame is refused with the reference's status convention, and nothing is launched
    tsvpp_roi bad{ 0, 0, 0, W + 2, 2 };
    void *one[1] = { arena.base };
    const int refused = tensor ? vpp.ConvertRois(inputs, 1, &bad, 1, one, options, &spec, "rois")
                        : area ? vpp.ConvertRoisArea(inputs, 1, &bad, 1, one, options, "rois")
                               : vpp.ConvertRois(inputs, 1, &bad, 1, one, options, "rois");
    if (refused != VREADER_ERROR) return 213;
    av_frame_free(&input);
    vpp.Close();
    arena.release();
    (void)hipFree(dY);
    (void)hipFree(dUV);
    return 0;
}
