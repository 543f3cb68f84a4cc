// vpp_rois_p010 -- converts a handful of boxes of one P010 frame through the C++ class (VideoProcessor::ConvertRoisP010) and prints a CRC-32 per box (zlib's);
// tests/test_gpu_rois_p010.py compares each with the CRC of the expected output (tests/p010_util.py).
//   vpp_rois_p010 [--dtype f16|bf16|f32] [--mean a,b,c] [--scale a,b,c] frame.p010 W H PITCH  DW DH TYPE  FOURCC PLANES NORM  L T R B [L T R B ...]
// --dtype / --mean / --scale: through the overload that takes a tsvpp_tensor_spec.
// The file holds H rows of PITCH BYTES of luma words, then H / 2 rows of PITCH bytes of chroma words (little-endian).  Prints "<index> <crc> <bytes>" per box;
// exit code 0 = converted.
#include "check_common.h"

int main(int argc, char **argv) {
    tsvpp_tensor_spec spec;
    const bool tensor = tensor_flags(argc, argv, spec);
    if (argc < 15 || (argc - 11) % 4 != 0) {
        fprintf(stderr, "usage: vpp_rois_p010 " TENSOR_FLAGS_USAGE " frame.p010 W H PITCH DW DH TYPE FOURCC PLANES NORM L T R B [L T R B ...]\n");
        return 200;
    }
    const int W = atoi(argv[2]), H = atoi(argv[3]), P = atoi(argv[4]);
    const int DW = atoi(argv[5]), DH = atoi(argv[6]), type = atoi(argv[7]);
    const int fcc = atoi(argv[8]), planes = atoi(argv[9]), norm = atoi(argv[10]);
    std::vector<tsvpp_roi> rois;
    for (int a = 11; a + 3 < argc; a += 4) rois.push_back(tsvpp_roi{ 0, atoi(argv[a]), atoi(argv[a + 1]), atoi(argv[a + 2]), atoi(argv[a + 3]) });
    uint8_t *dY = nullptr, *dUV = nullptr;
    if (int sts = load_nv12(argv[1], H, P, dY, dUV)) return sts; // (rows of P bytes: the same file layout)

    VideoProcessor vpp;
    if (vpp.Init(std::make_shared<Logger>()) != 0) return 203;
    AVFrame *input = nv12_frame(dY, dUV, W, H, P);
    FrameParameters options = frame_parameters(DW, DH, type, fcc, planes, norm);
    size_t bytes = 0;
    if (int sts = output_bytes(DW, DH, type, fcc, planes, norm, tensor ? &spec : nullptr, bytes)) return sts;
    OutputArena arena;
    if (int sts = arena.carve(rois.size(), bytes)) return sts;
    AVFrame *inputs[1] = { input };
    const auto convert = [&](const tsvpp_roi *boxes, int n, void *const *outs) {
        return tensor ? vpp.ConvertRoisP010(inputs, 1, boxes, n, outs, options, &spec, "rois_p010") : vpp.ConvertRoisP010(inputs, 1, boxes, n, outs, options, "rois_p010");
    };
    if (convert(rois.data(), (int)rois.size(), arena.outs.data()) != 0) return 210;
    if (int failed = print_outputs(vpp, "rois_p010", arena, crc32_zlib)) return failed;
    // a box outside its frame is refused with the reference's status convention, a box at an odd origin as not supported, and nothing is launched
    const tsvpp_roi outside{ 0, 0, 0, W + 2, 2 }, odd{ 0, 1, 0, 3, 2 };
    void *one[1] = { arena.base };
    if (convert(&outside, 1, one) != VREADER_ERROR) return 213;
    if (convert(&odd, 1, one) == 0) return 214;
    av_frame_free(&input);
    vpp.Close();
    arena.release();
    (void)hipFree(dY);
    (void)hipFree(dUV);
    return 0;
}
