// vpp_rois_sized -- converts a handful of boxes of one NV12 frame, each to its own output size, through the C++ class (VideoProcessor::ConvertRoisSized) and
// prints a CRC-32 per box (libavutil's AV_CRC_32_IEEE, as vpp_goldens computes it); tests/test_cpp_rois_sized_gpu.py compares each with the oracle's.
//   vpp_rois_sized [--dtype f16|bf16|f32] [--mean a,b,c] [--scale a,b,c] frame.nv12 W H PITCH  TYPE  FOURCC PLANES NORM  L T R B DW DH [L T R B DW DH ...]
// --dtype / --mean / --scale: through the ConvertRoisSized overload that takes a tsvpp_tensor_spec.
// The file holds H rows of PITCH bytes of luma, then H / 2 rows of PITCH bytes of chroma.  Prints "<index> <crc> <bytes>" per box; exit code 0 = converted, and
// the refused request behind it was refused.
#include "check_common.h"

int main(int argc, char **argv) {
    tsvpp_tensor_spec spec;
    const bool tensor = tensor_flags(argc, argv, spec);
    if (argc < 15 || (argc - 9) % 6 != 0) { fprintf(stderr, "usage: vpp_rois_sized " TENSOR_FLAGS_USAGE " frame.nv12 W H PITCH TYPE FOURCC PLANES NORM L T R B DW DH [L T R B DW DH ...]\n"); return 200; }
    const int W = atoi(argv[2]), H = atoi(argv[3]), P = atoi(argv[4]);
    const int type = atoi(argv[5]), fcc = atoi(argv[6]), planes = atoi(argv[7]), norm = atoi(argv[8]);
    std::vector<tsvpp_roi_sized> rois;
    for (int a = 9; a + 5 < argc; a += 6)
        rois.push_back(tsvpp_roi_sized{ 0, atoi(argv[a]), atoi(argv[a + 1]), atoi(argv[a + 2]), atoi(argv[a + 3]), atoi(argv[a + 4]), atoi(argv[a + 5]) });
    uint8_t *dY = nullptr, *dUV = nullptr;
    if (int sts = load_nv12(argv[1], H, P, dY, dUV)) return sts;

    VideoProcessor vpp;
    if (vpp.Init(std::make_shared<Logger>()) != 0) return 203;
    AVFrame *input = nv12_frame(dY, dUV, W, H, P);
    FrameParameters options = frame_parameters(0, 0, type, fcc, planes, norm); // the sizes are the boxes'
    const tsvpp_params flat{ 0, 0, 0, 0, 0, 0, type, fcc, planes, norm };
    std::vector<size_t> bytes(rois.size());
    for (size_t i = 0; i < rois.size(); i++) {
        bytes[i] = tsvpp_rois_sized_bytes(&flat, tensor ? &spec : nullptr, rois[i].dst_width, rois[i].dst_height);
        if (bytes[i] == 0) return 205; // a request the entry points refuse
    }
    OutputArena arena;
    if (int sts = arena.carve(bytes)) return sts;
    AVFrame *inputs[1] = { input };
    const int sts = tensor ? vpp.ConvertRoisSized(inputs, 1, rois.data(), (int)rois.size(), arena.outs.data(), options, &spec, "rois")
                           : vpp.ConvertRoisSized(inputs, 1, rois.data(), (int)rois.size(), arena.outs.data(), options, "rois");
    if (sts != 0) return 210;
    if (int failed = print_outputs(vpp, "rois", arena, crc32_av)) return failed;
    // a request that sets the parameters' own output size is refused with the reference's status convention, and nothing is launched
    FrameParameters wrong = frame_parameters(rois[0].dst_width, rois[0].dst_height, type, fcc, planes, norm);
    const int refused = tensor ? vpp.ConvertRoisSized(inputs, 1, rois.data(), 1, arena.outs.data(), wrong, &spec, "rois")
                               : vpp.ConvertRoisSized(inputs, 1, rois.data(), 1, arena.outs.data(), wrong, "rois");
    if (refused != VREADER_ERROR) return 213;
    av_frame_free(&input);
    vpp.Close();
    arena.release();
    (void)hipFree(dY);
    (void)hipFree(dUV);
    return 0;
}
