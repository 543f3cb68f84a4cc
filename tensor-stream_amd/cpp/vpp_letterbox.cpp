// vpp_letterbox -- letterboxes a few NV12 frames into canvases of one size through the C++ class (VideoProcessor::ConvertLetterbox) and prints a CRC-32 per canvas
// (the zlib / IEEE 802.3 one: reflected 0xEDB88320, as Python's zlib.crc32); tests/test_cpp_letterbox_gpu.py compares each with the CRC of the expected canvas.
//   vpp_letterbox [--area] [--dtype f16|bf16|f32] [--mean a,b,c] [--scale a,b,c] DW DH TYPE FOURCC PLANES NORM PADY PADU PADV  frame.nv12 W H PITCH [frame.nv12 W H PITCH ...]
// --area: through VideoProcessor::ConvertLetterboxArea (TYPE must then be 3, AREA; tests/test_cpp_letterbox_area_gpu.py).
// --dtype / --mean / --scale: through the ConvertLetterbox overload that takes a tsvpp_tensor_spec (tests/test_cpp_tensor_gpu.py); without them the output is byte
// for byte what it was.
// A file holds H rows of PITCH bytes of luma, then H / 2 rows of PITCH bytes of chroma.  Every frame gets the default rectangle (tsvpp_letterbox_rect).  Prints
// "<index> <crc> <bytes> <left> <top> <width> <height>" per canvas; exit code 0 = converted.
#include "check_common.h"

int main(int argc, char **argv) {
    const bool area = argc > 1 && strcmp(argv[1], "--area") == 0;
    if (area) {
        argv++;
        argc--;
    }
    tsvpp_tensor_spec spec;
    const bool tensor = tensor_flags(argc, argv, spec);
    if (argc < 14 || (argc - 10) % 4 != 0) {
        fprintf(stderr, "usage: vpp_letterbox [--area] " TENSOR_FLAGS_USAGE " DW DH TYPE FOURCC PLANES NORM PADY PADU PADV frame.nv12 W H PITCH [frame.nv12 W H PITCH ...]\n");
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
        uint8_t *dY = nullptr, *dUV = nullptr;
        if (int sts = load_nv12(path, H, P, dY, dUV)) return sts;
        inputs.push_back(nv12_frame(dY, dUV, W, H, P));
        planesDev.push_back(dY);
        planesDev.push_back(dUV);
    }

    VideoProcessor vpp;
    if (vpp.Init(std::make_shared<Logger>()) != 0) return 203;
    FrameParameters options = frame_parameters(DW, DH, type, fcc, planes, norm);
    size_t bytes = 0;
    if (int sts = output_bytes(DW, DH, type, fcc, planes, norm, tensor ? &spec : nullptr, bytes)) return sts;
    OutputArena arena;
    if (int sts = arena.carve((size_t)n, bytes)) return sts;
    // one request through the method the flags name
    const auto convert = [&](int count, const tsvpp_rect *rects) {
        if (area) {
            return tensor ? vpp.ConvertLetterboxArea(inputs.data(), count, rects, padY, padU, padV, arena.outs.data(), options, &spec, "letterbox")
                          : vpp.ConvertLetterboxArea(inputs.data(), count, rects, padY, padU, padV, arena.outs.data(), options, "letterbox");
        }
        return tensor ? vpp.ConvertLetterbox(inputs.data(), count, rects, padY, padU, padV, arena.outs.data(), options, &spec, "letterbox")
                      : vpp.ConvertLetterbox(inputs.data(), count, rects, padY, padU, padV, arena.outs.data(), options, "letterbox");
    };
    const int sts = convert(n, nullptr);
    if (sts != 0) return 210;
    const int printed = print_outputs(vpp, "letterbox", arena, crc32_zlib, [&](size_t k, std::string &line_end) {
        tsvpp_rect r = {};
        if (tsvpp_letterbox_rect(inputs[k]->width, inputs[k]->height, DW, DH, &r) != 0) return 213;
        char rect[64];
        snprintf(rect, sizeof(rect), " %d %d %d %d", r.left, r.top, r.width, r.height);
        line_end = rect;
        return 0;
    });
    if (printed != 0) return printed;
    // a rectangle outside the canvas is refused with the reference's status convention, and nothing is launched
    const tsvpp_rect bad{ 0, 0, DW + 2, 2 };
    const int refused = convert(1, &bad);
    if (refused != VREADER_ERROR) return 214;
    for (AVFrame *f : inputs) av_frame_free(&f);
    vpp.Close();
    arena.release();
    for (uint8_t *p : planesDev) (void)hipFree(p);
    return 0;
}
