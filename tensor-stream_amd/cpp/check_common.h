// check_common.h -- what the check programs share (vpp_rois, vpp_rois_sized, vpp_letterbox, vpp_warp, vpp_persp, vpp_remap, vpp_mesh; the file, upload and CRC
// pieces also vpp_goldens and vpp_stages): the two CRC-32s, the optional tensor arguments, an NV12 file into two device planes and an AVFrame over them, the
// FrameParameters of a command line, the size of an output, the output arena, and the loop that prints one line per output.  The exit codes are the programs':
// 201 a file that cannot be read, 202 a device allocation of the inputs, 204 the output arena, 205 a tensor request without a size, 211 the consumer's
// synchronisation, 212 the copy back.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "VideoProcessor.h"

// av_crc(av_crc_get_table(AV_CRC_32_IEEE), -1, buf, n) as the reference's tests call it: libavutil's table is the MSB-first
// polynomial 0x04C11DB7 run on a byte-swapped state, no final xor (validated by the decoder test's plane CRCs, which vpp_goldens
// checks first: tests/src/DecoderTests.cpp:63-65).
static inline uint32_t crc32_av(const uint8_t *buf, size_t n) {
    uint32_t c = __builtin_bswap32(0xFFFFFFFFu);
    for (size_t i = 0; i < n; i++) {
        c ^= (uint32_t)buf[i] << 24;
        for (int k = 0; k < 8; k++) c = (c & 0x80000000u) ? (c << 1) ^ 0x04C11DB7u : (c << 1);
    }
    return __builtin_bswap32(c);
}
// the zlib / IEEE 802.3 one: reflected 0xEDB88320, as Python's zlib.crc32
static inline uint32_t crc32_zlib(const uint8_t *buf, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) {
        c ^= buf[i];
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : (c >> 1);
    }
    return c ^ 0xFFFFFFFFu;
}

#define TENSOR_FLAGS_USAGE "[--dtype f16|bf16|f32] [--mean a,b,c] [--scale a,b,c]"

// [--dtype f16|bf16|f32] [--mean a,b,c] [--scale a,b,c] in front of the positional arguments: fills `spec` (defaults: f32, mean 0, scale 1) and returns
// true when any was given; the arguments are shifted past the flags.
static inline bool tensor_flags(int &argc, char **&argv, tsvpp_tensor_spec &spec) {
    spec = tsvpp_tensor_spec{ TSVPP_F32, { 0.f, 0.f, 0.f }, { 1.f, 1.f, 1.f } };
    bool any = false;
    while (argc > 2 && (strcmp(argv[1], "--dtype") == 0 || strcmp(argv[1], "--mean") == 0 || strcmp(argv[1], "--scale") == 0)) {
        const char *v = argv[2];
        if (strcmp(argv[1], "--dtype") == 0) spec.dtype = strcmp(v, "f16") == 0 ? TSVPP_F16 : (strcmp(v, "bf16") == 0 ? TSVPP_BF16 : (strcmp(v, "f32") == 0 ? TSVPP_F32 : -1));
        else {
            float *dst = strcmp(argv[1], "--mean") == 0 ? spec.mean : spec.scale;
            if (sscanf(v, "%f,%f,%f", dst, dst + 1, dst + 2) != 3) dst[0] = dst[1] = dst[2] = __builtin_nanf(""); // (refused by the library: TSVPP_ERROR)
        }
        any = true;
        argv += 2;
        argc -= 2;
    }
    return any;
}

// `bytes` of a file, exactly; says so on stderr when it cannot
static inline bool read_file(const char *path, uint8_t *dst, size_t bytes) {
    FILE *f = fopen(path, "rb");
    const bool ok = f && fread(dst, 1, bytes, f) == bytes;
    if (f) fclose(f);
    if (!ok) fprintf(stderr, "cannot read %s\n", path);
    return ok;
}

// An NV12 file -- H rows of P bytes of luma, then H / 2 rows of P bytes of chroma -- read (201) ...
static inline int read_nv12(const char *path, int H, int P, std::vector<uint8_t> &host) {
    host.resize((size_t)P * H * 3 / 2);
    return read_file(path, host.data(), host.size()) ? 0 : 201;
}
// ... and uploaded into two device planes of its own (202)
static inline int upload_nv12(const std::vector<uint8_t> &host, int H, int P, uint8_t *&dY, uint8_t *&dUV) {
    dY = dUV = nullptr;
    if (hipMalloc(&dY, (size_t)P * H) != hipSuccess || hipMalloc(&dUV, (size_t)P * H / 2) != hipSuccess) return 202;
    (void)hipMemcpy(dY, host.data(), (size_t)P * H, hipMemcpyHostToDevice);
    (void)hipMemcpy(dUV, host.data() + (size_t)P * H, (size_t)P * H / 2, hipMemcpyHostToDevice);
    return 0;
}
static inline int load_nv12(const char *path, int H, int P, uint8_t *&dY, uint8_t *&dUV) {
    std::vector<uint8_t> host;
    if (int sts = read_nv12(path, H, P, host)) return sts;
    return upload_nv12(host, H, P, dY, dUV);
}

// a fresh AVFrame over the two planes: W x H, both pitches P
static inline AVFrame *nv12_frame(uint8_t *dY, uint8_t *dUV, int W, int H, int P) {
    AVFrame *frame = av_frame_alloc();
    frame->data[0] = dY;
    frame->data[1] = dUV;
    frame->linesize[0] = frame->linesize[1] = P;
    frame->width = W;
    frame->height = H;
    return frame;
}

static inline FrameParameters frame_parameters(int DW, int DH, int type, int fcc, int planes, int norm) {
    ColorOptions color((FourCC)fcc);
    color.planesPos = (Planes)planes;
    color.normalization = norm != 0;
    ResizeOptions resize(DW, DH);
    resize.type = (ResizeType)type;
    return FrameParameters(resize, color);
}

// the bytes of one DW x DH output: channels * DW * DH elements of one byte, or four with `norm`; with a spec tsvpp_tensor_bytes, and 205 for a
// (parameters, spec) pair the tensor entry points refuse
static inline int output_bytes(int DW, int DH, int type, int fcc, int planes, int norm, const tsvpp_tensor_spec *spec, size_t &bytes) {
    bytes = (size_t)(channelsByFourCC((FourCC)fcc) * (float)DW) * (size_t)DH * (norm ? sizeof(float) : 1);
    if (spec) {
        const tsvpp_params flat{ 0, 0, 0, 0, DW, DH, type, fcc, planes, norm };
        bytes = tsvpp_tensor_bytes(&flat, spec);
        if (bytes == 0) return 205;
    }
    return 0;
}

// One device allocation that holds every output, each at a multiple of 256 bytes.
struct OutputArena {
    uint8_t *base = nullptr;
    std::vector<size_t> bytes;
    std::vector<void *> outs;
    // outputs of the listed sizes (204)
    int carve(const std::vector<size_t> &sizes) {
        bytes = sizes;
        size_t total = 0;
        for (size_t b : bytes) total += (b + 255) & ~(size_t)255;
        if (hipMalloc(&base, total) != hipSuccess) return 204;
        size_t at = 0;
        for (size_t b : bytes) {
            outs.push_back(base + at);
            at += (b + 255) & ~(size_t)255;
        }
        return 0;
    }
    // n outputs of one size
    int carve(size_t n, size_t each) { return carve(std::vector<size_t>(n, each)); }
    void release() { (void)hipFree(base); }
};

// Waits for the consumer (211: the conversion is asynchronous, on the consumer's stream), copies every output back (212) and prints "<index> <crc> <bytes>" and
// what `rest(index, line_end)` appends -- which returns 0 or the program's exit code, before anything of the line is printed.
template <class Rest> static inline int print_outputs(VideoProcessor &vpp, const char *consumer, const OutputArena &arena, uint32_t (*crc)(const uint8_t *, size_t), Rest rest) {
    if (tsvpp_consumer_synchronize(vpp.context(), consumer) != 0) return 211;
    std::vector<uint8_t> result;
    for (size_t i = 0; i < arena.outs.size(); i++) {
        result.resize(arena.bytes[i]);
        if (hipMemcpy(result.data(), arena.outs[i], arena.bytes[i], hipMemcpyDeviceToHost) != hipSuccess) return 212;
        std::string line_end;
        if (int sts = rest(i, line_end)) return sts;
        printf("%zu %u %zu%s\n", i, crc(result.data(), arena.bytes[i]), arena.bytes[i], line_end.c_str());
    }
    return 0;
}
static inline int print_outputs(VideoProcessor &vpp, const char *consumer, const OutputArena &arena, uint32_t (*crc)(const uint8_t *, size_t)) {
    return print_outputs(vpp, consumer, arena, crc, [](size_t, std::string &) { return 0; });
}
