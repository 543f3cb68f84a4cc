// VideoProcessor.h -- the reference's VPP class, re-hosted on the MI355X C ABI (include/tsvpp.h).
//
// Same public surface as reference include/VideoProcessor.h:20-149 (enum values, option structs,
// class methods and argument meaning) for `TensorStream::getFrame` (reference src/Wrappers/WrapperPython.cpp:312,
// src/Wrappers/WrapperC.cpp:291); cudaStream_t becomes hipStream_t.  No gtest and no FFmpeg exist in this image, so the reference's
// VPP tests themselves are not compiled: vpp_goldens.cpp replays their harness (tests/src/VPPTests.cpp:101-132 -- Init, Convert,
// CRC of opaque, DumpFrame, CRC of the file) with all 38 CRC literals of the reference (tests/test_cpp_goldens_gpu.py).
// Everything device-side lives behind tsvpp_*; this file is a thin adapter.
//
// AVFrame: when FFmpeg's <libavutil/frame.h> is on the include path it is used; otherwise (this
// image has no FFmpeg) a stand-in with the few fields Convert() touches keeps the class buildable
// and testable -- data[0], data[1], linesize[0], linesize[1], width, height, opaque.
#pragma once

#include <cstdint>
#include <cstdio>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#if defined(__has_include)
#if __has_include(<libavutil/frame.h>)
extern "C" {
#include <libavutil/frame.h>
}
#define TSVPP_HAVE_LIBAV 1
#endif
#endif
#ifndef TSVPP_HAVE_LIBAV
struct AVFrame { // stand-in, NOT layout compatible with FFmpeg's
    uint8_t *data[8] = {};
    int linesize[8] = {};
    int width = 0, height = 0;
    void *opaque = nullptr;
};
inline AVFrame *av_frame_alloc() { return new AVFrame(); }
inline void av_frame_unref(AVFrame *f) { if (f) *f = AVFrame(); }
inline void av_frame_free(AVFrame **f) { if (f && *f) { delete *f; *f = nullptr; } }
#endif

#include <hip/hip_runtime.h>

#include "tsvpp.h"

// ---- reference include/Common.h:19-24, 29-34, 62-70 -------------------------------------------
enum Internal { VREADER_ERROR = -3, VREADER_UNSUPPORTED = -2, VREADER_REPEAT = -1, VREADER_OK = 0 };
enum LogsLevel { NONE, LOW, MEDIUM, HIGH };
class Logger {
public:
    void initialize(LogsLevel level, std::string logName = "logs.txt") { logsLevel = level; logFileName = logName; }
    std::string logFileName;
    LogsLevel logsLevel = LogsLevel::NONE;
    bool enableNVTX = false; // honoured as roctx ranges when the tracer is linked in
};

// ---- reference include/VideoProcessor.h:20-105 (same enumerator values, same defaults) ---------
enum FourCC { Y800 = 0, RGB24, BGR24, NV12, UYVY, YUV444, HSV };
enum Planes { PLANAR = 0, MERGED };
enum ResizeType { NEAREST = 0, BILINEAR, BICUBIC, AREA };

struct ColorOptions {
    ColorOptions(FourCC fourCC = FourCC::RGB24) : normalization(fourCC == FourCC::HSV), planesPos(Planes::MERGED), dstFourCC(fourCC) {}
    bool normalization;
    Planes planesPos;
    FourCC dstFourCC;
};
struct ResizeOptions {
    ResizeOptions(int w = 0, int h = 0) : width((unsigned)w), height((unsigned)h), type(ResizeType::NEAREST) {}
    unsigned int width, height; // 0 = no resize
    ResizeType type;
};
struct CropOptions {
    CropOptions(std::tuple<int, int> lt = { 0, 0 }, std::tuple<int, int> rb = { 0, 0 }) : leftTopCorner(lt), rightBottomCorner(rb) {}
    std::tuple<int, int> leftTopCorner, rightBottomCorner; // (x, y); empty box = no crop
};
struct FrameParameters {
    FrameParameters(ResizeOptions r = ResizeOptions(), ColorOptions c = ColorOptions(), CropOptions k = CropOptions()) : resize(r), color(c), crop(k) {}
    ResizeOptions resize;
    ColorOptions color;
    CropOptions crop;
};

float channelsByFourCC(FourCC fourCC);
float channelsByFourCC(std::string fourCC);

// ---- the reference's public stage launchers (include/VideoProcessor.h:110-115), source-compatible ----------------------
// The fused kernels have no stages; these thin functions run ONE stage each through the same C ABI (NV12 in, NV12 out for
// crop / resize) with the reference's buffer contract, so code that called the stages directly keeps compiling and the stages
// can be compared one by one (tests/test_cpp_stages_gpu.py).  `maxThreadsPerBlock` is accepted and ignored; the work is
// enqueued on *stream of the calling thread's current device (a process-wide context per device, created on first use).
//   cropHost:      dst->data[0] / data[1] = fresh device buffers (cw * ch, cw * ch / 2) holding the box; dst sizes / linesize untouched
//                  (reference src/Crop.cu:23-48; the caller sets dst->width / height and later hipFree()s both buffers)
//   resizeKernel:  src->width / height / linesize (0 = width) describe the input; dst->data[0] / data[1] = fresh buffers of
//                  resize.width x resize.height; `crop` = the input buffers came from cropHost and are freed here (src/Resize.cu:408-473)
//   colorConversionKernel<T>: input = src planes of dst->width x dst->height (pitch src->linesize[0] or that width);
//                  dst->opaque = fresh buffer of channels * w * h elements of T (src/ColorConversion.cu:280-382); T = float iff
//                  color.normalization (or HSV), as VideoProcessor::Convert calls it
int cropHost(AVFrame *src, AVFrame *dst, CropOptions crop, int maxThreadsPerBlock, hipStream_t *stream);
int resizeKernel(AVFrame *src, AVFrame *dst, bool crop, ResizeOptions resize, int maxThreadsPerBlock, hipStream_t *stream);
template <class T> int colorConversionKernel(AVFrame *src, AVFrame *dst, ColorOptions color, int maxThreadsPerBlock, hipStream_t *stream);

class VideoProcessor {
public:
    // Init(logger, maxConsumers, enableDumps): reference src/VideoProcessor.cpp:79-92.  `device` is an
    // addition (the reference always queries device 0): -1 = the calling thread's current HIP device.
    int Init(std::shared_ptr<Logger> logger, uint8_t maxConsumers = 5, bool enableDumps = false, int device = -1);
    // Convert: reference src/VideoProcessor.cpp:94-166.  Reads input->data[0..1], linesize[0..1], width,
    // height; writes output->opaque (device memory the CALLER frees with hipFree, exactly like the
    // reference's cudaMalloc'ed result), output->width/height; consumes `input` (av_frame_unref).
    // Work is enqueued on the stream owned by `consumerName`; nothing is freed or synchronised here.
    int Convert(AVFrame *input, AVFrame *output, FrameParameters &options, std::string consumerName);
    // Same conversion into caller-owned memory (no allocation at all) -- what a torch-backed
    // getFrame should call with tensor.data_ptr().
    int ConvertInto(AVFrame *input, void *deviceOut, FrameParameters &options, std::string consumerName, int *outWidth = nullptr, int *outHeight = nullptr);
    // The cascade behind a detector (tsvpp_convert_rois, include/tsvpp.h; not in the reference): box rois[i] of inputs[rois[i].frame] -- the frames may differ in size
    // and pitch -- is cut out, resized to options.resize.width x height, colour-converted and written to deviceOuts[i] (caller-owned device memory of
    // channels * width * height elements), one kernel launch per TSVPP_MAX_ROIS boxes on the consumer's stream.  options.crop must be empty; the inputs are NOT
    // consumed (no av_frame_unref: a frame usually serves several calls).  Same status convention as ConvertInto.
    int ConvertRois(AVFrame *const *inputs, int nInputs, const tsvpp_roi *rois, int nRois, void *const *deviceOuts, FrameParameters &options, std::string consumerName);
    // The same for options.resize.type == AREA (tsvpp_convert_rois_area: every box with both ratios above 1 is averaged, any other takes AREA's up-scale rule; no
    // weight table is built or cached).  ConvertRois refuses AREA and this refuses everything else: two entry points until the C ABI folds them.
    int ConvertRoisArea(AVFrame *const *inputs, int nInputs, const tsvpp_roi *rois, int nRois, void *const *deviceOuts, FrameParameters &options, std::string consumerName);
    // The frame in front of a detector (tsvpp_convert_letterbox, include/tsvpp.h; not in the reference): inputs[k] -- the frames may differ in size and pitch -- is
    // resized with its aspect kept into rects[k] (null: the rectangle of tsvpp_letterbox_rect) of a canvas of options.resize.width x height, the rest of the canvas is
    // the colour conversion of the sample (padY, padU, padV), written to deviceOuts[k] (caller-owned device memory of channels * width * height elements), one kernel
    // launch per TSVPP_MAX_LETTERBOX frames on the consumer's stream.  options.crop must be empty; the inputs are NOT consumed.  Same status convention as ConvertInto.
    int ConvertLetterbox(AVFrame *const *inputs, int n, const tsvpp_rect *rects, int padY, int padU, int padV, void *const *deviceOuts, FrameParameters &options,
                         std::string consumerName);
    // What a network takes (tsvpp_convert_rois_tensor / tsvpp_convert_letterbox_tensor, include/tsvpp.h): the same calls with a tensor spec -- element type
    // (TSVPP_F16 / TSVPP_BF16 / TSVPP_F32), mean and scale (= 1 / std) per stored channel; every element is cvt((x / 255 - mean[c]) * scale[c]).  options.color:
    // RGB24 / BGR24 PLANAR or Y800, normalization = true; deviceOuts[k] holds tsvpp_tensor_bytes bytes.  This ConvertRois takes all four resize types, AREA included.
    int ConvertRois(AVFrame *const *inputs, int nInputs, const tsvpp_roi *rois, int nRois, void *const *deviceOuts, FrameParameters &options,
                    const tsvpp_tensor_spec *spec, std::string consumerName);
    int ConvertLetterbox(AVFrame *const *inputs, int n, const tsvpp_rect *rects, int padY, int padU, int padV, void *const *deviceOuts, FrameParameters &options,
                         const tsvpp_tensor_spec *spec, std::string consumerName);
    // ConvertLetterbox for options.resize.type == AREA (tsvpp_convert_letterbox_area, include/tsvpp.h): every frame with both ratios above 1 is averaged with the AREA
    // down-scale, any other takes AREA's up-scale rule; the rectangle holds what ConvertInto returns for the rectangle's size with AREA, bit for bit; no weight
    // table is built or cached, so the first call of a scale is as capturable as any other.  ConvertLetterbox refuses AREA and this refuses everything else.
    // Plain, and with a tensor spec (null: the plain call).
    int ConvertLetterboxArea(AVFrame *const *inputs, int n, const tsvpp_rect *rects, int padY, int padU, int padV, void *const *deviceOuts, FrameParameters &options,
                             std::string consumerName);
    int ConvertLetterboxArea(AVFrame *const *inputs, int n, const tsvpp_rect *rects, int padY, int padU, int padV, void *const *deviceOuts, FrameParameters &options,
                             const tsvpp_tensor_spec *spec, std::string consumerName);
    // Boxes that each go to their OWN output size (tsvpp_convert_rois_sized, include/tsvpp.h; not in the reference): text lines of one height and their own widths,
    // the levels of a pyramid, the inputs of several heads behind one detector pass.  rois[i] carries the box and its dst_width x dst_height; deviceOuts[i] holds
    // tsvpp_rois_sized_bytes bytes.  options.resize.width and height must be 0 (the sizes are the boxes') and options.crop empty; options.resize.type is NEAREST,
    // BILINEAR or BICUBIC (AREA is refused).  One kernel launch per TSVPP_MAX_ROIS_SIZED boxes of a store class on the consumer's stream; the inputs are NOT
    // consumed.  Same status convention as ConvertInto.  With a tensor spec: tsvpp_convert_rois_sized_tensor.
    int ConvertRoisSized(AVFrame *const *inputs, int nInputs, const tsvpp_roi_sized *rois, int nRois, void *const *deviceOuts, FrameParameters &options,
                         std::string consumerName);
    int ConvertRoisSized(AVFrame *const *inputs, int nInputs, const tsvpp_roi_sized *rois, int nRois, void *const *deviceOuts, FrameParameters &options,
                         const tsvpp_tensor_spec *spec, std::string consumerName);
    // Rotated and affine-warped boxes (tsvpp_convert_warp, include/tsvpp.h; not in the reference): warps[i] samples inputs[warps[i].frame] BILINEAR through its
    // output -> source matrix into options.resize.width x height, colour-converted and written to deviceOuts[i], one kernel launch per TSVPP_MAX_WARPS outputs on the
    // consumer's stream.  borderY = borderU = borderV = -1 replicates the frame's edge; else each is 0..255, the sample outside the frame.  options.resize.type must
    // be BILINEAR, options.crop empty; the inputs are NOT consumed.  Same status convention as ConvertInto.  With a tensor spec: tsvpp_convert_warp_tensor.
    int ConvertWarp(AVFrame *const *inputs, int nInputs, const tsvpp_warp *warps, int nWarps, int borderY, int borderU, int borderV, void *const *deviceOuts,
                    FrameParameters &options, std::string consumerName);
    int ConvertWarp(AVFrame *const *inputs, int nInputs, const tsvpp_warp *warps, int nWarps, int borderY, int borderU, int borderV, void *const *deviceOuts,
                    FrameParameters &options, const tsvpp_tensor_spec *spec, std::string consumerName);
    // Homography-warped outputs (tsvpp_convert_perspective, include/tsvpp.h; not in the reference): ConvertWarp with a 3 x 3 output -> source homography per
    // output (tsvpp_persp_from_quad makes one from a quadrilateral).  A homography whose horizon crosses the output is refused.  With a tensor spec:
    // tsvpp_convert_perspective_tensor.
    int ConvertPerspective(AVFrame *const *inputs, int nInputs, const tsvpp_persp *persps, int nPersps, int borderY, int borderU, int borderV, void *const *deviceOuts,
                           FrameParameters &options, std::string consumerName);
    int ConvertPerspective(AVFrame *const *inputs, int nInputs, const tsvpp_persp *persps, int nPersps, int borderY, int borderU, int borderV, void *const *deviceOuts,
                           FrameParameters &options, const tsvpp_tensor_spec *spec, std::string consumerName);
    // ConvertWarp and ConvertPerspective sampled with the library's BICUBIC (tsvpp_convert_warp_bicubic, tsvpp_convert_perspective_bicubic, include/tsvpp.h; not in
    // the reference): the coordinate is the BILINEAR method's bit for bit, the 4 x 4 taps follow the reference's edge rule, the sums are Convert(BICUBIC)'s.
    // options.resize.type must be BICUBIC (ConvertWarp / ConvertPerspective refuse it, and these refuse everything else); every other argument and the status
    // convention are the BILINEAR method's.  Plain, and with a tensor spec (null: the plain call).
    int ConvertWarpBicubic(AVFrame *const *inputs, int nInputs, const tsvpp_warp *warps, int nWarps, int borderY, int borderU, int borderV, void *const *deviceOuts,
                           FrameParameters &options, std::string consumerName);
    int ConvertWarpBicubic(AVFrame *const *inputs, int nInputs, const tsvpp_warp *warps, int nWarps, int borderY, int borderU, int borderV, void *const *deviceOuts,
                           FrameParameters &options, const tsvpp_tensor_spec *spec, std::string consumerName);
    int ConvertPerspectiveBicubic(AVFrame *const *inputs, int nInputs, const tsvpp_persp *persps, int nPersps, int borderY, int borderU, int borderV,
                                  void *const *deviceOuts, FrameParameters &options, std::string consumerName);
    int ConvertPerspectiveBicubic(AVFrame *const *inputs, int nInputs, const tsvpp_persp *persps, int nPersps, int borderY, int borderU, int borderV,
                                  void *const *deviceOuts, FrameParameters &options, const tsvpp_tensor_spec *spec, std::string consumerName);
    // Per-pixel coordinate maps -- lens undistortion, rectification, unwraps (tsvpp_convert_remap, include/tsvpp.h; not in the reference): output k samples frame
    // remaps[k].frame BILINEAR where the device-resident map remaps[k].map says, into options' width x height, colour-converted and stored to deviceOuts[k];
    // on the consumer's stream, status convention as ConvertWarp.  options.crop must be empty.  With a tensor spec: tsvpp_convert_remap_tensor.
    int ConvertRemap(AVFrame *const *inputs, int nInputs, const tsvpp_map *maps, int nMaps, const tsvpp_remap *remaps, int nRemaps, int borderY, int borderU, int borderV,
                     void *const *deviceOuts, FrameParameters &options, std::string consumerName);
    int ConvertRemap(AVFrame *const *inputs, int nInputs, const tsvpp_map *maps, int nMaps, const tsvpp_remap *remaps, int nRemaps, int borderY, int borderU, int borderV,
                     void *const *deviceOuts, FrameParameters &options, const tsvpp_tensor_spec *spec, std::string consumerName);
    // Sparse control-grid warps -- a warp mesh per lens or per stabilised frame (tsvpp_convert_mesh, include/tsvpp.h; not in the reference): ConvertRemap with the
    // coordinate interpolated from the device-resident control grid remaps[k].map (an index into `meshes`) instead of read per pixel; bit for bit ConvertRemap of
    // the expanded mesh (tsvpp_mesh_expand).  Everything else as ConvertRemap.  With a tensor spec: tsvpp_convert_mesh_tensor.
    int ConvertMesh(AVFrame *const *inputs, int nInputs, const tsvpp_mesh *meshes, int nMeshes, const tsvpp_remap *remaps, int nRemaps, int borderY, int borderU, int borderV,
                    void *const *deviceOuts, FrameParameters &options, std::string consumerName);
    int ConvertMesh(AVFrame *const *inputs, int nInputs, const tsvpp_mesh *meshes, int nMeshes, const tsvpp_remap *remaps, int nRemaps, int borderY, int borderU, int borderV,
                    void *const *deviceOuts, FrameParameters &options, const tsvpp_tensor_spec *spec, std::string consumerName);
    // Hands a result of Convert (output->opaque) BACK to the processor instead of hipFree()ing it (round 6).  hipFree stays legal -- it is the reference's
    // contract (c_examples/src/Sample.cpp:27,36) -- but it costs a device-wide synchronisation and the next Convert a hipMalloc: 120-180 us a frame with millisecond
    // outliers, where the conversion itself takes ~6.  A released buffer is reused by the next Convert that needs the same number of bytes: no allocator call in
    // the steady state.  `stream`: the stream on which the caller's LAST use of the buffer was enqueued (nullptr = the legacy default stream); the reuse is ordered
    // behind an event recorded there, nothing is synchronised.  Buffers still pooled at Close() are freed.  VREADER_ERROR for a pointer Convert did not hand out (or one released twice).
    // The processor remembers every result it handed out until it is released, its address is handed out again, or Close(): a result is never forgotten while its
    // caller may still Release() it, however many Converts lie in between.  A caller that hipFree()s its results costs one remembered entry per distinct address.
    // Convert and Release may be called from several threads on one object (the pool has its own lock); Init and Close may not run beside them.
    int Release(void *opaque, hipStream_t stream = nullptr);
    template <class T> int DumpFrame(T *output, FrameParameters options, std::shared_ptr<FILE> dumpFile);
    void Close();
    ~VideoProcessor() { Close(); }
    tsvpp_ctx *context() const { return ctx; }

private:
    bool enableDumps = false;
    tsvpp_ctx *ctx = nullptr;
    std::mutex dumpSync;
    // result buffers: what Convert handed out (pointer -> bytes) and what Release took back (bytes -> buffers, each with the event of its release)
    struct Pooled { void *ptr; hipEvent_t released; };
    std::mutex poolSync;
    std::unordered_map<void *, size_t> handedOut;
    std::unordered_map<size_t, std::vector<Pooled>> pool;
    std::vector<hipEvent_t> spareEvents;
    bool isClosed = true;
    std::shared_ptr<Logger> logger;
};
