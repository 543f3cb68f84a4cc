/*
 * tsvpp.h -- C ABI of the MI355X-native Video Post Processing (VPP) path.
 *
 * Drop-in boundary for the hot path of osai-ai/tensor-stream:
 *     NV12 crop -> nearest/bilinear/bicubic/area resize -> YUV->RGB24/BGR24
 *     (+ fp32 normalise, planar/merged)
 * i.e. everything that sits behind `VideoProcessor::Convert()`
 * (reference src/VideoProcessor.cpp:94-166) and its three CUDA launchers
 * `cropHost` (src/Crop.cu:23-48), `resizeKernel` (src/Resize.cu:408-473) and
 * `colorConversionKernel<T>` (src/ColorConversion.cu:280-382).
 *
 * The reference has no C ABI (its boundary is the C++ class); these entry points
 * are what a `VideoProcessor` built for ROCm binds instead of the CUDA launchers.
 * INTEGRATION.md shows the adapter; tensor-stream_amd/cpp/VideoProcessor.{h,cpp}
 * is that adapter, written out.
 *
 * Conventions
 *   - plain C types only: device pointers are `void*` / `const uint8_t*`, the HIP
 *     stream is passed as `void*` (a `hipStream_t`; NULL = the null stream);
 *   - every function returning `int` uses the reference's status convention
 *     (include/Common.h:19-24): 0 = OK, negative = VREADER_* code, positive = a
 *     `hipError_t` value (the reference returns `cudaError_t` the same way);
 *   - all work is enqueued on the given stream and is asynchronous; nothing in the
 *     per-frame path frees or synchronises, and nothing allocates once the request
 *     has been seen by tsvpp_prepare_batch (the reference does 1-5 cudaMalloc + 0-4
 *     cudaFree per frame, src/VideoProcessor.cpp:94-166).  Without a prepare call the
 *     FIRST conversion of a new AREA scale builds its weight table, and the first
 *     UYVY / YUV444 conversion behind a resize on a stream sizes that stream's NV12
 *     scratch buffer (one hipMalloc each; an outgrown buffer is kept until
 *     tsvpp_destroy, never freed under running work);
 *   - every entry point leaves the calling thread's current HIP device as it found it;
 *   - output memory is CALLER-allocated and tight: channels*W*H elements of
 *     uint8 (normalization == 0) or float (normalization != 0), layout as the
 *     reference's kernels write it (src/ColorConversion.cu:41-93).
 */
#ifndef TSVPP_H
#define TSVPP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes: reference include/Common.h:19-24 (enum Internal) ---- */
#define TSVPP_OK 0
#define TSVPP_REPEAT (-1)
#define TSVPP_UNSUPPORTED (-2)
#define TSVPP_ERROR (-3)

/* ---- enums: byte-compatible with reference include/VideoProcessor.h:20-28,32-35,57-62 ---- */
enum tsvpp_fourcc { TSVPP_Y800 = 0, TSVPP_RGB24 = 1, TSVPP_BGR24 = 2, TSVPP_NV12 = 3, TSVPP_UYVY = 4, TSVPP_YUV444 = 5, TSVPP_HSV = 6 };
enum tsvpp_planes { TSVPP_PLANAR = 0, TSVPP_MERGED = 1 };
enum tsvpp_resize { TSVPP_NEAREST = 0, TSVPP_BILINEAR = 1, TSVPP_BICUBIC = 2, TSVPP_AREA = 3 };

#define TSVPP_MAX_BATCH 128 /* frames per launch; larger batches are split (round 4: 64 -> 128; the pointer table travels in the kernarg segment: 3 KiB) */

/* One NV12 frame in device memory.  Mirrors the AVFrame fields Convert() reads
 * (reference src/Crop.cu:37-38, src/Resize.cu:420-421, src/ColorConversion.cu:301):
 * data[0], data[1], linesize[0], linesize[1], width, height.
 * pitch == 0 means "pitch = width", exactly as the reference's fallback. */
typedef struct tsvpp_nv12 {
    const uint8_t *y;  /* AVFrame::data[0] */
    const uint8_t *uv; /* AVFrame::data[1], interleaved U,V */
    int32_t pitch_y;   /* AVFrame::linesize[0] */
    int32_t pitch_uv;  /* AVFrame::linesize[1] */
    int32_t width;
    int32_t height;
} tsvpp_nv12;

/* The source limit.  Inside one plane the kernels address with unsigned 32-bit byte offsets, counted from the address they are handed -- and the kernels
 * that fetch 16-byte chunks count from the 16-byte boundary at or below it, up to 15 bytes earlier.  The SPAN of a plane, as seen from that address,
 *     span = (rows - 1) * pitch + row_bytes
 * must therefore stay below TSVPP_SOURCE_SPAN_LIMIT = 2^32 - 16, for the luma plane (rows, row_bytes = height, width of the region) and for the chroma
 * plane (height / 2, width) each, with each plane's own pitch.  The region, and the address it is seen from, is
 *   tsvpp_convert / _batch / _table, tsvpp_describe      the crop box where Convert's crop stage applies (the planes advanced to its origin), else the frame;
 *   tsvpp_convert_rois / _rois_area / _rois_tensor       each box (the planes advanced to the box's origin): a small box in a huge frame is legal;
 *   letterbox, warp, perspective, remap, mesh            the whole frame.
 * A request with a span at or above the limit is TSVPP_UNSUPPORTED, from the describe call and the convert call alike, before anything is launched.  It comes
 * after the TSVPP_ERROR rules on the request itself (sizes, crop, boxes, pitches), which the describe calls share; the convert calls look at their pointers
 * only afterwards, so a null plane or output pointer together with an over-limit span answers TSVPP_UNSUPPORTED, not TSVPP_ERROR.  Spans of 2^31 and more are
 * ordinary requests.  A pitch travels in 32 bits (below 2^31); a coordinate map or control grid is addressed
 * with 64-bit offsets and has no such limit; an output stays below 2^32 bytes (each call's own rule). */
#define TSVPP_SOURCE_SPAN_LIMIT 0xFFFFFFF0ull

/* Flat mirror of FrameParameters {ResizeOptions, ColorOptions, CropOptions}
 * (reference include/VideoProcessor.h:39-105).  Zero-initialised == the
 * reference defaults except fourcc/planes (reference: RGB24, MERGED). */
typedef struct tsvpp_params {
    int32_t crop_left, crop_top;     /* CropOptions::leftTopCorner  (x, y) */
    int32_t crop_right, crop_bottom; /* CropOptions::rightBottomCorner (x, y) */
    int32_t dst_width, dst_height;   /* ResizeOptions::width/height, 0 = no resize */
    int32_t resize_type;             /* enum tsvpp_resize */
    int32_t fourcc;                  /* enum tsvpp_fourcc */
    int32_t planes;                  /* enum tsvpp_planes */
    int32_t normalization;           /* ColorOptions::normalization */
} tsvpp_params;

/* The eight colour constants of reference src/ColorConversion.cu:23,25,30,35:
 * {1.163999557, 1.5959997177, 2.017999649, -0.812999725, -0.390999794, 0.5, 16, 128}.
 * They are literals in the reference; here they live in the context so that a
 * multi-GPU job can broadcast one block from rank 0 (RCCL) and every rank can
 * verify it against the compiled-in defaults. */
typedef struct tsvpp_coeffs {
    float y_scale, v_to_r, u_to_b, v_to_g, u_to_g, round_bias, y_offset, c_offset;
} tsvpp_coeffs;

typedef struct tsvpp_ctx tsvpp_ctx;

/* VideoProcessor::Init (reference src/VideoProcessor.cpp:79-92): selects `device`,
 * creates `max_consumers` streams for the named-consumer pool.  Unlike the
 * reference it queries the properties of `device`, not of device 0. */
int tsvpp_create(int device, int max_consumers, tsvpp_ctx **out_ctx);
/* VideoProcessor::Close (src/VideoProcessor.cpp:168-178) + release of cached tables. */
void tsvpp_destroy(tsvpp_ctx *ctx);

/* findFree<cudaStream_t>(consumerName, streamArr) (reference include/Common.h:225-237,
 * src/VideoProcessor.cpp:98-104): the stream bound to `name`, claiming a free slot
 * for a new name; TSVPP_ERROR when all `max_consumers` slots are taken. */
int tsvpp_consumer_stream(tsvpp_ctx *ctx, const char *name, void **out_stream);
/* The stream the consumer's NEXT conversion should be enqueued on (round 6; VideoProcessor::Convert / ConvertInto use it).  By default that is
 * tsvpp_consumer_stream's: one stream per consumer, every conversion ordered behind the previous one -- the reference's model.  Under
 * TSVPP_OPT_INPUTS_READY (below) a consumer owns TWO streams and this call alternates between them: conversion k + 1 is launched while conversion k still
 * drains (a single 1080p -> 720p frame is ~2.3 us of HBM time behind a ~1.5-1.9 us dependent-launch boundary; measured: one consumer, one frame per launch,
 * 0.27 -> 0.41 of the HBM roofline, two frames per launch 0.44 -> 0.58, four 0.47 -> 0.68, eight 0.60 -> 0.72; profiles/r06_curve_values.txt).  `launch_bytes` = the bytes the conversion about to be
 * enqueued moves (source + output bytes of all its frames; 0 = unknown, taken as one frame): only launches of at most TSVPP_OVERLAP_MAX_BYTES alternate -- two
 * LARGE launches side by side lose (64-frame launches of the headline: 0.78 -> 0.67 of the roofline), so those stay on the consumer's first stream.  The second
 * stream is created on the consumer's first call with the option set (one hipStreamCreate).  tsvpp_consumer_synchronize waits (on the host) for everything
 * enqueued on the consumer's streams. */
#define TSVPP_OVERLAP_MAX_BYTES ((size_t)256 << 20)
#define TSVPP_BARRIER_FREE_MAX_BYTES ((size_t)64 << 20) /* ... and only launches up to this size go out without the barrier bit (profiles/r06_curve_values.txt) */
int tsvpp_consumer_next_stream(tsvpp_ctx *ctx, const char *name, size_t launch_bytes, void **out_stream);
int tsvpp_consumer_synchronize(tsvpp_ctx *ctx, const char *name);

/* Stage selection of Convert() (reference src/VideoProcessor.cpp:106-135) without
 * running anything: final width/height and the tight output size in bytes. */
int tsvpp_out_dims(const tsvpp_params *p, int in_width, int in_height, int *out_width, int *out_height);
size_t tsvpp_out_bytes(const tsvpp_params *p, int in_width, int in_height);
/* channelsByFourCC (reference src/VideoProcessor.cpp:4-14). */
float tsvpp_channels(int fourcc);

/* VideoProcessor::Convert for one frame, as ONE fused kernel launch on `stream`.
 * `out` must hold tsvpp_out_bytes() bytes. */
int tsvpp_convert(tsvpp_ctx *ctx, const tsvpp_nv12 *in, const tsvpp_params *p, void *out, void *stream);

/* The same conversion for `n` independent frames of identical geometry, in
 * ceil(n / TSVPP_MAX_BATCH) launches.  `in` and `outs` are HOST arrays of n entries.
 * (Not in the reference: one 1080p frame is ~2.5 us of HBM time, below a launch.) */
int tsvpp_convert_batch(tsvpp_ctx *ctx, int n, const tsvpp_nv12 *in, const tsvpp_params *p, void *const *outs, void *stream);

/* ---- persistent frame tables (round 5; not in the reference) ------------------------------------------------------------------------------------------
 * tsvpp_convert_batch passes its (y, uv, out) pointer triples by value in the kernarg segment: no copy, no device-side descriptor -- and at most
 * TSVPP_MAX_BATCH frames per launch.  A pipeline whose decoder surfaces and output buffers are POOLS (the usual case: the same surfaces and tensors come
 * round again) can instead register them once in a device-resident table and convert any run of its entries with launches of up to
 * TSVPP_MAX_TABLE_LAUNCH frames: the small-output configurations (BASELINE C3: 1.8 MB per frame) move 0.64 of the HBM roofline in 64-frame launches and
 * 0.70+ from 256 frames on (profiles/r05_table_ab.txt); nothing is copied per call.
 *   tsvpp_table_create    `capacity` entries; every entry shares one geometry (width, height, pitches: fixed by the first tsvpp_table_set).
 *   tsvpp_table_set       entries [first, first + n) <- in[i] / outs[i] (HOST arrays); uploaded on `stream` out of pinned staging the table owns (one slot per
 *                         upload in flight, four slots: a fifth concurrent upload waits for the oldest): the arrays may be freed on return, conversions enqueued
 *                         on the same stream afterwards see the new entries, conversions enqueued BEFORE it see the old ones.
 *   tsvpp_convert_table   == tsvpp_convert_batch over entries [first, first + n), same results, same status codes.
 *   tsvpp_table_destroy   frees the table (the caller has waited for conversions that use it).  Destroying the CONTEXT first is legal: tsvpp_destroy releases the
 *                         device memory of its live tables, their handles remain valid arguments of tsvpp_table_destroy only.
 * tsvpp_table_set on a stream that is being captured into a hipGraph is refused: TSVPP_UNSUPPORTED, nothing is enqueued and the table is unchanged (its copies
 * would become graph nodes that re-read recycled staging memory at every replay).  Set the entries on an ordinary stream before or after the capture; the captured
 * tsvpp_convert_table reads whatever the table holds at replay time.  (A NULL stream is taken as not capturing.)
 * A table belongs to the context that created it (its device).  tsvpp_table_set calls are serialised against each other; a tsvpp_convert_table that runs
 * concurrently with a tsvpp_table_set of the SAME entries from another thread is the caller's race (as two writers of one AVFrame would be), and a captured
 * hipGraph replays the table as the device holds it at replay time (entries are read by the kernels, not baked into the graph). */
#define TSVPP_MAX_TABLE_LAUNCH 1024
typedef struct tsvpp_table tsvpp_table;
int tsvpp_table_create(tsvpp_ctx *ctx, int capacity, tsvpp_table **out_table);
void tsvpp_table_destroy(tsvpp_table *table);
int tsvpp_table_set(tsvpp_table *table, int first, int n, const tsvpp_nv12 *in, void *const *outs, void *stream);
int tsvpp_convert_table(tsvpp_ctx *ctx, const tsvpp_table *table, int first, int n, const tsvpp_params *p, void *stream);

/* ---- regions of interest (not in the reference: one crop box per Convert, src/VideoProcessor.cpp:106-135) ------------------------------------------------
 * The cascade behind a detector: `n_rois` boxes, taken from one or several NV12 frames, each resized to the SAME p->dst_width x p->dst_height, colour-converted
 * and stored to its own output, in ceil(n_rois / TSVPP_MAX_ROIS) kernel launches (one tsvpp_convert with crop_* per box is one launch per box: ~4 us of host
 * time and a dependent-launch boundary for well under 1 us of HBM time).
 *   rois[i]     box [left, right) x [top, bottom) of frames[rois[i].frame], in luma pixels; even width and height; inside its frame.  Boxes may overlap,
 *               touch the frame's edges or span its full width / height (such a box IS cut out here, unlike Convert's crop stage, which ignores a crop that
 *               is not smaller than the frame in both dimensions), and may be smaller than the output (up-scaling) on either axis.
 *   frames      may differ in size and pitch (a detector batch over several streams).
 *   outs[i]     device memory of box i, tight: channels * dst_width * dst_height elements (channels = tsvpp_channels(p->fourcc): 3 for RGB24 / BGR24, 1 for
 *               Y800) of uint8 (p->normalization == 0) or float, i.e. tsvpp_out_bytes(p, dst_width, dst_height) bytes, laid out as tsvpp_convert's output.
 *   p           dst_width / dst_height (> 0, even), resize_type, fourcc, planes, normalization; p->crop_* must be zero (the boxes are the crops).
 * The result of a box is, bit for bit, what tsvpp_convert returns for a frame that consists of the box alone (luma rows [top, bottom) x columns [left, right);
 * chroma rows [top / 2, top / 2 + height / 2) x BYTE columns [left, right): the crop rule of Convert, an odd `left` swaps U and V as it does there), resized
 * with xr = (float)width / dst_width, yr = (float)height / dst_height; for a box Convert's crop stage accepts it equals tsvpp_convert(crop = box).  A box of
 * exactly dst_width x dst_height is a plain colour conversion (every interpolation weight is zero).
 * Supported: NEAREST, BILINEAR, BICUBIC; RGB24 / BGR24 planar and merged, Y800; uint8 and fp32.  TSVPP_UNSUPPORTED here: AREA (it has an entry point
 * of its own, tsvpp_convert_rois_area below), NV12 / UYVY / YUV444 / HSV outputs.  Neither are boxes out of a tsvpp_table; per-box output sizes are tsvpp_convert_rois_sized's (below); rotated and affine-warped boxes are tsvpp_convert_warp's (below).
 * fp16 / bf16 outputs and a per-channel mean / scale are tsvpp_convert_rois_tensor's (below), not this call's.
 * `frames`, `rois`, `outs` are HOST arrays and may be freed on return: the per-box records (plane origins, pitches, size, ratios, output pointer: 48 bytes)
 * travel BY VALUE in the kernarg segment of their launch -- no staging buffer, no copy, no allocation, no host synchronisation -- which is what bounds a
 * launch to TSVPP_MAX_ROIS boxes.  The call is therefore legal while `stream` is being captured into a hipGraph: the graph replays the records (the pointers
 * and boxes of the captured call) as they were.  Always an ordinary in-order launch (TSVPP_OPT_INPUTS_READY does not apply); TSVPP_OPT_COLOR_G_TERM and the
 * context's coefficient block are honoured; the replay cache is not involved.
 * Status, decided before any device is touched (tsvpp_describe_rois returns the same one):
 *   TSVPP_ERROR        null arguments, n_rois <= 0, n_frames <= 0, a frame without size or with a pitch below its width, `frame` out of range, a box that is
 *                      empty, inverted or not inside its frame, dst_width / dst_height <= 0, non-zero crop_* in `p` (and, converting: a null plane or output)
 *   TSVPP_UNSUPPORTED  odd box width / height, odd dst_*, odd frame size, AREA, an unknown resize type, an output format outside the list above. */
#define TSVPP_MAX_ROIS 64 /* boxes per launch; more are split */
typedef struct tsvpp_roi {
    int32_t frame;                    /* index into `frames` */
    int32_t left, top, right, bottom; /* as CropOptions: leftTopCorner (x, y), rightBottomCorner (x, y) */
} tsvpp_roi;
int tsvpp_convert_rois(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois, const tsvpp_params *p, void *const *outs,
                       void *stream);
/* What tsvpp_convert_rois WOULD launch, as one line of key=value text in tsvpp_describe's style: "mode=bilinear out=f32_planar dst=224x224 rois=33 frames=1
 * launches=1 kernel=vpp_rois<...> shape=8x16 lds=.. grid=.. tiles=7x7 staged=.. tail=.. nt=.. limit=64".  Host only: needs no context and no GPU, the plane
 * pointers in `frames` are not read (taken as 256-byte aligned); TSVPP_* knobs are honoured.  lds= / grid= are the first launch's; staged= is the number of
 * boxes whose every tile stages its source footprint in LDS (the LDS budget, TSVPP_LDS_KB, decides; the others gather from global memory); tail= as in
 * tsvpp_describe (2: shifted last tile column; 0). */
int tsvpp_describe_rois(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois, int aligned_outputs, char *buf,
                        size_t buf_len);

/* ---- regions of interest, AREA ---------------------------------------------------------------------------------------------------------------------------
 * tsvpp_convert_rois with p->resize_type == TSVPP_AREA -- the filter a cascade wants when it shrinks a 300-500 pixel box to 112 x 112 or 224 x 224: the only one
 * of the four that averages every source pixel.  Arguments, box rules, output layout, launch splitting (TSVPP_MAX_ROIS_AREA boxes per launch), the order of the
 * statuses and "decided before any device is touched" are tsvpp_convert_rois's, word for word; so is the contract: the result of a box is, bit for bit, what
 * tsvpp_convert returns for a frame that consists of the box alone, resized with TSVPP_AREA, and for a box Convert's crop stage accepts it equals
 * tsvpp_convert(crop = box, AREA).  The differences:
 *   resize type   p->resize_type must be TSVPP_AREA; anything else is TSVPP_UNSUPPORTED (and tsvpp_convert_rois keeps answering TSVPP_UNSUPPORTED for AREA).
 *   per box       as Convert decides per request (reference src/Resize.cu:435): a box with xr > 1 AND yr > 1 runs the AREA down-scale (the weighted box); any
 *                 other box -- up-scaled on either axis, or exactly the output size -- runs the AREA up-scale rule (the 2 x 2 blend).  One launch may mix both.
 *   no tables     tsvpp_convert builds a device weight table per distinct scale (one allocation and one synchronous copy per axis the first time a scale is seen,
 *                 kept until tsvpp_destroy); boxes behind a detector have a new scale each.  Here the kernel generates the weight rows a tile reads inside the
 *                 tile (csrc/vpp_rois_area.hip): no allocation, no copy, no host synchronisation, nothing cached in the context, records by value in the kernarg
 *                 segment -- legal while `stream` is being captured, like tsvpp_convert_rois.
 *   limits        TSVPP_UNSUPPORTED for a down-scale box that needs more than 40 taps on an axis (taps = ceil(ratio): 1920 columns to 112 need 18, 1080 rows
 *                 to 30 need 36), and for dst_width or dst_height above 65536.
 *   cost          a tile of a down-scale box first waits for one lane to generate the weight rows of every output column / row in front of it (~75 ns each,
 *                 once per tile: ~17 us for the last tile column of a 224-wide output), so a launch with a down-scale box takes 25-50 us where the BILINEAR
 *                 launch takes 5-16 (profiles/rois_area_ab.txt).  Linear in the output size: meant for NN-input sizes, not for outputs thousands of pixels wide.
 *   deviation     tsvpp_convert refuses (TSVPP_UNSUPPORTED) a ratio whose weight pattern does not close within 65536 rows.  This call never needs more than
 *                 dst_width / dst_height rows and answers such a box with the generator's rows (the rows tsvpp_convert's table would begin with).
 * Why a second entry point instead of one more resize type of tsvpp_convert_rois: that call's answer to AREA (TSVPP_UNSUPPORTED, from tsvpp_describe_rois,
 * tsvpp_convert_rois and the Python / C++ facades alike) is pinned by its tests.  tsvpp_convert_rois_tensor (below) is the folded form: it takes all four resize types.
 * tsvpp_describe_rois_area prints tsvpp_describe_rois's keys (mode=area, kernel=vpp_rois_area<...>, limit=64; lds= includes the weight rows) and then
 * "down=<boxes on the down-scale path> taps=<largest taps_x>x<largest taps_y>" (0x0 without a down-scale box). */
#define TSVPP_MAX_ROIS_AREA 64 /* boxes per launch; more are split (the per-box record is tsvpp_convert_rois's: nothing had to grow) */
int tsvpp_convert_rois_area(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois, const tsvpp_params *p, void *const *outs,
                            void *stream);
int tsvpp_describe_rois_area(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois, int aligned_outputs, char *buf,
                             size_t buf_len);
/* DEBUG ONLY (tests), host only: the weight rows tsvpp_convert_rois_area's kernel generates for output indices first .. first + n - 1 of an axis with ratio
 * `scale` (> 1) -- the same generator, evaluated on the host -- as n rows of *taps = ceil(scale) floats in `out` (max_floats entries).  Row j equals row
 * j % rows of tsvpp_area_pattern(scale).  Returns n; TSVPP_UNSUPPORTED for scale <= 1, more than 40 taps or first + n > 65536; TSVPP_ERROR for null / negative
 * arguments or a buffer that is too small. */
int tsvpp_roi_area_rows(float scale, int first, int n, float *out, int max_floats, int *taps);

/* ---- letterbox (not in the reference: Convert stretches the frame to dst_width x dst_height) ----------------------------------------------------------------
 * The frame in front of a detector: `n` NV12 frames, each resized WITH ITS ASPECT KEPT into an inner rectangle of one canvas of p->dst_width x p->dst_height, the
 * rest of the canvas filled with a constant, in ceil(n / TSVPP_MAX_LETTERBOX) kernel launches (a Convert to the inner size into a temporary, a fill of the canvas
 * and a strided copy are three launches and an extra write and read of the output).
 *   in[k]       may differ in size and pitch from frame to frame, as in tsvpp_convert_rois.
 *   outs[k]     device memory of canvas k, tight: channels * dst_width * dst_height elements of uint8 (p->normalization == 0) or float, laid out as
 *               tsvpp_convert's output for a dst_width x dst_height frame.
 *   rects       NULL: every frame gets the rectangle of tsvpp_letterbox_rect (below).  Else n rectangles, one per frame: left, top, width, height all even,
 *               width and height > 0, inside the canvas.  The rectangle need not keep the aspect and may be larger than the frame (up-scaling).
 *   pad_y/u/v   the pad, as one NV12 sample, each 0..255: (114, 128, 128) is gray 114 and (16, 128, 128) is black under the default coefficients.
 *   p           dst_width / dst_height (the canvas: > 0, even), resize_type, fourcc, planes, normalization; p->crop_* must be zero.
 * For frame k the canvas is, bit for bit:
 *   inner rectangle   origin (left, top), size (width, height): what tsvpp_convert returns for that frame with dst = (width, height) and the same resize type,
 *                     fourcc, planes and normalization -- the contract of tsvpp_convert_rois with the whole frame as the box, xr = (float)in_w / width,
 *                     yr = (float)in_h / height.  A frame of exactly the inner size is the plain colour conversion.
 *   pad               every pixel outside it: what the colour back end makes of the constant sample (pad_y, pad_u, pad_v), i.e. the value tsvpp_convert without a
 *                     resize returns for a frame of that constant.  The pad is given in YUV because it then runs through the one colour back end the library has,
 *                     in every flavour (uint8 and fp32, planar and merged, swapped channels, Y800 -- which keeps pad_y alone --, the TSVPP_OPT_COLOR_G_TERM
 *                     variants), and needs no store code of its own.
 * Supported: NEAREST, BILINEAR, BICUBIC; RGB24 / BGR24 planar and merged, Y800; uint8 and fp32.  Not: AREA (its down-scale needs weight rows: a call of its own,
 * tsvpp_convert_letterbox_area below, generates them), NV12 / UYVY / YUV444 / HSV outputs, crops, frames out of a tsvpp_table, an RGB pad colour.
 * `in`, `rects`, `outs` are HOST arrays and may be freed on return: the per-frame records (planes, pitches, size, ratios, rectangle, canvas pointer: 64 bytes)
 * travel BY VALUE in the kernarg segment of their launch -- no allocation, no copy, no host synchronisation, nothing cached in the context, no replay cache --
 * which is what bounds a launch to TSVPP_MAX_LETTERBOX frames.  The call is therefore legal while `stream` is being captured into a hipGraph.  Always an ordinary
 * in-order launch (TSVPP_OPT_INPUTS_READY does not apply); TSVPP_OPT_COLOR_G_TERM and the context's coefficient block are honoured.
 * Status, decided before any device is touched (tsvpp_describe_letterbox returns the same one), in this order:
 *   TSVPP_ERROR        null arguments, n <= 0, a frame without size or with a pitch below its width, dst_width / dst_height <= 0, non-zero crop_* in `p`, a
 *                      rectangle that is empty or not inside the canvas, a pad component outside 0..255 (and, converting: a null context, plane or output)
 *   TSVPP_UNSUPPORTED  odd dst_*, an odd frame size, an odd rectangle field, AREA or an unknown resize type, an unknown `planes` value, an output format outside
 *                      the list above, an output of 4 GiB or more. */
#define TSVPP_MAX_LETTERBOX 32 /* frames per launch; more are split */
typedef struct tsvpp_rect {
    int32_t left, top, width, height;
} tsvpp_rect;
/* The default inner rectangle of an in_w x in_h frame in a dst_w x dst_h canvas: the largest even-sized rectangle of the frame's aspect (to the nearest even
 * number), centred on an even origin.  64-bit integers only, so host, tests and callers agree:
 *   in_w * dst_h >= in_h * dst_w:  width = dst_w,  height = 2 * ((in_h * dst_w + in_w) / (2 * in_w)) clamped to [2, dst_h]
 *   otherwise:                     height = dst_h, width  = 2 * ((in_w * dst_h + in_h) / (2 * in_h)) clamped to [2, dst_w]
 *   left = ((dst_w - width) / 2) & ~1, top = ((dst_h - height) / 2) & ~1.
 * 1920 x 1080 into 640 x 640 gives 640 x 360 at (0, 140).  TSVPP_ERROR for a null `out` or a size <= 0, TSVPP_UNSUPPORTED for an odd dst_w / dst_h. */
int tsvpp_letterbox_rect(int in_w, int in_h, int dst_w, int dst_h, tsvpp_rect *out);
int tsvpp_convert_letterbox(tsvpp_ctx *ctx, int n, const tsvpp_nv12 *in, const tsvpp_params *p, const tsvpp_rect *rects, int pad_y, int pad_u, int pad_v,
                            void *const *outs, void *stream);
/* What tsvpp_convert_letterbox WOULD launch, as one line of key=value text with tsvpp_describe_rois's keys: "mode=bilinear out=f32_planar dst=640x640 frames=2
 * launches=1 kernel=vpp_letterbox<...> shape=8x16 lds=.. grid=.. tiles=20x20 staged=.. tail=.. nt=.. limit=32", then "inner=WxH+left+top", the first frame's
 * rectangle.  Host only: needs no context and no GPU, the plane pointers in `in` are not read; TSVPP_* knobs are honoured.  lds= / grid= are the first launch's;
 * staged= is the number of frames whose every tile stages its source footprint in LDS (the others gather from global memory). */
int tsvpp_describe_letterbox(const tsvpp_params *p, int n, const tsvpp_nv12 *in, const tsvpp_rect *rects, int aligned_outputs, char *buf, size_t buf_len);

/* ---- tensors for a network: fp16 / bf16 / fp32 elements, per-channel mean and scale (not in the reference) ---------------------------------------------------
 * tsvpp_convert_rois / tsvpp_convert_rois_area / tsvpp_convert_letterbox stop one step short of what a network takes: they hand over fp32 x / 255, and the caller
 * runs a second element-wise pass for (x / 255 - mean[c]) / std[c], usually into half precision.  These entry points store that value themselves.
 * Contract.  Let q be the fp32 value the existing entry point stores for an element with p->normalization != 0: k / 255 correctly rounded, k the clamped colour
 * byte or the Y800 sample.  The element of stored channel c is
 *     cvt(dtype, (q - mean[c]) * scale[c])
 *   - two fp32 operations, a subtraction and then a multiplication, each rounded once, nothing fused;
 *   - TSVPP_F16 / TSVPP_BF16: converted ONCE, round to nearest even, IEEE: fp16 subnormals are kept, a magnitude beyond the type's range becomes infinity;
 *   - c indexes the channel AS STORED: plane 0, 1, 2 after the RGB / BGR choice (BGR24: mean[0] belongs to blue); Y800 uses mean[0] and scale[0] alone;
 *   - the caller passes scale = 1 / std: the library never divides;
 *   - dtype = TSVPP_F32, mean = 0, scale = 1 gives exactly the bits of the existing entry point;
 *   - in a letterbox canvas the pad pixel goes through the same expression as every sample.
 * Everything else is the existing entry point's, word for word: box and rectangle rules, output layout (planar: NCHW), splitting at TSVPP_MAX_ROIS (all four
 * resize types) / TSVPP_MAX_LETTERBOX, records by value in the kernarg segment, no allocation, no copy, no host synchronisation, legal under stream capture.
 * tsvpp_convert_rois_tensor accepts all four resize types: TSVPP_AREA runs tsvpp_convert_rois_area's kernel with that call's rules and limits (per box down-scale or
 * up-scale rule, at most 40 taps per axis, dst_width / dst_height up to 65536).
 * Supported outputs: RGB24 / BGR24 with TSVPP_PLANAR, and Y800, in all three dtypes.  MERGED (interleaved) tensor output is out of scope: TSVPP_UNSUPPORTED.
 *   outs[i]     tsvpp_tensor_bytes(p, spec) bytes, aligned to the element (2 or 4 bytes; TSVPP_ERROR otherwise).  16-byte aligned outputs take the vector stores,
 *               any other the element-wise kernel, as in the existing entry points.
 * Status, decided before any device is touched (the describe call returns the same one), in this order:
 *   1. the status of the existing entry point for the request (tsvpp_convert_rois's rules, tsvpp_convert_rois_area's for TSVPP_AREA, tsvpp_convert_letterbox's), if
 *      it is not TSVPP_OK;
 *   2. TSVPP_ERROR for a null `spec`, or a mean or scale that is not finite, or a scale of zero, in a channel the format uses (Y800: channel 0);
 *   3. TSVPP_UNSUPPORTED for an unknown dtype, p->normalization == 0, TSVPP_MERGED with RGB24 / BGR24, a fourcc outside RGB24 / BGR24 / Y800.
 * The describe calls print the existing keys; out= is f16_planar / bf16_planar / f32n_planar (Y800: f16_y800 / bf16_y800 / f32n_y800), kernel= names the tensor
 * instantiation (vpp_rois_tensor<...>, vpp_rois_area_tensor<...>, vpp_letterbox_tensor<...>; fp16 and bf16 share one, EL_HALF, that branches on the launch's dtype). */
enum tsvpp_dtype { TSVPP_F32 = 0, TSVPP_F16 = 1, TSVPP_BF16 = 2 };
typedef struct tsvpp_tensor_spec {
    int32_t dtype;  /* tsvpp_dtype */
    float mean[3];  /* per stored channel, in units of q (0..1) */
    float scale[3]; /* 1 / std */
} tsvpp_tensor_spec; /* 28 bytes */
/* channels * dst_width * dst_height * element size of one output; 0 for a (p, spec) pair the tensor entry points refuse (rules 2 and 3 above, a null `p`,
 * dst_width / dst_height that are not positive and even, an output of 4 GiB or more as fp32) */
size_t tsvpp_tensor_bytes(const tsvpp_params *p, const tsvpp_tensor_spec *spec);
int tsvpp_convert_rois_tensor(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois, const tsvpp_params *p,
                              const tsvpp_tensor_spec *spec, void *const *outs, void *stream);
int tsvpp_describe_rois_tensor(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois,
                               int aligned_outputs, char *buf, size_t buf_len);
int tsvpp_convert_letterbox_tensor(tsvpp_ctx *ctx, int n, const tsvpp_nv12 *in, const tsvpp_params *p, const tsvpp_tensor_spec *spec, const tsvpp_rect *rects,
                                   int pad_y, int pad_u, int pad_v, void *const *outs, void *stream);
int tsvpp_describe_letterbox_tensor(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n, const tsvpp_nv12 *in, const tsvpp_rect *rects,
                                    int aligned_outputs, char *buf, size_t buf_len);

/* ---- letterbox with AREA (not in the reference) ------------------------------------------------------------------------------------------------------------------
 * The letterbox call with the one filter a down-scale to a detector input should use.  1920 x 1080 into a 640 x 640 canvas is the exact ratio 3: every BILINEAR
 * weight is zero there and tsvpp_convert_letterbox point-samples one source pixel in nine (4K -> 640 is ratio 6, 720p -> 640 x 360 ratio 2).  Without this call
 * the answer is tsvpp_convert(AREA) into a temporary, a fill and a strided copy -- and the first tsvpp_convert of a scale allocates and synchronously copies a
 * device weight table, so that call cannot be captured.
 * One pair of entry points for both output families:
 *   spec == NULL  outputs and rules of tsvpp_convert_letterbox: uint8 / fp32, RGB24 / BGR24 planar and merged, Y800;
 *   spec != NULL  outputs and rules of tsvpp_convert_letterbox_tensor, word for word: planar and Y800 only, fp16 / bf16 / fp32 elements, outputs aligned to the
 *                 element, the pad through the same expression as every sample.
 * The differences to those calls:
 *   resize type   p->resize_type must be TSVPP_AREA; anything else is TSVPP_UNSUPPORTED (and the two existing pairs keep answering TSVPP_UNSUPPORTED for AREA).
 *   contract      the inner rectangle of canvas k is, bit for bit and in every flavour, what tsvpp_convert returns for frame k with dst = the rectangle's size and
 *                 TSVPP_AREA.  Per frame as Convert decides per request (reference src/Resize.cu:435): xr > 1 AND yr > 1 runs the weighted box of the down-scale,
 *                 any other frame the AREA up-scale rule (the 2 x 2 blend).  One launch may mix both.  The pad is tsvpp_convert_letterbox's.
 *   no tables     the kernel generates the weight rows a tile reads inside the tile, as tsvpp_convert_rois_area's does: no allocation, no copy, no host
 *                 synchronisation, nothing cached in the context, records by value in the kernarg segment -- legal under stream capture, the first call of a
 *                 scale included.  TSVPP_MAX_LETTERBOX frames per launch.
 *   limits        tsvpp_convert_rois_area's, with the rectangle as the output: TSVPP_UNSUPPORTED for a down-scale frame that needs more than 40 taps on an axis
 *                 (taps = ceil(ratio)) and for a rectangle side above 65536.  Deviation as there: a ratio whose weight pattern never closes is answered with the
 *                 generator's rows, where tsvpp_convert refuses it.
 *   cost          tsvpp_convert_rois_area's tile waits for one lane to run the generator over every output index in front of it.  The generator returns to its
 *                 initial state wherever its closing test passes -- periodically, every P indices -- so this kernel starts each chain at the last multiple of P in
 *                 front of its tile and runs first % P steps instead of `first`; a wave finds P by testing 64 candidates per round (csrc/vpp_letterbox_area.h).
 *                 1920 -> 640, 1080 -> 360, 3840 -> 640, 1280 -> 640: P = 1, no steps in front of any tile.  1920 -> 608: P = 57.  1366 -> 640: P = 320, up to
 *                 304 steps (the chroma chain in front of column 608, which starts at 0).  A pattern that does not close in front of a tile costs that tile what it costs in tsvpp_convert_rois_area; the rows are the same
 *                 either way.  The host neither searches periods nor plans tiles when converting.
 * Status, decided before any device is touched (the describe call returns the same one): tsvpp_convert_letterbox's, in its order; then the limits above; then,
 * with a spec, rules 2 and 3 of the tensor entry points.
 * tsvpp_describe_letterbox_area prints tsvpp_describe_letterbox's keys (mode=area, kernel=vpp_letterbox_area<...> / vpp_letterbox_area_tensor<...>; lds= includes
 * the weight rows) and then "inner=WxH+left+top down=<frames on the down-scale path> taps=<largest taps_x>x<largest taps_y> chain=<steps>": the most generator
 * steps any chain of any tile of the FIRST launch runs in front of its tile's first row (0 for 1920 x 1080 into 640 x 640).  chain= is worked out on the host, in
 * this call only. */
int tsvpp_convert_letterbox_area(tsvpp_ctx *ctx, int n, const tsvpp_nv12 *in, const tsvpp_params *p, const tsvpp_tensor_spec *spec /* may be NULL */,
                                 const tsvpp_rect *rects, int pad_y, int pad_u, int pad_v, void *const *outs, void *stream);
int tsvpp_describe_letterbox_area(const tsvpp_params *p, const tsvpp_tensor_spec *spec /* may be NULL */, int n, const tsvpp_nv12 *in, const tsvpp_rect *rects,
                                  int aligned_outputs, char *buf, size_t buf_len);
/* DEBUG ONLY (tests), host only: tsvpp_roi_area_rows as tsvpp_convert_letterbox_area's kernel produces the rows -- the generator begun at the jump start of
 * (scale, first), the largest multiple of the pattern's period that is <= first (0 where the pattern does not close in 1 .. first), which *start receives.
 * Arguments, result and statuses as tsvpp_roi_area_rows. */
int tsvpp_letterbox_area_rows(float scale, int first, int n, float *out, int max_floats, int *taps, int *start);

/* ---- regions of interest, each to its own output size (not in the reference) -----------------------------------------------------------------------------------
 * tsvpp_convert_rois with the output size taken PER BOX: text lines that go to one height and a width of their own, the levels of a pyramid or preview ladder,
 * the inputs of several heads (112 x 112, 96 x 32, 128 x 256) behind one detector pass.  With tsvpp_convert_rois that is one call per distinct size.
 * Contract: output i is, bit for bit and in every flavour, what tsvpp_convert_rois returns for the ONE box rois[i] with p->dst_width = rois[i].dst_width and
 * p->dst_height = rois[i].dst_height.  Ratios, the crop rule, an odd `left`, a box of exactly its output size and the replicated edges are inherited from there.
 *   rois[i]     tsvpp_roi's fields under tsvpp_roi's rules, then dst_width / dst_height: THIS box's output size, > 0 and even.
 *   outs[i]     tsvpp_rois_sized_bytes(p, spec, rois[i].dst_width, rois[i].dst_height) bytes of device memory, tight, laid out as tsvpp_convert_rois's output.
 *   p           resize_type, fourcc, planes, normalization.  p->dst_width and p->dst_height MUST BE 0 (a caller who sets them believes they apply: TSVPP_ERROR);
 *               p->crop_* must be zero.
 * Supported: NEAREST, BILINEAR, BICUBIC; RGB24 / BGR24 planar and merged, Y800; uint8 and fp32.  The tensor forms take tsvpp_convert_rois_tensor's `spec` under
 * that block's rules, word for word: planar and Y800 only, fp16 / bf16 / fp32, outputs aligned to their element.  AREA is TSVPP_UNSUPPORTED in all four entry points,
 * the tensor ones included: its kernel generates the weight rows of a tile behind a serial chain over the output columns in front of it, and wide strips are the
 * wrong shape for that -- a follow-up.
 * As in tsvpp_convert_rois: `frames`, `rois`, `outs` are HOST arrays and may be freed on return; the per-box records (tsvpp_convert_rois's 48 bytes + the output
 * size and the box's place in the grid: 64 bytes) travel BY VALUE in the kernarg segment, which bounds a launch to TSVPP_MAX_ROIS_SIZED boxes; no allocation, no
 * copy, no host synchronisation; legal while `stream` is being captured; always an ordinary in-order launch; TSVPP_OPT_COLOR_G_TERM and the context's coefficient
 * block are honoured.
 * Launch splitting.  Vector stores need a 16-byte aligned output and a box that is not a narrow tail (an output 4 k + 2 columns wide and narrower than 32).  Outputs
 * of different sizes packed tightly are misaligned all the time, and one such box must not drag the others onto the element-wise kernel: the call splits its boxes
 * into the vector-eligible ones and the rest, keeps the order inside each class and issues each class in chunks of TSVPP_MAX_ROIS_SIZED, the vector class first:
 * launches = ceil(n_vec / 48) + ceil(n_el / 48), all on `stream`.  The outputs are independent: the result does not depend on the split.
 * Status, decided before any device is touched (the describe calls return the same one); every TSVPP_ERROR condition over all boxes comes before any
 * TSVPP_UNSUPPORTED one:
 *   TSVPP_ERROR        everything tsvpp_convert_rois calls an error; a box with dst_width or dst_height <= 0; non-zero p->dst_width / p->dst_height (and,
 *                      converting: a null context, plane or output, a tensor output not aligned to its element)
 *   TSVPP_UNSUPPORTED  odd box width / height, odd dst_* of a box, odd frame size, AREA or an unknown resize type, an output format outside the list above, a box
 *                      whose source span reaches TSVPP_SOURCE_SPAN_LIMIT, a box whose output is 4 GiB or more (or has 2^31 / 48 tiles of 32 x 32 or more); then,
 *                      tensor forms, rules 2 and 3 of the tensor block above.
 * The describe line, key=value throughout: "mode=bilinear out=u8_merged dst=var rois=12 frames=2 launches=1 kernel=vpp_rois_sized<...> shape=8x16 lds=.. grid=..
 * sizes=<distinct output sizes> maxdst=<largest width>x<largest height> staged=<boxes whose every tile stages, all launches> vec=<boxes in vector launches> nt=..
 * limit=48".  lds=, grid=, kernel= and nt= are the FIRST launch's (the first vector chunk, or the first element-wise chunk of a request without vector boxes);
 * grid= is exactly the sum of its boxes' tile counts, ceil(w / 32) * ceil(h / 32) each.  `aligned_outputs` != 0 takes every output as 16-byte aligned. */
#define TSVPP_MAX_ROIS_SIZED 48 /* boxes per launch; more are split */
typedef struct tsvpp_roi_sized {
    int32_t frame, left, top, right, bottom; /* tsvpp_roi's fields and rules */
    int32_t dst_width, dst_height;           /* THIS box's output size: > 0, even */
} tsvpp_roi_sized;                           /* 28 bytes */
/* bytes of one output of the given size: tsvpp_out_bytes(p, w, h) with p->dst_* = w, h (spec == NULL), or the tensor form's channels * w * h * element size; 0 for
 * what the entry points refuse (a null `p`, AREA, a format outside the list, a size that is not positive and even, 4 GiB or more -- the tensor form: as fp32 --,
 * non-zero p->dst_* or p->crop_*, rules 2 and 3 of the tensor block) */
size_t tsvpp_rois_sized_bytes(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int dst_width, int dst_height);
int tsvpp_convert_rois_sized(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi_sized *rois, const tsvpp_params *p,
                             void *const *outs, void *stream);
int tsvpp_describe_rois_sized(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi_sized *rois, int aligned_outputs,
                              char *buf, size_t buf_len);
int tsvpp_convert_rois_sized_tensor(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi_sized *rois, const tsvpp_params *p,
                                    const tsvpp_tensor_spec *spec, void *const *outs, void *stream);
int tsvpp_describe_rois_sized_tensor(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n_frames, const tsvpp_nv12 *frames, int n_rois,
                                     const tsvpp_roi_sized *rois, int aligned_outputs, char *buf, size_t buf_len);
/* DEBUG ONLY (tests), host only: the (box, tile column, tile row) and the tile's first output column / row that workgroup `wg` of the FIRST launch of this request
 * takes -- the same __host__ __device__ function the kernel calls (sized_tile, csrc/vpp_rois_sized.h).  out5 = { box, txi, tyi, j_first, i_first }; `box` indexes
 * `rois`.  The request's status if it is not TSVPP_OK; TSVPP_ERROR for a null `out5` or wg outside [0, grid). */
int tsvpp_rois_sized_tile(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi_sized *rois, int aligned_outputs, unsigned wg,
                          int32_t *out5);

/* ---- affine warps (not in the reference) ---------------------------------------------------------------------------------------------------------------------
 * The second stage behind a detector when an axis-aligned box is not enough: a face aligned to 112 x 112 by a similarity transform, a rotated OCR / aerial box,
 * an affine crop for a pose head.  `n_warps` outputs, each p->dst_width x p->dst_height, each sampled BILINEAR out of one of `n_frames` NV12 frames through its own
 * 2 x 3 matrix, colour-converted and stored to its own output, in ceil(n_warps / TSVPP_MAX_WARPS) kernel launches (today: a tsvpp_convert of the whole frame to
 * fp32 planar, then a grid sampler over it -- a full-frame round trip through memory, and not this library's arithmetic).
 *   The map      m is the output -> source (inverse) map.  With u = j + 0.5, v = i + 0.5 the centre of output pixel (row i, column j), the source position is
 *                    X = m[0] u + m[1] v + m[2]        Y = m[3] u + m[4] v + m[5]
 *                in luma pixels of the WHOLE frame, pixel k covering [k, k + 1).  From OpenCV's index-based inverse matrix [a b c; d e f] (what warpAffine takes
 *                with WARP_INVERSE_MAP): m = (a, b, c + 0.5 - 0.5 (a + b), d, e, f + 0.5 - 0.5 (d + e)).
 *   Arithmetic   The host computes once per warp, in fp32 with one rounding each, tx = m[2] - 0.5f, ty = m[5] - 0.5f, ctx = m[2] * 0.5f - 0.5f,
 *                cty = m[5] * 0.5f - 0.5f (the multiplication by 0.5 is exact).  Luma, output pixel (i, j), contraction off, the fmaf()s explicit:
 *                    fx = fmaf((float)j + 0.5f, m[0], fmaf((float)i + 0.5f, m[1], tx))        fy = fmaf((float)j + 0.5f, m[3], fmaf((float)i + 0.5f, m[4], ty))
 *                then per axis the tail of the library's BILINEAR coordinate with limit = the frame's width / height: p = floor(f), w = f - p; p < 0 -> p = 0, w = 0;
 *                p > limit - 1 -> p = limit - 1, w = 0; the second tap is p + 1 if p + 1 < limit, else p (where w was forced to 0 it is multiplied by zero and need
 *                not be fetched).  The four taps go through the library's bilinear blend (the fma tree the reference's goldens pin), truncated.  Chroma pair
 *                (ci, cj): the same with ctx / cty on the pair's own indices, limits width / 2 and height / 2, U and V from byte columns 2 p and 2 p + 1 -- never
 *                derived from the luma coordinates.  The kernel clamps f into [-1, limit] before converting it to an integer, which changes no result.  The
 *                virtual NV12 frame of dst_width x dst_height that results goes through the one colour back end: the output is, bit for bit, what tsvpp_convert
 *                without a resize returns for that virtual frame.  With m = ((float)w / dst_w, 0, 0, 0, (float)h / dst_h, 0) the expressions reduce to the
 *                BILINEAR coordinate itself: the call equals tsvpp_convert(BILINEAR, dst) of the whole frame bit for bit.
 *   Border       border_y = border_u = border_v = -1: replicate -- the clamps above are the whole rule.  Otherwise each is 0..255 and a sample whose position lies
 *                outside the frame takes the border component instead of a blend: luma where fx < -0.5f || fx >= w - 0.5f || fy < -0.5f || fy >= h - 0.5f, chroma
 *                under the same test on its own fx, fy with w / 2, h / 2 (luma and chroma decide independently).  The border value then goes through the colour
 *                back end like any sample, as the letterbox pad does.
 * `frames`, `outs`, `p`, the output layout and size (tsvpp_out_bytes(p, dst_width, dst_height)) are tsvpp_convert_rois's, and so are: host arrays that may be freed on
 * return; the per-warp records (72 bytes) by value in the kernarg segment, which bounds a launch to TSVPP_MAX_WARPS; no allocation, no copy, no host
 * synchronisation; legal while `stream` is being captured; always an ordinary in-order launch; TSVPP_OPT_COLOR_G_TERM and the coefficient block honoured.
 * Supported: p->resize_type == TSVPP_BILINEAR; RGB24 / BGR24 planar and merged, Y800; uint8 and fp32.
 * Status, decided before any device is touched (tsvpp_describe_warp returns the same one):
 *   TSVPP_ERROR        null arguments, n_frames <= 0, n_warps <= 0, a frame without size or with a pitch below its width, `frame` out of range, dst_* <= 0, non-zero
 *                      crop_*, a border component outside -1..255 or a mix of -1 and non-negative components, a matrix entry that is not finite; when converting:
 *                      a null plane or output.
 *   TSVPP_UNSUPPORTED  odd dst_*, an odd frame size, a resize type other than BILINEAR, an output format outside the list, |m[k]| > 2^24 (with that bound every
 *                      coordinate is finite), an output of 4 GiB or more.
 * Out of scope, follow-ups: NEAREST / AREA warps, a device-resident matrix list, per-warp output sizes, merged half-precision tensors.  BICUBIC answers
 * TSVPP_UNSUPPORTED here: it has an entry point of its own, tsvpp_convert_warp_bicubic (below).  Perspective (3 x 3) maps are tsvpp_convert_perspective's (below). */
#define TSVPP_MAX_WARPS 32 /* outputs per launch; more are split */
typedef struct tsvpp_warp {
    int32_t frame; /* index into `frames` */
    float m[6];    /* output -> source, see above */
} tsvpp_warp;      /* 28 bytes */
int tsvpp_convert_warp(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_warps, const tsvpp_warp *warps, const tsvpp_params *p, int border_y, int border_u,
                       int border_v, void *const *outs, void *stream);
/* What tsvpp_convert_warp WOULD launch, as one line of key=value text with tsvpp_describe_rois's keys: "mode=warp_bilinear out=f32_planar dst=112x112 warps=33 frames=1
 * launches=2 kernel=vpp_warp<...> shape=8x16 lds=.. grid=.. tiles=4x4 staged=.. tail=.. nt=.. limit=32 border=replicate" (or border=Y,U,V).  staged = the warps whose
 * every tile stages its source bounding box in LDS; a launch may mix staged and gathering tiles.  Host only: needs no context and no GPU. */
int tsvpp_describe_warp(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_warps, const tsvpp_warp *warps, int border_y, int border_u, int border_v,
                        int aligned_outputs, char *buf, size_t buf_len);
/* The tensor forms: outputs, `spec` and the status rules are tsvpp_convert_rois_tensor's, word for word (rule 1 is tsvpp_convert_warp's status; rules 2 and 3 come
 * after it); the border sample goes through the spec like every sample.  Kernel names vpp_warp_tensor<...>. */
int tsvpp_convert_warp_tensor(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_warps, const tsvpp_warp *warps, const tsvpp_params *p,
                              const tsvpp_tensor_spec *spec, int border_y, int border_u, int border_v, void *const *outs, void *stream);
int tsvpp_describe_warp_tensor(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n_frames, const tsvpp_nv12 *frames, int n_warps, const tsvpp_warp *warps,
                               int border_y, int border_u, int border_v, int aligned_outputs, char *buf, size_t buf_len);
/* The matrix that maps the whole dst_w x dst_h output onto the box of size box_w x box_h centred at (cx, cy) (luma pixels) and rotated by angle_rad (from the x
 * axis towards the y axis, i.e. clockwise on screen).  With c = cos(angle_rad), s = sin(angle_rad), evaluated in double and each entry rounded once to float:
 *     m = (box_w c / dst_w, -box_h s / dst_h, cx - 0.5 box_w c + 0.5 box_h s,        box_w s / dst_w, box_h c / dst_h, cy - 0.5 box_w s - 0.5 box_h c)
 * Angle 0 with the box equal to the frame gives ((float)w / dst_w, 0, 0, 0, (float)h / dst_h, 0).  out->frame is left as it is.  TSVPP_ERROR for a null `out`, an
 * argument that is not finite, box_w / box_h / dst_w / dst_h <= 0. */
int tsvpp_warp_rotated_box(double cx, double cy, double box_w, double box_h, double angle_rad, int dst_w, int dst_h, tsvpp_warp *out);
/* DEBUG ONLY (tests), host only: the source bounding box the kernel and the host compute for output columns [j_first, j_last] / rows [i_first, i_last] (a tile:
 * even first, odd last) of `warp` on a frame of frame_w x frame_h: out8 = { xlo, xhi, ylo, yhi } in luma pixels, then { cxlo, cxhi, cylo, cyhi } in chroma pairs.
 * TSVPP_ERROR for null arguments, a frame size <= 0, an empty or negative range. */
int tsvpp_warp_footprint(const tsvpp_warp *warp, int frame_w, int frame_h, int j_first, int j_last, int i_first, int i_last, int32_t *out8);

/* ---- BICUBIC affine warps (not in the reference) ---------------------------------------------------------------------------------------------------------------
 * tsvpp_convert_warp with the library's BICUBIC in place of its BILINEAR: recognition heads are trained on bicubic-aligned crops, and an up-sampled plate or text
 * line is visibly soft under BILINEAR.  An entry point of its own because tsvpp_convert_warp's answer to BICUBIC (TSVPP_UNSUPPORTED) is part of its contract.  One
 * pair serves both output families: `spec` == NULL -- outputs and rules are tsvpp_convert_warp's (uint8 and fp32, RGB24 / BGR24 planar and merged, Y800); with a
 * `spec` they are tsvpp_convert_warp_tensor's, word for word.  tsvpp_warp, TSVPP_MAX_WARPS, the records by value in the kernarg segment, no allocation, no copy,
 * no host synchronisation, legality under stream capture, TSVPP_OPT_COLOR_G_TERM and the coefficient block: all as tsvpp_convert_warp.
 *   Coordinate   tsvpp_convert_warp's fx, fy, bit for bit (the two fused multiply-adds; chroma with ctx / cty on the pair grid, never derived from luma).  f is
 *                clamped into [-1, limit] before it becomes an integer, which changes no result.
 *   Axis         p = floor(f), w = f - p (exact in fp32); p < 0 -> p = 0, w = 0; p > limit - 1 -> p = limit - 1, w = 0: the library's BICUBIC axis on the warp's
 *                coordinate.  limit = the frame's width / height; chroma: half of each.
 *   Taps         the reference's edge rule: p - lo, p, p + hi, p + 2 hi with hi = 0 where p + 1 or p + 2 would leave the plane (BOTH upper taps collapse onto the
 *                centre), lo = 0 at the low edge, else 1; the same on rows.  Chroma: the rule on pairs with limits w / 2, h / 2, U from byte column 2 x, V from
 *                2 x + 1 (for an even width this is the resize's rule on byte columns with step 2).
 *   Sum          the library's BICUBIC: Keys' cubic with a = -0.75, coefficients from (double)w with the exact square and the correctly rounded cube,
 *                    c0 = (a w - 2a w2) + a w3    c1 = (1 - (a + 3) w2) + (a + 2) w3    c2 = ((-a) w + (2a + 3) w2) - (a + 2) w3    c3 = a w2 - a w3
 *                four horizontal sums ((c0 p0 + c1 p1) + c2 p2) + c3 p3 in fp64, each rounded half away from zero and clamped to 0..255, then the vertical sum
 *                of those four integers with the row weights, formed, rounded and clamped the same way.  (The kernel evaluates in fp32 and recomputes in fp64
 *                within 5e-4 of a tie: the result is the fp64 one.)  The virtual NV12 frame then goes through the one colour back end.
 *   Border       tsvpp_convert_warp's rule and test: -1, -1, -1 replicates -- the edge rule above is the whole rule; otherwise a sample whose position lies outside
 *                the frame takes the border component whole, never mixed into the cubic.
 *   Identities   m = ((float)w / dst_w, 0, 0, 0, (float)h / dst_h, 0) gives tsvpp_convert(BICUBIC, dst) of the whole frame bit for bit (the coordinate reduces to
 *                fmaf(j + 0.5f, ratio, -0.5f)); a translation by even integers inside the frame is the plain colour conversion of that crop (w = 0: coefficients
 *                0, 1, 0, 0).
 * Status: tsvpp_convert_warp's, in its order, with "a resize type other than BICUBIC" (BILINEAR, NEAREST, AREA, unknown: TSVPP_UNSUPPORTED); with a spec, rules 2
 * and 3 of the tensor block follow.  Out of scope: BICUBIC for tsvpp_convert_remap / tsvpp_convert_mesh, NEAREST / AREA warps, per-output sizes. */
int tsvpp_convert_warp_bicubic(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_warps, const tsvpp_warp *warps, const tsvpp_params *p,
                               const tsvpp_tensor_spec *spec /* may be NULL */, int border_y, int border_u, int border_v, void *const *outs, void *stream);
/* What tsvpp_convert_warp_bicubic WOULD launch: tsvpp_describe_warp's (with a spec: tsvpp_describe_warp_tensor's) line with mode=warp_bicubic and
 * kernel=vpp_warp_bicubic<...> (vpp_warp_bicubic_tensor<...>); every other key is that call's.  staged = the warps whose every tile stages its box in LDS: the
 * BILINEAR box with the 4-tap halo.  Host only: needs no context and no GPU. */
int tsvpp_describe_warp_bicubic(const tsvpp_params *p, const tsvpp_tensor_spec *spec /* may be NULL */, int n_frames, const tsvpp_nv12 *frames, int n_warps,
                                const tsvpp_warp *warps, int border_y, int border_u, int border_v, int aligned_outputs, char *buf, size_t buf_len);
/* DEBUG ONLY (tests), host only: tsvpp_warp_footprint for the BICUBIC call -- [p(min) - 1, p(max) + 2] per axis, clamped into the frame, p() the centre tap (the
 * floor clamped into 0 .. limit - 1) of the least and the greatest of the tile's corner coordinates: every tap lies in [p - 1, p + 2] and p is monotone in f.
 * Arguments and statuses as tsvpp_warp_footprint. */
int tsvpp_warp_bicubic_footprint(const tsvpp_warp *warp, int frame_w, int frame_h, int j_first, int j_last, int i_first, int i_last, int32_t *out8);

/* ---- perspective warps (not in the reference) ---------------------------------------------------------------------------------------------------------------
 * What no 2 x 3 matrix rectifies: a licence plate, a document page, a shelf label, a court seen from a broadcast camera, a road surface for a bird's-eye view --
 * quadrilaterals that are no parallelograms.  `n` outputs, each p->dst_width x p->dst_height, each sampled BILINEAR out of one of `n_frames` NV12 frames through
 * its own 3 x 3 homography, colour-converted and stored to its own output, in ceil(n / TSVPP_MAX_PERSP) kernel launches.
 *   The map      h is the output -> source homography, row-major.  With u = j + 0.5, v = i + 0.5 the centre of output pixel (row i, column j), the source position,
 *                in luma pixels of the WHOLE frame with pixel k covering [k, k + 1), is
 *                    X = (h[0] u + h[1] v + h[2]) / (h[6] u + h[7] v + h[8])        Y = (h[3] u + h[4] v + h[5]) / (h[6] u + h[7] v + h[8])
 *   Arithmetic   The half-pixel shift is folded into the numerators.  The host computes once per output, in fp32 with one rounding each (the products by 0.5 and
 *                by 2 are exact):
 *                    luma    ax = h0 - 0.5f h6    bx = h1 - 0.5f h7    cx = h2 - 0.5f h8        ay = h3 - 0.5f h6    by = h4 - 0.5f h7    cy = h5 - 0.5f h8
 *                            g  = h6              hh = h7              k  = h8
 *                    chroma  ax' = h0 - h6        bx' = h1 - h7        cx' = h2 0.5f - h8 0.5f  ay' = h3 - h6        by' = h4 - h7        cy' = h5 0.5f - h8 0.5f
 *                            g' = 2 h6            hh' = 2 h7           k'  = h8
 *                Per sample, contraction off, the fmaf()s explicit, u = (float)j + 0.5f, v = (float)i + 0.5f:
 *                    nx = fmaf(u, ax, fmaf(v, bx, cx))        ny = fmaf(u, ay, fmaf(v, by, cy))        nw = fmaf(u, g, fmaf(v, hh, k))
 *                    rw = 1.0f / nw   (IEEE, correctly rounded)        fx = nx * rw        fy = ny * rw
 *                One reciprocal and two products, not two divisions.  Chroma pair (ci, cj): the same expressions with the primed terms on the pair's own indices
 *                -- never derived from the luma coordinates.  From fx, fy on everything is tsvpp_convert_warp's, word for word: the axis tail with limit = the
 *                frame's width / height (chroma: half of each), the four taps through the library's bilinear blend, U and V from byte columns 2 p and 2 p + 1,
 *                the border rule, and the virtual NV12 frame through the one colour back end.  Hence: with h = (m0, m1, m2, m3, m4, m5, 0, 0, 1) the output is
 *                bit for bit tsvpp_convert_warp's with m (cx = m2 - 0.5f is tx, cx' = m2 0.5f - 0.5f is ctx, nw = rw = 1 and nx * 1 is exact), so the scale-only
 *                homography equals tsvpp_convert(BILINEAR, dst) of the whole frame; and h and 4 h give the same bits (every operation scales exactly).
 *   Domain       nw is monotone in u and in v separately (every operation is monotone, rounding is monotone), so its extremes over the output are those of the
 *                four corner pixels.  The request is TSVPP_UNSUPPORTED unless nw >= 2^-64, evaluated by the expression above, at the four corner pixels of the
 *                luma grid and at the four corner pairs of the chroma grid.  Then every rw is finite and positive (<= 2^64), every coordinate is finite and no
 *                NaN can arise.  A map whose vanishing line (the horizon) crosses the output has no answer here.
 *   Border       as tsvpp_convert_warp: -1, -1, -1 replicates; else a sample whose position lies outside the frame takes the border component.
 * `frames`, `outs`, `p`, the output layout and everything about the call are tsvpp_convert_warp's: host arrays that may be freed on return; the per-output records
 * (112 bytes) by value in the kernarg segment, which bounds a launch to TSVPP_MAX_PERSP; no allocation, no copy, no host synchronisation; legal while `stream` is
 * being captured; TSVPP_OPT_COLOR_G_TERM and the coefficient block honoured.  Supported: TSVPP_BILINEAR; RGB24 / BGR24 planar and merged, Y800; uint8 and fp32.
 * Status, decided before any device is touched (tsvpp_describe_perspective returns the same one), in tsvpp_convert_warp's order:
 *   TSVPP_ERROR        everything tsvpp_convert_warp answers with it, an entry of h that is not finite among them; when converting: a null plane or output.
 *   TSVPP_UNSUPPORTED  everything tsvpp_convert_warp answers with it (|h[k]| > 2^24 for its matrix bound), then the horizon rule above.
 * Out of scope, TSVPP_UNSUPPORTED or follow-ups: NEAREST / AREA sampling, a device-resident matrix list, per-output sizes, merged half-precision tensors, maps
 * whose horizon crosses the output.  BICUBIC answers TSVPP_UNSUPPORTED here: it has an entry point of its own, tsvpp_convert_perspective_bicubic (below). */
#define TSVPP_MAX_PERSP 32 /* outputs per launch; more are split */
typedef struct tsvpp_persp {
    int32_t frame; /* index into `frames` */
    float h[9];    /* output -> source, row-major, see above */
} tsvpp_persp;     /* 40 bytes */
int tsvpp_convert_perspective(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n, const tsvpp_persp *persps, const tsvpp_params *p, int border_y,
                              int border_u, int border_v, void *const *outs, void *stream);
/* What tsvpp_convert_perspective WOULD launch: tsvpp_describe_warp's line and keys (warps= counts the outputs) with mode=persp_bilinear, kernel=vpp_persp<...> (tensor form:
 * vpp_persp_tensor<...>) and limit=32.  staged = the outputs whose every tile stages its interval box in LDS.  Host only: needs no context and no GPU. */
int tsvpp_describe_perspective(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n, const tsvpp_persp *persps, int border_y, int border_u,
                               int border_v, int aligned_outputs, char *buf, size_t buf_len);
/* The tensor forms: outputs, `spec` and the status rules are tsvpp_convert_warp_tensor's (rule 1 is tsvpp_convert_perspective's status; rules 2 and 3 come after
 * it); the border sample goes through the spec like every sample. */
int tsvpp_convert_perspective_tensor(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n, const tsvpp_persp *persps, const tsvpp_params *p,
                                     const tsvpp_tensor_spec *spec, int border_y, int border_u, int border_v, void *const *outs, void *stream);
int tsvpp_describe_perspective_tensor(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n_frames, const tsvpp_nv12 *frames, int n, const tsvpp_persp *persps,
                                      int border_y, int border_u, int border_v, int aligned_outputs, char *buf, size_t buf_len);
/* The homography that maps the corners of the dst_w x dst_h output onto the source points quad = (x0, y0, x1, y1, x2, y2, x3, y3) (luma pixels), in the order
 * top-left, top-right, bottom-right, bottom-left: Heckbert's closed form, evaluated in double, each entry rounded once to float.
 *     sx = x0 - x1 + x2 - x3        sy = y0 - y1 + y2 - y3        dx1 = x1 - x2   dx2 = x3 - x2   dy1 = y1 - y2   dy2 = y3 - y2
 *     sx == 0 and sy == 0 (a parallelogram): g = h = 0 exactly;  otherwise den = dx1 dy2 - dx2 dy1, g = (sx dy2 - dx2 sy) / den, h = (dx1 sy - sx dy1) / den
 *     h0 = (x1 - x0 + g x1) / dst_w   h1 = (x3 - x0 + h x3) / dst_h   h2 = x0        h3 = (y1 - y0 + g y1) / dst_w   h4 = (y3 - y0 + h y3) / dst_h   h5 = y0
 *     h6 = g / dst_w                  h7 = h / dst_h                  h8 = 1
 * out->frame is left as it is.  TSVPP_ERROR for null arguments, an input that is not finite, dst_w / dst_h <= 0, den == 0.  Whether the result is usable (a convex
 * quad, the horizon off the output) is the request rules' decision, not this helper's. */
int tsvpp_persp_from_quad(const double quad[8], int dst_w, int dst_h, tsvpp_persp *out);
/* DEBUG ONLY (tests), host only: tsvpp_warp_footprint for `persp` -- the interval box the kernel and the host compute for a tile.  TSVPP_ERROR as there;
 * TSVPP_UNSUPPORTED where the denominator falls below 2^-64 on either grid of the range (the request rules refuse such an output). */
int tsvpp_persp_footprint(const tsvpp_persp *persp, int frame_w, int frame_h, int j_first, int j_last, int i_first, int i_last, int32_t *out8);

/* ---- BICUBIC perspective warps (not in the reference) ------------------------------------------------------------------------------------------------------------
 * tsvpp_convert_perspective with the library's BICUBIC: the coordinate is tsvpp_convert_perspective's, bit for bit (two numerators, one denominator, one
 * reciprocal, two products; chroma with the primed terms on the pair grid); from fx, fy on everything is tsvpp_convert_warp_bicubic's, word for word -- axis,
 * taps, sum, border.  Hence: h = (m0, m1, m2, m3, m4, m5, 0, 0, 1) gives the bits of tsvpp_convert_warp_bicubic with m, and h and 4 h give the same bits.  `spec`
 * == NULL: outputs and rules of tsvpp_convert_perspective; with a spec, of tsvpp_convert_perspective_tensor.  tsvpp_persp, TSVPP_MAX_PERSP and everything about
 * the call are tsvpp_convert_perspective's.  Status: tsvpp_convert_perspective's, in its order (the horizon rule included), with "a resize type other than
 * BICUBIC"; with a spec, rules 2 and 3 of the tensor block follow. */
int tsvpp_convert_perspective_bicubic(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n, const tsvpp_persp *persps, const tsvpp_params *p,
                                      const tsvpp_tensor_spec *spec /* may be NULL */, int border_y, int border_u, int border_v, void *const *outs, void *stream);
/* What tsvpp_convert_perspective_bicubic WOULD launch: tsvpp_describe_perspective's (with a spec: its tensor form's) line with mode=persp_bicubic and
 * kernel=vpp_persp_bicubic<...> (vpp_persp_bicubic_tensor<...>).  Host only: needs no context and no GPU. */
int tsvpp_describe_perspective_bicubic(const tsvpp_params *p, const tsvpp_tensor_spec *spec /* may be NULL */, int n_frames, const tsvpp_nv12 *frames, int n,
                                       const tsvpp_persp *persps, int border_y, int border_u, int border_v, int aligned_outputs, char *buf, size_t buf_len);
/* DEBUG ONLY (tests), host only: tsvpp_persp_footprint for the BICUBIC call -- the interval box with the 4-tap halo, [p(min) - 1, p(max) + 2] per axis, clamped
 * into the frame.  Arguments and statuses as tsvpp_persp_footprint. */
int tsvpp_persp_bicubic_footprint(const tsvpp_persp *persp, int frame_w, int frame_h, int j_first, int j_last, int i_first, int i_last, int32_t *out8);

/* ---- per-pixel coordinate maps (not in the reference) ----------------------------------------------------------------------------------------------------------
 * What no matrix describes: the lens.  Undistortion of wide-angle, fisheye and action cameras, stereo rectification, undistort and resize in one pass, cylindrical
 * and polar unwraps, a stabiliser's mesh warp -- OpenCV's remap.  `n` outputs, each p->dst_width x p->dst_height, each sampled BILINEAR out of one of `n_frames`
 * NV12 frames through one of `n_maps` coordinate maps in DEVICE memory, colour-converted and stored to its own output, in ceil(n / TSVPP_MAX_REMAPS) kernel
 * launches (today: a tsvpp_convert of the whole frame to fp32 planar, then a grid sampler over it).
 *   The map      dst_height rows of dst_width (x, y) pairs, interleaved fp32 (OpenCV's CV_32FC2, a torch tensor (H, W, 2)), rows `pitch` bytes apart.  It is
 *                OpenCV's: index-based, pixel k centred at k.  Output pixel (row i, column j) samples at fx = map[i][j].x, fy = map[i][j].y with no arithmetic at
 *                all -- the index space of tsvpp_convert_warp's fx / fy after its - 0.5f.
 *   Chroma       never derived from the luma taps.  Pair (ci, cj) takes the four luma entries of its 2 x 2 block, x00 x01 / x10 x11 (rows 2 ci, 2 ci + 1, columns
 *                2 cj, 2 cj + 1), and computes in fp32, contraction off, s = (x00 + x01) + (x10 + x11) -- three additions in that order, each rounded -- then
 *                cfx = fmaf(s, 0.125f, -0.25f): the block's mean position moved to the pair grid.  cfy likewise from the y entries.
 *   Any bits     Every bit pattern is a legal coordinate.  Each coordinate is clamped first, c = fminf(fmaxf(f, -1.0f), (float)limit), limit = the frame's width or
 *                height (chroma: half of it).  fmaxf comes first, so a NaN counts as -1 -- the NaN that +inf + -inf makes in s included.  Everything after the
 *                clamp works on c.  (For tsvpp_convert_warp this clamp changes no result.)
 *   Sampling     From c on everything is tsvpp_convert_warp's, word for word: the axis tail, the four taps through the library's bilinear blend, U and V from byte
 *                columns 2 p and 2 p + 1, the border rule evaluated on c (luma and chroma decide independently; -1, -1, -1 replicates), and the virtual NV12 frame
 *                of dst_width x dst_height through the one colour back end.
 *   Identities   The identity map x = j, y = i with dst equal to the frame size is tsvpp_convert without a resize.  A map that holds the BILINEAR coordinates of an
 *                exact power-of-two ratio (x = 2 j + 0.5, y = 2 i + 0.5 on a frame twice the output) is tsvpp_convert(BILINEAR) at that ratio.  A translation by
 *                even integers inside the frame is the plain colour conversion of that crop.  A general affine map is NOT bit-identical to tsvpp_convert_warp of
 *                the same matrix: the chroma coordinate here is the rounded mean of four rounded luma coordinates, there an expression of its own (at
 *                w / dst = 322 / 70 the two differ by up to 1.5e-5).
 *   Map memory   is read when the kernel runs -- at launch or at graph replay: the records hold the pointer, not the data, so a captured graph sees map updates.
 *                The kernel reads no byte outside dst_height rows x 8 * dst_width bytes of each map: pitch padding is never touched.
 *   LDS hint     A tile stages the bounding box of its taps in LDS, and the kernel finds that box itself (a min / max reduction over the workgroup): the host never
 *                sees the map and plans nothing per tile.  So it cannot size the launch's LDS either.  Without a hint a launch asks for the context's budget
 *                (TSVPP_LDS_KB, default 40 KiB, less the kernel's static LDS).  With lds_bytes > 0 on the maps a launch uses it asks for the largest hint among
 *                them, capped by the budget; a map without a hint counts as the budget.  A tile whose box needs more than the launch has gathers its taps from
 *                global memory: a wrong hint is never wrong, only slower.  A smooth undistortion map needs 2 - 4 KiB per tile, and the hint restores the
 *                occupancy a 40 KiB request costs.  tsvpp_remap_lds_need computes it from a host copy of the map.
 * `frames`, `outs`, `p`, the output layout and everything about the call are tsvpp_convert_warp's: host arrays (maps and remaps too) that may be freed on return;
 * the per-output records (56 bytes) by value in the kernarg segment, which bounds a launch to TSVPP_MAX_REMAPS; no allocation, no copy, no host synchronisation;
 * legal while `stream` is being captured; TSVPP_OPT_COLOR_G_TERM and the coefficient block honoured.  Supported: TSVPP_BILINEAR; RGB24 / BGR24 planar and merged,
 * Y800; uint8 and fp32.
 * Status, decided before any device is touched (tsvpp_describe_remap returns the same one), in tsvpp_convert_warp's order:
 *   TSVPP_ERROR        everything tsvpp_convert_warp answers with it except its matrix rule; null `maps` or `remaps`, n_maps <= 0; `map` out of range; a pitch that
 *                      is non-zero and below 8 * dst_width or no multiple of 8; a negative lds_bytes; when converting: a null plane or output, an `xy` that is
 *                      null or not 8-byte aligned.
 *   TSVPP_UNSUPPORTED  odd dst_*, an odd frame size, a resize type other than BILINEAR, an output format outside the list, an output of 4 GiB or more.
 * Out of scope, follow-ups: NEAREST / BICUBIC sampling, fixed-point (CV_16SC2) and split x / y maps, per-output sizes, merged half-precision tensors. */
#define TSVPP_MAX_REMAPS 32 /* outputs per launch; more are split */
typedef struct tsvpp_map {
    const float *xy;   /* DEVICE memory: dst_height rows of dst_width (x, y) pairs, interleaved fp32; 8-byte aligned */
    int32_t pitch;     /* bytes per row; 0 = tight (8 * dst_width) */
    int32_t lds_bytes; /* hint, 0 = none: see "LDS hint" */
} tsvpp_map;           /* 16 bytes */
typedef struct tsvpp_remap {
    int32_t frame; /* index into `frames` */
    int32_t map;   /* index into `maps` */
} tsvpp_remap;     /* 8 bytes */
int tsvpp_convert_remap(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_maps, const tsvpp_map *maps, int n, const tsvpp_remap *remaps,
                        const tsvpp_params *p, int border_y, int border_u, int border_v, void *const *outs, void *stream);
/* What tsvpp_convert_remap WOULD launch: tsvpp_describe_warp's line with mode=remap_bilinear, remaps=<n> maps=<n_maps> for warps=, kernel=vpp_remap<OUT,vec|elem,
 * staged|gather,replicate|border> (tensor form: vpp_remap_tensor<...>) and limit=32.  There is no staged= count: the host cannot know it.  lds= is the first
 * launch's dynamic LDS, and the kernel is the staged one iff that is non-zero.  `xy` is not read and may be null.  Host only: needs no context and no GPU. */
int tsvpp_describe_remap(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_maps, const tsvpp_map *maps, int n, const tsvpp_remap *remaps,
                         int border_y, int border_u, int border_v, int aligned_outputs, char *buf, size_t buf_len);
/* The tensor forms: outputs, `spec` and the status rules are tsvpp_convert_rois_tensor's (rule 1 is tsvpp_convert_remap's status; rules 2 and 3 come after it);
 * the border sample goes through the spec like every sample. */
int tsvpp_convert_remap_tensor(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_maps, const tsvpp_map *maps, int n, const tsvpp_remap *remaps,
                               const tsvpp_params *p, const tsvpp_tensor_spec *spec, int border_y, int border_u, int border_v, void *const *outs, void *stream);
int tsvpp_describe_remap_tensor(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n_frames, const tsvpp_nv12 *frames, int n_maps, const tsvpp_map *maps,
                                int n, const tsvpp_remap *remaps, int border_y, int border_u, int border_v, int aligned_outputs, char *buf, size_t buf_len);
/* DEBUG ONLY (tests), host only: the source bounding box the kernel computes for output columns [j_first, j_last] / rows [i_first, i_last] (a tile: even first,
 * odd last) of a map of dst_w x dst_h entries on a frame of frame_w x frame_h, from `host_xy`, a HOST copy of the map (`pitch` bytes per row, 0 = tight):
 * out8 = { xlo, xhi, ylo, yhi } in luma pixels, then { cxlo, cxhi, cylo, cyhi } in chroma pairs -- floor of the least clamped coordinate .. floor of the largest
 * + 1, clamped into the frame.  TSVPP_ERROR for null arguments, a size <= 0, an odd size, a bad pitch, a range that is empty or leaves the map. */
int tsvpp_remap_footprint(const float *host_xy, int pitch, int dst_w, int dst_h, int frame_w, int frame_h, int j_first, int j_last, int i_first, int i_last,
                          int32_t *out8);
/* Host only: the largest LDS need (bytes) over all 32 x 32 tiles of a map on a frame_w x frame_h frame, from a HOST copy -- what a caller puts into
 * tsvpp_map::lds_bytes.  Both tilings count: the plain one and, for 4 k + 2 >= 32 columns, the last tile column shifted to the right edge.  `luma_only`: for Y800
 * outputs, which stage no chroma.  A negative status for the arguments tsvpp_remap_footprint refuses. */
int tsvpp_remap_lds_need(const float *host_xy, int pitch, int dst_w, int dst_h, int frame_w, int frame_h, int luma_only);

/* ---- sparse control-grid warps: the warp mesh (not in the reference) ---------------------------------------------------------------------------------------------
 * The maps people use are smooth: undistortion, rectification, cylindrical unwraps, a stabiliser's per-frame mesh, rolling-shutter correction are described to a
 * few hundredths of a pixel by one control point per 16 x 16 or 32 x 32 output pixels -- the form every vendor dewarper takes.  A dense map is the largest thing
 * tsvpp_convert_remap reads (16.6 MB at 1080p, to produce and upload per frame for a stabiliser); the same warp as a 16 x 16 mesh is 67 KB.  tsvpp_convert_mesh is
 * tsvpp_convert_remap with the coordinate COMPUTED from four control points instead of read, and that computation is a contract:
 *   Control grid cols = ((dst_width - 1) >> log2_cw) + 2 points per row, rows = ((dst_height - 1) >> log2_ch) + 2 rows (tsvpp_mesh_dims), (x, y) interleaved fp32,
 *                rows `pitch` bytes apart, in DEVICE memory.  Control point (r, c) is the source position -- index-based, as a dense map's entry -- of output
 *                pixel (row r << log2_ch, column c << log2_cw).  The last row and column may lie beyond the output.
 *   Coordinate   of output pixel (row i, column j), per component, in fp32 with contraction off: c = j >> log2_cw, tx = (float)(j & (cw - 1)) * (1.0f / cw) with
 *                cw = 1 << log2_cw (exact); r and ty likewise from i.  With A = P[r][c], B = P[r][c + 1], C = P[r + 1][c], D = P[r + 1][c + 1]:
 *                    top = fmaf(tx, B - A, A)      bot = fmaf(tx, D - C, C)      f = fmaf(ty, bot - top, top)
 *                three subtractions and three fused multiply-adds, each rounded once.  At a control point f is the control value itself.
 *   From f on    the dense call, word for word: E(mesh), the dst_height x dst_width map of these f, is a tsvpp_map, and the result is, bit for bit,
 *                tsvpp_convert_remap of E(mesh).  The chroma coordinate of a pair comes from the four UNCLAMPED f of its 2 x 2 block; the clamp ("any bits": a NaN,
 *                the one inf - inf makes here included, counts as -1), the sampler, the border rule, the colour back end, the staging decision per tile (the
 *                footprint is reduced from the tile's own clamped coordinates: tsvpp_remap_footprint of E(mesh) describes it) and the LDS hint are that call's.
 *   Identities   hold because the interpolation of such control points is exact: the identity mesh x = j, y = i with dst equal to the frame is tsvpp_convert
 *                without a resize; the mesh of x = 2 j + 0.5, y = 2 i + 0.5 is tsvpp_convert(BILINEAR) at 2 : 1; a translation by even integers is the crop.
 *   Mesh memory  is read when the kernel runs (a captured graph sees mesh updates); no byte outside rows x 8 * cols bytes of a mesh is read: pitch padding is
 *                never touched.
 * Everything about the call is tsvpp_convert_remap's: `remaps` pairs a frame with a mesh (`map` indexes `meshes`); host arrays that may be freed on return; the
 * per-output records (64 bytes, a record type of this call's own) by value in the kernarg segment, ceil(n / TSVPP_MAX_MESHES) launches; no allocation, no copy,
 * no host synchronisation; legal under stream capture; the same formats, border, TSVPP_OPT_COLOR_G_TERM and coefficient block.
 * Status, in tsvpp_convert_remap's order with the mesh rules where its map rules are:
 *   TSVPP_ERROR        what tsvpp_convert_remap answers with it for frames, remaps, sizes and border; null `meshes`, n_meshes <= 0; `map` out of range; a pitch that
 *                      is no multiple of 8 or -- for a cell size inside 2..8 -- non-zero and below 8 * cols; a negative lds_bytes; when converting: a null
 *                      plane or output, an `xy` that is null or not 8-byte aligned.
 *   TSVPP_UNSUPPORTED  what tsvpp_convert_remap answers with it; a log2_cw or log2_ch outside 2..8.
 * Out of scope: cell sizes that are no power of two, bicubic or spline interpolation of the control points, NEAREST / BICUBIC sampling, per-output sizes. */
#define TSVPP_MAX_MESHES 32 /* outputs per launch; more are split */
typedef struct tsvpp_mesh {
    const float *xy;          /* DEVICE memory: rows x cols control points, (x, y) interleaved fp32, 8-byte aligned */
    int32_t pitch;            /* bytes per control row; 0 = tight (8 * cols) */
    int32_t log2_cw, log2_ch; /* cell size in output pixels: 2..8 each (4 .. 256 pixels) */
    int32_t lds_bytes;        /* hint, as tsvpp_map's */
} tsvpp_mesh;                 /* 24 bytes */
int tsvpp_convert_mesh(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_meshes, const tsvpp_mesh *meshes, int n, const tsvpp_remap *remaps,
                       const tsvpp_params *p, int border_y, int border_u, int border_v, void *const *outs, void *stream);
/* What tsvpp_convert_mesh WOULD launch: tsvpp_describe_remap's line with mode=mesh_bilinear, meshes=<n_meshes> cell=<W>x<H> (the first mesh's cell) for maps=,
 * kernel=vpp_mesh<OUT,vec|elem,staged|gather,replicate|border> (tensor form: vpp_mesh_tensor<...>) and limit=32.  `xy` is not read.  Host only. */
int tsvpp_describe_mesh(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_meshes, const tsvpp_mesh *meshes, int n, const tsvpp_remap *remaps,
                        int border_y, int border_u, int border_v, int aligned_outputs, char *buf, size_t buf_len);
/* The tensor forms, under the rules of tsvpp_convert_remap_tensor. */
int tsvpp_convert_mesh_tensor(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_meshes, const tsvpp_mesh *meshes, int n, const tsvpp_remap *remaps,
                              const tsvpp_params *p, const tsvpp_tensor_spec *spec, int border_y, int border_u, int border_v, void *const *outs, void *stream);
int tsvpp_describe_mesh_tensor(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n_frames, const tsvpp_nv12 *frames, int n_meshes, const tsvpp_mesh *meshes,
                               int n, const tsvpp_remap *remaps, int border_y, int border_u, int border_v, int aligned_outputs, char *buf, size_t buf_len);
/* Host only, all of the following: no context, no GPU; meshes and maps are HOST copies, pitches in bytes with 0 = tight.  Each returns TSVPP_ERROR for a null
 * argument, a size <= 0 or odd, or a bad pitch, and TSVPP_UNSUPPORTED for a cell size outside 2..8.
 * tsvpp_mesh_dims: the control grid of a dst_w x dst_h output, cols and rows as above. */
int tsvpp_mesh_dims(int dst_w, int dst_h, int log2_cw, int log2_ch, int *cols, int *rows);
/* E(mesh): the dense map (dst_h rows of dst_w (x, y) pairs) that tsvpp_convert_mesh samples through, computed by the function the kernel calls. */
int tsvpp_mesh_expand(const float *host_mesh, int pitch, int dst_w, int dst_h, int log2_cw, int log2_ch, float *out_xy, int out_pitch);
/* A dense map sampled at the control positions.  A position past the last pixel of an axis is linearly extrapolated from that axis's last two entries, in double,
 * x first and then y; each value is rounded once to float. */
int tsvpp_mesh_from_map(const float *host_xy, int pitch, int dst_w, int dst_h, int log2_cw, int log2_ch, float *out_mesh, int out_pitch);
/* The largest |E(mesh) - map| over the entries where both are finite (either component), so that a caller can pick a cell size. */
int tsvpp_mesh_error(const float *host_xy, int pitch, int dst_w, int dst_h, const float *host_mesh, int mesh_pitch, int log2_cw, int log2_ch, float *max_abs);
/* tsvpp_remap_lds_need of E(mesh): what a caller puts into tsvpp_mesh::lds_bytes. */
int tsvpp_mesh_lds_need(const float *host_mesh, int pitch, int dst_w, int dst_h, int log2_cw, int log2_ch, int frame_w, int frame_h, int luma_only);

/* Pre-build everything a (params, input size) pair needs so that later tsvpp_convert* calls for it touch no
 * allocator -- e.g. before hipGraph capture: the AREA weight tables (the reference mallocs, copies and leaks them
 * per frame, src/Resize.cu:389-406,436-452) and, for UYVY / YUV444 behind a resize, the resized-NV12 scratch of
 * `stream` sized for calls of up to `n_frames` frames (the reference cudaMallocs that intermediate per frame,
 * src/Resize.cu:411-416).  BILINEAR / AREA up-scale requests also get the geometry tables of the 2x2-tap kernel (tile
 * footprints, per-column and per-row coordinates and weights, evaluated once on the host) for the tile shape a batch of
 * `n_frames` frames runs with; a conversion that was not prepared builds them on first use -- except while its stream
 * is being captured into a graph, where it never allocates and runs the kernel that computes coordinates itself (same
 * bits).  The tables are prepared for frames as the decoder delivers them: pitches that are multiples of 16 and plane
 * pointers that keep the crop origin dword-aligned; a conversion whose real pitches / alignment select another tile shape
 * builds its own set on first use (or, while capturing, runs the self-computing kernel).  A context keeps the table sets of
 * its 1024 most recently used geometries.  tsvpp_prepare == tsvpp_prepare_batch(..., 0, NULL): tables only (single-frame
 * tile shape). */
int tsvpp_prepare(tsvpp_ctx *ctx, const tsvpp_params *p, int in_width, int in_height);
int tsvpp_prepare_batch(tsvpp_ctx *ctx, const tsvpp_params *p, int in_width, int in_height, int n_frames, void *stream);

/* Memory a context keeps although it no longer uses it.  Nothing is ever freed under running work: a geometry-table set pushed out of the cache (the 1024 most recently
 * used geometries stay) and an outgrown NV12 scratch buffer are RETIRED -- a launch already enqueued, or a captured hipGraph, may still hold their addresses, and a
 * hipFree would synchronise the device.  A context retires at most 256 MiB of table sets (a table set is tens of KiB: several thousand distinct geometries); past that,
 * new geometries run the kernels that compute their own coordinates (same bits, slower) and the library says so once on stderr.  tsvpp_trim releases the retired
 * memory: call it at a QUIESCENT point -- every conversion enqueued through this context has finished and no hipGraph captured from it will be replayed again.
 * `released_bytes` (may be NULL) receives the bytes of table sets released. */
int tsvpp_trim(tsvpp_ctx *ctx, size_t *released_bytes);

/* roctx ranges around every conversion ("tsvpp_convert n=.. WxH->WxH ..."), the counterpart of the reference's NVTX
 * ranges (include/Common.h:72-105 PUSH_RANGE/POP_RANGE, src/VideoProcessor.cpp:95; switched on by
 * Logger::enableNVTX / TensorStreamConverter.enable_nvtx()).  The tracer library (rocprofiler-sdk-roctx or
 * libroctx64) is looked up at run time; TSVPP_UNSUPPORTED if neither is installed. */
int tsvpp_enable_markers(tsvpp_ctx *ctx, int on);

/* ---- context options (round 6; not in the reference) -----------------------------------------------------------------------------------------------
 * TSVPP_OPT_INPUTS_READY (default 0).  The reference's getFrame hands a consumer a frame the decoder has FINISHED (Decoder::GetFrame blocks on a condition
 * variable until the decode thread publishes it, reference src/Decoder.cpp:97-131) and converts it into a buffer nobody else uses; its consumer streams
 * carry nothing but conversions (src/VideoProcessor.cpp:98-104).  A pipeline with that shape may set this option: every fused launch of the context then goes
 * out with the AQL barrier bit cleared (hipExtAnyOrderLaunch) -- it does not wait for work enqueued EARLIER on its stream, so back-to-back single-frame
 * conversions of one consumer overlap instead of paying a dependent-launch boundary each (~1.5-1.9 us against ~2.3 us of HBM time for a 1080p -> 720p frame).
 * Consumers served through tsvpp_consumer_next_stream additionally alternate between two streams (see there).
 * The caller promises, for every conversion while the option is set:
 *   (1) the input planes are complete in device memory when the call is made (not merely enqueued earlier on `stream`);
 *   (2) nothing enqueued earlier on `stream` still reads or writes the output buffer.
 * What stays ordered: anything enqueued LATER on the stream (events, copies, other kernels, synchronisation) still waits for the conversion; the two-pass
 * formats (UYVY / YUV444 where no single-pass kernel applies) and launches out of a tsvpp_table never use the option (their scratch buffer / table upload
 * are ordered by the stream).
 * Results are identical either way.
 * Value: 0 = off; 1 = on; (2 / 3: A-B values -- 2 = barrier-free launches without the second stream, 3 = the second stream without barrier-free launches). */
#define TSVPP_OPT_INPUTS_READY 1
/* TSVPP_OPT_COLOR_G_TERM (default 0).  The colour conversion's green chroma term `-0.813 (V-128) - 0.391 (U-128)` (reference src/ColorConversion.cu:30-35) is
 * the one place of the path where the reference's result depends on how nvcc contracted the expression AND no golden of the reference decides it (DESIGN.md
 * section 2; 36 of the 2^24 (Y, U, V) triples differ by one in G between the variants, R and B never):
 *   0  fma(-0.813, V-128, -(0.391 (U-128)))   the LLVM fadd -> fma rule that the resize goldens pin, applied here (the default since 0.3.0)
 *   1  (-0.813 (V-128)) - (0.391 (U-128))     plain IEEE, both products rounded (the library's output until 0.2.x)
 *   2  fma(-0.391, U-128, -0.813 (V-128))     the right-hand product fused
 * for whoever holds goldens of the real reference binary (tools/ref_capture/ produces them on an NVIDIA box).  Same speed; every kernel honours it. */
#define TSVPP_OPT_COLOR_G_TERM 2
/* TSVPP_OPT_UNSAFE_COEFFS (default 0): tsvpp_set_coeffs refuses (TSVPP_UNSUPPORTED) a block that differs from tsvpp_default_coeffs by a single bit unless this is
 * set -- the library's parity statements are about the reference's literals. */
#define TSVPP_OPT_UNSAFE_COEFFS 3
#define TSVPP_HAVE_OPTIONS 1
/* Threads.  tsvpp_set_option, tsvpp_get_option and tsvpp_enable_markers may be called while other threads convert through the same context: every option is
 * read and written atomically, and a conversion that runs beside the call uses the old value or the new one, whole -- never a launch remembered from the old
 * value after the call has returned to a thread that then converts.  What the OPTION promises is still the caller's to keep: a conversion that may see
 * TSVPP_OPT_INPUTS_READY set must meet its conditions (1) and (2).  tsvpp_set_coeffs is different, see there. */
int tsvpp_set_option(tsvpp_ctx *ctx, int option, int value);
int tsvpp_get_option(const tsvpp_ctx *ctx, int option, int *value);

/* Colour constants: read the active block, replace it (e.g. with the block received
 * from rank 0), restore the defaults.  tsvpp_set_coeffs accepts only the default block (bit for bit) unless
 * TSVPP_OPT_UNSAFE_COEFFS is set: TSVPP_UNSUPPORTED otherwise.
 * tsvpp_set_coeffs needs a QUIESCENT context: no conversion, tsvpp_prepare* or tsvpp_get_coeffs of this context may run on another thread
 * during the call -- the block is eight floats that launches copy as they are, not an atomic value.  Set it once, after tsvpp_create (the multi-GPU broadcast
 * does), or between two points where the caller has joined its converting threads. */
int tsvpp_get_coeffs(const tsvpp_ctx *ctx, tsvpp_coeffs *out);
int tsvpp_set_coeffs(tsvpp_ctx *ctx, const tsvpp_coeffs *in);
void tsvpp_default_coeffs(tsvpp_coeffs *out);

/* AREA (down-scale) weight table of generateResizePattern (reference
 * src/Resize.cu:359-386) as this library builds it: writes rows*taps floats
 * (taps = ceil(scale)) to `out` if it fits `max_floats`; returns rows or <0. */
int tsvpp_area_pattern(float scale, float *out, int max_floats, int *taps);
/* DEBUG ONLY (tests): the number of AREA tables the context has cached so far -- one per distinct scale tsvpp_convert* has seen, plus the divisor tables per
 * pair of scales; they stay until tsvpp_destroy.  tsvpp_convert_rois_area never adds one.  TSVPP_ERROR for a null context. */
int tsvpp_debug_area_tables(tsvpp_ctx *ctx);

/* What tsvpp_convert_batch WOULD launch for this request -- stage selection (reference
 * src/VideoProcessor.cpp:106-151) plus this library's kernel / workgroup-shape / LDS choice -- as one line of
 * key=value text, e.g. "mode=bilinear out=f32_planar ... kernel=vpp_bilinear_kernel<...> shape=32x8 rpt=2 ...".
 * Needs no context and no GPU (host logic only; TSVPP_* knobs are honoured).  `aligned_outputs`: outputs are 16-byte
 * aligned.  tail= says how an output 4 k + 2 columns wide ends its rows: 2 = the launch's last tile column is shifted to the
 * frame's right edge (one launch), 1 = a second, element-wise launch converts the two-column row tail, 0 = neither is needed.
 * Returns TSVPP_OK or the status tsvpp_convert would return for the request. */
int tsvpp_describe(const tsvpp_params *p, int in_width, int in_height, int pitch_y, int pitch_uv, int n_frames, int aligned_outputs, char *buf,
                   size_t buf_len);
/* (describe, continued) nt= is the store variant of the launch (0 plain stores, 1 / 2 non-temporal, + 4: the 4-byte uint8
 * stores non-temporal too), staged= says that the launch stages its source through LDS (for the colour-only kernel: that
 * its dword-aligned fast path is taken), in4= that every plane pointer and both pitches are multiples of 4 (frame
 * pointers assumed 256-byte aligned). */

/* DEBUG ONLY (tests): what the calling thread's last tsvpp_convert / tsvpp_convert_batch / tsvpp_convert_table actually
 * launched -- a replayed launch included -- in tsvpp_describe's format (src= / dst= are the launch's; lds= is the
 * dynamic LDS only).  Answers only when TSVPP_DEBUG_KNOBS=1 is set now (else TSVPP_UNSUPPORTED).  TSVPP_ERROR when the
 * thread's last conversion recorded nothing: it ran in a context created without TSVPP_DEBUG_KNOBS=1, it failed, or
 * the thread has converted nothing.  A record of an earlier conversion is never reported. */
int tsvpp_debug_last_launch(char *buf, size_t buf_len);

/* Human-readable text for a status returned by this library. */
const char *tsvpp_strerror(int status);
/* "tsvpp <version> gfx950" */
const char *tsvpp_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TSVPP_H */
