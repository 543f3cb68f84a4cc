// vpp_letterbox.hip -- n frames, each resized with its aspect kept into an inner rectangle of ONE canvas size, the rest of the canvas filled with a constant, in one
// launch (tsvpp_convert_letterbox, include/tsvpp.h).
//
// The grid runs over the CANVAS: a workgroup finds its (frame, canvas tile) with one division, and LaunchDesc::dst_w / dst_h are the canvas, so a tile goes out
// through the library's colour back end unchanged (color_store_tile: vector stores for 16-byte aligned outputs, element-wise stores otherwise, the shifted last
// tile column for widths 4 k + 2).  What differs per frame -- planes, pitches, size, ratios, rectangle, canvas pointer -- is a 64-byte record indexed by the
// workgroup's frame: wave-uniform, read with scalar loads out of the kernarg segment.
//
// Every field of the rectangle is even.  A thread tile is 2 rows x 4 columns at an even origin, so its two rows are both inside the rectangle or both outside, and
// each of its two 2-column chroma pairs is wholly in or out: canvas pixel (i, j) inside the rectangle is inner pixel (i - top, j - left), canvas pair (i >> 1,
// j >> 1) is inner pair ((i - top) >> 1, (j - left) >> 1).  The thread tile samples at those inner coordinates -- clamped into the part of the rectangle its
// workgroup's tile covers, so every access stays inside the staged footprint whatever the lane -- and then selects, per pair, between the samples and the pad
// sample before the one call of the colour back end: the pad runs through the same colour arithmetic as every sample, in every flavour.
//
// Source side: the ROI kernel's (vpp_rois.hip).  The footprint of the part of the tile inside the rectangle is staged in LDS with 16-byte loads (stage_planes) and
// sampled through LdsSrc; a tile whose footprint does not fit the launch's LDS gathers from global memory (GlobalSrc), a wave-uniform branch; a tile that does not
// touch the rectangle stages nothing, samples nothing and stores pad.
//
// Arithmetic contract as everywhere: single IEEE-754 operations in the reference's order, contraction off; the only fused operations are the explicit ones of the
// shared samplers.  Written for wave64 / CDNA4 only.

#include "vpp_letterbox_core.h"

#pragma clang fp contract(off)

namespace tsvpp {

// (the kernel: vpp_letterbox_core.h, shared with vpp_letterbox_tensor.hip)

namespace {

const char *const kModeNames[M_COUNT] = { "M_NONE", "M_NEAREST", "M_BILINEAR", "M_BICUBIC", "M_AREA_DOWN", "M_AREA_UP" };
const char *const kOutNames[O_COUNT] = { "O_U8_PLANAR", "O_U8_MERGED", "O_F32_PLANAR", "O_F32_MERGED", "O_NV12_U8", "O_NV12_F32", "O_Y800_U8", "O_Y800_F32", "O_HSV_F32" };

template <int MODE, int OUT, bool VEC, bool STAGED>
hipError_t launch_k(const LbLaunch &L, unsigned grid, size_t lds, hipStream_t stream) {
    hipLaunchKernelGGL((vpp_letterbox_kernel<MODE, OUT, VEC, STAGED>), dim3(grid), dim3(ROI_THREADS), lds, stream, L);
    return hipGetLastError();
}
template <int MODE, int OUT>
hipError_t launch_mo(bool vec, bool staged, const LbLaunch &L, unsigned grid, size_t lds, hipStream_t stream) {
    if (vec) return staged ? launch_k<MODE, OUT, true, true>(L, grid, lds, stream) : launch_k<MODE, OUT, true, false>(L, grid, 0, stream);
    return staged ? launch_k<MODE, OUT, false, true>(L, grid, lds, stream) : launch_k<MODE, OUT, false, false>(L, grid, 0, stream);
}
// the flavours this kernel is instantiated for: RGB / BGR planar and merged, Y800
constexpr bool lb_flavour(int out) { return out == O_U8_PLANAR || out == O_U8_MERGED || out == O_F32_PLANAR || out == O_F32_MERGED || out == O_Y800_U8 || out == O_Y800_F32; }
template <int MODE>
hipError_t launch_m(OutKind out, bool vec, bool staged, const LbLaunch &L, unsigned grid, size_t lds, hipStream_t stream) {
    return with_out_kind(out, [&](auto O) {
        constexpr int OUT = decltype(O)::value;
        if constexpr (lb_flavour(OUT)) return launch_mo<MODE, OUT>(vec, staged, L, grid, lds, stream);
        else return hipErrorNotSupported; // a missing kernel is an error, never a fallback
    });
}

} // namespace

hipError_t launch_letterbox(Mode mode, OutKind out, bool vec, bool staged, const LbLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                            size_t name_len, bool dry_run) {
    const bool known = (mode == M_NEAREST || mode == M_BILINEAR || mode == M_BICUBIC) && lb_flavour(out);
    if (!known) return hipErrorNotSupported;
    if (name && name_len) snprintf(name, name_len, "vpp_letterbox<%s,%s,%s,%s>", kModeNames[mode], kOutNames[out], vec ? "vec" : "elem", staged ? "staged" : "gather");
    if (dry_run) return hipSuccess;
    switch (mode) {
    case M_NEAREST: return launch_m<M_NEAREST>(out, vec, staged, L, grid, lds_bytes, stream);
    case M_BILINEAR: return launch_m<M_BILINEAR>(out, vec, staged, L, grid, lds_bytes, stream);
    default: return launch_m<M_BICUBIC>(out, vec, staged, L, grid, lds_bytes, stream);
    }
}

} // namespace tsvpp
