// vpp_warp.hip -- rotated and affine-warped boxes, each sampled BILINEAR into ONE output size, in one launch (tsvpp_convert_warp, include/tsvpp.h).
//
// The output side is tsvpp_convert_rois's: every warp becomes dst_w x dst_h, a workgroup finds its (warp, output tile) with one division and stores its tile through
// the library's colour back end.  What differs per warp -- planes, pitches, frame size, the 2 x 2 linear part and the four translations, output pointer -- is a
// 72-byte record indexed by the workgroup's warp: wave-uniform, read with scalar loads out of the kernarg segment.
//
// Source side: the coordinate of an output pixel depends on both of its indices, fx = fmaf(u, m0, fmaf(v, m1, tx)), so a tile's footprint is no product of a
// column span and a row span.  It is the bounding box of the tile's image: every operation of the coordinate is monotone in u and in v, so the extremes over the
// tile are those of its four corner pixels (warp_footprint, vpp_warp.h -- the numbers the host sized the launch's LDS with).  A box that fits the launch's LDS is
// staged with 16-byte loads (stage_planes) and sampled through LdsSrc; one that does not -- a steep down-scale, a large rotated tile -- gathers its taps from
// global memory (GlobalSrc), a wave-uniform branch.  BORDER is a template parameter: the replicate kernels carry no compare and no select.
//
// Arithmetic contract as everywhere: single IEEE-754 operations, contraction off; the only fused operations are the two of the coordinate (vpp_warp.h) and
// bilerp's.  Written for wave64 / CDNA4 only.

#include "vpp_warp_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

// (the kernel and its tag: vpp_warp_core.h, shared with vpp_warp_tensor.hip; the launcher: vpp_tile_launch.h)
hipError_t launch_warp(OutKind out, bool vec, bool staged, bool border, const WarpLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                       size_t name_len, bool dry_run) {
    return launch_coord<WarpKernels>(out, vec, staged, border, L, grid, lds_bytes, stream, name, name_len, dry_run);
}

} // namespace tsvpp
