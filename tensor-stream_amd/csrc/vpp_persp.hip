// vpp_persp.hip -- homography-warped outputs, each sampled BILINEAR into ONE output size, in one launch (tsvpp_convert_perspective, include/tsvpp.h).
//
// The output side is tsvpp_convert_warp's: every output is dst_w x dst_h, a workgroup finds its (output, tile) with one division and stores its tile through the
// library's colour back end.  What differs per output -- planes, pitches, frame size, the nine terms of each grid, output pointer -- is a 112-byte record indexed
// by the workgroup's output: wave-uniform, read with scalar loads out of the kernarg segment.
//
// Source side: fx = nx * (1 / nw), fy = ny * (1 / nw) with nx, ny, nw the affine warp's fused multiply-adds (vpp_persp.h).  A quotient of monotone functions is
// not monotone after rounding, so a tile's footprint is no bounding box of corner coordinates: it is the interval box of the numerators' and the reciprocal's
// ranges (persp_footprint -- the numbers the host sized the launch's LDS with), rigorous whatever the matrix and looser than the true box under strong
// perspective.  A box that fits the launch's LDS is staged with 16-byte loads (stage_planes) and sampled through LdsSrc; one that does not gathers its taps from
// global memory (GlobalSrc), a wave-uniform branch.  BORDER is a template parameter: the replicate kernels carry no compare and no select.
//
// Arithmetic contract as everywhere: single IEEE-754 operations, contraction off; the reciprocal is the correctly rounded division 1.0f / nw.  Written for
// wave64 / CDNA4 only.

#include "vpp_persp_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

// (the kernel and its tag: vpp_persp_core.h, shared with vpp_persp_tensor.hip; the launcher: vpp_tile_launch.h)
hipError_t launch_persp(OutKind out, bool vec, bool staged, bool border, const PerspLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                        size_t name_len, bool dry_run) {
    return launch_coord<PerspKernels>(out, vec, staged, border, L, grid, lds_bytes, stream, name, name_len, dry_run);
}

} // namespace tsvpp
