// vpp_remap.hip -- per-pixel coordinate maps: every output samples its frame BILINEAR where a device-resident map says, in one launch (tsvpp_convert_remap,
// include/tsvpp.h).
//
// The output side is tsvpp_convert_warp's: every output is dst_w x dst_h, a workgroup finds its (output, tile) with one division and stores its tile through the
// library's colour back end.  What differs per output -- planes, pitches, frame size, map address and pitch, output pointer -- is a 56-byte record indexed by the
// workgroup's output: wave-uniform, read with scalar loads out of the kernarg segment.
//
// Source side: the coordinate of an output pixel is READ from the map, so no one but the kernel knows a tile's footprint -- the host plans nothing per tile.  Each
// thread loads the eight entries of its thread tile, clamps them, and the workgroup reduces the extremes of the clamped coordinates on both grids (cross-lane
// within a wave, a few LDS words across the two waves): floor(min) .. floor(max) + 1, clamped into the frame, is the bounding box of every tap (remap_footprint,
// vpp_remap.h -- the function the host evaluates for the tests and for the LDS hint).  A box that fits the launch's LDS is staged with 16-byte loads
// (stage_planes) and sampled through LdsSrc; one that does not -- a map that folds the frame into a tile, garbage -- gathers its taps from global memory
// (GlobalSrc), a wave-uniform branch.  BORDER is a template parameter: the replicate kernels carry no compare and no select.
//
// Arithmetic contract as everywhere: single IEEE-754 operations, contraction off; the only fused operations are the chroma coordinate's (vpp_remap.h) and
// bilerp's.  Written for wave64 / CDNA4 only.

#include "vpp_remap_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

// (the kernel and its tag: vpp_remap_core.h, shared with vpp_remap_tensor.hip; the launcher: vpp_tile_launch.h)
hipError_t launch_remap(OutKind out, bool vec, bool staged, bool border, const RemapLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                        size_t name_len, bool dry_run) {
    return launch_coord<RemapKernels>(out, vec, staged, border, L, grid, lds_bytes, stream, name, name_len, dry_run);
}

} // namespace tsvpp
