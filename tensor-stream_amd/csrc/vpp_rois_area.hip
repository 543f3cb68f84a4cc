// vpp_rois_area.hip -- AREA resize for regions of interest (tsvpp_convert_rois_area, include/tsvpp.h): vpp_rois.hip's launch -- one 32 x 32 output tile of one box
// per workgroup, the per-box record read with scalar loads out of the kernarg segment, the colour back end of the library -- with AREA's two rules chosen per box
// (roi_area_mode, a wave-uniform branch on the record): the 2x2 blend (areaup_axis) through the shared M_AREA_UP samplers, and the weighted box of the down-scale.
//
// The down-scale needs, per axis, the weight rows of the output indices the tile holds.  tsvpp_convert keeps them as a device table per distinct scale (an
// allocation and a synchronous copy the first time a scale is seen); boxes behind a detector have a new scale each, so this kernel GENERATES its rows instead:
// roi_area_step (vpp_rois.h) runs the float operations of build_area_rows one output index at a time, wrapping where the pattern closes.  The recurrence is serial
// in the output index (the carry of index j depends on every row before it), so one lane walks indices 0 .. j_last of the x axis while its neighbour lane walks
// 0 .. i_last of the y axis in the same instructions, and stores the row RECORDS (lead fraction, number of ones, tail fraction: 12 bytes) of the tile's luma indices
// [first, last] and chroma indices [first >> 1, last >> 1] in LDS (two different ranges; a shifted last tile column starts at an index that is no multiple of 32).
// The two lanes belong to the workgroup's SECOND wave: the first wave goes straight to staging the tile's source footprint (stage_planes, which does not depend on
// the rows), so its loads are in flight while the chains run, as are those of the other workgroups of the CU.  A barrier; 98 lanes expand one record each into its
// row of `taps` floats; a second barrier (down-scale boxes only); then every lane samples out of LDS -- footprint bytes and weight rows -- in the reference's
// order (sample_luma<M_AREA_DOWN>, vpp_device.h): wgt = px[b] * wy rounded, div = div + wgt (the running divisor: no divisor table), sum = fma(data, wgt, sum),
// one division, truncation.  Taps past the box (zero padding of a row) are fetched clamped into the box, as GlobalSrc does: never outside the frame's planes.
// A tile whose footprint does not fit the launch's LDS gathers from global memory; the weight rows always fit (ROI_AREA_MAX_TAPS: at most 17 272 bytes, 16.9 KiB).
//
// What was tried (profiles/rois_area_ab.txt holds the figures of both variants, the BILINEAR launch on the same boxes and the host timing quoted below):
//   1. the chain as build_area_rows is written -- its `while (left - 1 > 0)` loop, every row entry stored by the chain lane itself: ~80 instructions and ~20
//      branches per index on a single lane, ~330 ns per index; 64 boxes to 224 x 224: 99 us, 6.3 x the BILINEAR launch.
//   2. this file: the exact subtractions of that loop collapsed (vpp_rois.h), the step branch-free (~36 instructions, ~75 ns per index), the chain lane stores
//      12-byte records and the rows are expanded by 98 lanes in parallel: 64 boxes to 224 x 224 in 52 us, to 112 x 112 in 36 us -- 3.3 x the BILINEAR launch,
//      still above the factor of two at which the issue asks for the next variant.
// Not built: the host computing each box's carries at tile boundaries.  That is dst_w + dst_h generator steps per box on the host at 7-9 ns each (measured),
// ~225 us per 64 boxes at 224 x 224, more than the launch of variant 2 takes, and a larger record (fewer boxes per launch).
// Cost to know about: the chain is linear in the output size and runs once per tile -- ~17 us in front of the last tile column of a 224-wide output, ~80 us at
// 1024, ~5 ms at the accepted maximum of 65536 (extrapolated from the per-index figure; not measured beyond 224).  The entry point is for NN-input sizes.
//
// Arithmetic contract as everywhere: single IEEE-754 operations in the reference's order, contraction off.  Written for wave64 / CDNA4 only.

#include "vpp_rois_area_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

// (the kernel: vpp_rois_area_core.h, shared with vpp_rois_area_tensor.hip)

hipError_t launch_rois_area(OutKind out, bool vec, bool staged, const RoiLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name, size_t name_len,
                            bool dry_run) {
    if (!tile_flavour(out)) return hipErrorNotSupported;
    if (name && name_len) snprintf(name, name_len, "vpp_rois_area<%s,%s,%s>", kOutNames[out], vec_name(vec), staged_name(staged));
    if (dry_run) return hipSuccess;
    return with_tile_flavour(out, [&](auto O) {
        return with_vec_staged(vec, staged, [&](auto V, auto S) { // (lds_bytes either way: the weight rows need LDS in the gather kernel too)
            hipLaunchKernelGGL((vpp_rois_area_kernel<decltype(O)::value, decltype(V)::value, decltype(S)::value>), dim3(grid), dim3(ROI_THREADS), lds_bytes, stream, L);
            return hipGetLastError();
        });
    });
}

} // namespace tsvpp
