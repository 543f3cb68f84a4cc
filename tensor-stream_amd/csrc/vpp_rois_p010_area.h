// vpp_rois_p010_area.h -- what the P010 AREA region-of-interest kernel (vpp_rois_p010_area.hip, vpp_rois_p010_area_tensor.hip) shares with the host API
// (tsvpp_rois_p010_area.cpp: tsvpp_convert_rois_p010_area / tsvpp_describe_rois_p010_area).  The launch block is the P010 ROI call's RoiLaunch (plane addresses
// advanced to the box origin, pitches in BYTES, the box's size in samples; xr / yr are not read: N and n suffice) with the band walk's two numbers behind it, as LbBoxLaunch.
// Product code -- never includes anything from oracle/.
#pragma once
#include "vpp_box_p010.h"
#include "vpp_rois_p010.h"

namespace tsvpp {

// One band height per launch, the widest tile's.  A launch mixes a 40-pixel box with a 1500-pixel one, and a height per TILE -- each workgroup deriving what its
// own footprint width buys from the launch's byte budget, narrow tiles walking in 32-row bands beside wide ones -- was built and measured: 64 boxes of 40 .. 80
// and 1000 .. 1500 pixels to 96 x 96 took 166.6 us against 158.4 us with the launch's height, outside the blocks' spread of 0.7 us, and two other rows tied
// (profiles/rois_p010_area_ab.txt).  A taller band is not a better one: the first band's load overlaps nothing.  So the launch-wide form stays.
struct RoiBoxLaunch : RoiLaunch {
    int32_t band;     // source rows per band (vpp_box_p010.h), 1 .. BOX_BAND_MAX_ROWS; 0: not even one row of the widest tile fits the budget -- never launched
    int32_t band_cpr; // 16-byte chunks per staged row the band buffers are sized for: the widest footprint row of the launch's tiles, either plane
};
static_assert(sizeof(RoiBoxLaunch) + 256 <= 4096, "RoiBoxLaunch no longer fits the kernarg segment");

// The band height `budget` bytes buy at `cpr` chunks per row: box_band_rows, or 0 where not even one-row bands fit
inline int roi_box_band(int budget, int cpr) {
    const int rows = box_band_rows(budget, cpr);
    return box_band_lds(rows, cpr) <= budget ? rows : 0;
}
// chunks per staged row of output columns [j0, j1] of a box W wide into an output w wide: luma words, chroma (U, V) word pairs.  The footprint is exact and
// lies inside the BOX's plane
__host__ __device__ inline int roi_box_cpr_y(int j0, int j1, int W, int w) {
    int lo, hi;
    box_span(j0, j1, W, w, lo, hi);
    return roi_chunks(2 * (hi - lo + 1));
}
__host__ __device__ inline int roi_box_cpr_uv(int j0, int j1, int W, int w) {
    int lo, hi;
    box_span(j0 >> 1, j1 >> 1, W >> 1, w >> 1, lo, hi);
    return roi_chunks(4 * (hi - lo + 1));
}
// The widest footprint row the limits allow, in chunks.  Luma: a tile's 32 output columns of at most BOX_P010_MAX_TAPS = 17 taps each (an exact ratio of 17 has
// them all, and shares none) -- 17 x 32 = 544 words = 1088 bytes, roi_chunks = 69.  Chroma: 16 pairs alike -- 17 x 16 = 272 pairs of 4 bytes = 1088 bytes, 69
// chunks as well.  One-row bands of it: 128 bytes of row means + 2 buffers x 16 x 128 slots (69 rounded up to the DMA loop's 64) = 4224 bytes, so the default
// 40 KiB budget behind at most 12 KiB of the store side's static slabs refuses no request within the limits.
constexpr int ROI_BOX_MAX_CPR = ((2 * ROI_TILE_W * BOX_P010_MAX_TAPS + 14) >> 4) + 1;
static_assert(ROI_BOX_MAX_CPR == 69 && ((4 * (ROI_TILE_W / 2) * BOX_P010_MAX_TAPS + 14) >> 4) + 1 == 69, "the widest footprint row");

// (vpp_rois_p010_area.hip) launches -- or, with `dry_run`, only names -- the kernel of (out, vec)
hipError_t launch_rois_p010_area(OutKind out, bool vec, const RoiBoxLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name, size_t name_len,
                                 bool dry_run);
// (vpp_rois_p010_area_tensor.hip) the same for the tensor instantiations: `out` is O_F32_PLANAR or O_Y800_F32, the element is L.spec.dtype's
hipError_t launch_rois_p010_area_tensor(OutKind out, bool vec, const RoiBoxLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                        size_t name_len, bool dry_run);

} // namespace tsvpp
