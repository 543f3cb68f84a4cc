// vpp_rois_sized.h -- launch block and workgroup lookup of the region-of-interest kernel with PER-BOX output sizes (vpp_rois_sized.hip), shared with the host API
// (tsvpp_rois_sized.cpp: tsvpp_convert_rois_sized / tsvpp_describe_rois_sized, their tensor forms and tsvpp_rois_sized_tile).  The source side -- footprints,
// staging, tile geometry of one box -- is vpp_rois.h's, unchanged.  Product code -- never includes anything from oracle/.
#pragma once
#include "vpp_rois.h"

#pragma clang fp contract(off)

namespace tsvpp {

// What differs per box: RoiRec's 48 bytes, then the output side that vpp_rois_kernel takes from its launch.  Wave-uniform: indexed with the workgroup's box, read
// with scalar loads out of the kernarg segment.
struct SizedRec {
    uint64_t y, uv, out;       // as RoiRec's
    int32_t pitch_y, pitch_uv;
    int32_t src_w, src_h;
    float xr, yr;              // (float)src_w / dst_w, (float)src_h / dst_h with THIS box's output size
    int32_t dst_w, dst_h;      // the box's output
    int32_t tiles_x;           // ceil(dst_w / ROI_TILE_W)
    int32_t tile0;             // the box's first workgroup in its launch: tile_end of the box before it (0 for the first)
};
static_assert(sizeof(SizedRec) == 64, "SizedRec layout");

// One launch: up to TSVPP_MAX_ROIS_SIZED boxes, by value in the kernarg segment (3.3 KiB; HIP's hidden arguments take up to 256 bytes of the segment's 4 KiB).
struct SizedLaunch {
    int32_t swap_rb, color_g;
    tsvpp_coeffs k;
    int32_t n_rois;
    int32_t nt_stores, u8_xchg;               // as LaunchDesc's
    int32_t lds_bytes;                        // as RoiLaunch's: a tile whose footprint needs more gathers from global memory
    uint32_t tile_end[TSVPP_MAX_ROIS_SIZED];  // ascending: workgroups [tile_end[b - 1], tile_end[b]) are box b's tiles, row-major; entries from n_rois on are
                                              // 0xffffffff (no workgroup index reaches them).  tile_end[n_rois - 1] is the grid
    SizedRec r[TSVPP_MAX_ROIS_SIZED];
    tsvpp_tensor_spec spec;                   // the tensor instantiations', as RoiLaunch's
};
static_assert(sizeof(SizedLaunch) + 256 <= 4096, "SizedLaunch no longer fits the kernarg segment");

// The shifted last tile column of THIS box (tile_col0, vpp_device.h), as tile_fill (tsvpp_tiles.h) decides it per launch: outputs 4 k + 2 columns wide and at
// least a tile wide, vector stores only
__host__ __device__ inline int sized_last_col0(bool vec, int dst_w) { return (vec && (dst_w & 3) != 0 && dst_w >= ROI_TILE_W) ? dst_w - ROI_TILE_W : 0; }

// workgroup -> (box, tile column, tile row).  ONE function for the kernel and for tsvpp_rois_sized_tile (tests/test_rois_sized_cpu.py walks every workgroup of
// seeded requests through it).  It reads `wg` (blockIdx.x) and kernel arguments only: wave-uniform, so the compiler keeps it on the scalar side.  The box is the
// number of tile_end[] entries <= wg -- 48 independent compares over three 16-dword scalar loads, no chain of dependent loads (a binary search over the records
// has six); then one division by the box's tiles_x.  All tiles of a box are neighbours in the grid and row-major, as in vpp_rois_kernel: adjacent tiles share
// lines in L2.  The caller guarantees wg < tile_end[n_rois - 1], the launch's grid.
struct SizedTile {
    int box, txi, tyi;
};
__host__ __device__ __forceinline__ SizedTile sized_tile(const SizedLaunch &L, unsigned wg) {
    SizedTile t;
    int box = 0;
#pragma unroll
    for (int i = 0; i < TSVPP_MAX_ROIS_SIZED; i++) box = L.tile_end[i] <= wg ? i + 1 : box; // (ascending: the last entry at or below wg is their count)
    t.box = box;
    const SizedRec &r = L.r[box];
    const int rem = (int)(wg - (unsigned)r.tile0);
    t.tyi = rem / r.tiles_x;
    t.txi = rem - t.tyi * r.tiles_x;
    return t;
}

// (vpp_rois_sized.hip) launches -- or, with `dry_run`, only names -- the kernel of (mode, out, vec, staged); `name` receives the name tsvpp_describe_rois_sized reports
hipError_t launch_rois_sized(Mode mode, OutKind out, bool vec, bool staged, const SizedLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                             size_t name_len, bool dry_run);
// (vpp_rois_sized_tensor.hip) the same for the tensor instantiations: `out` is O_F32_PLANAR or O_Y800_F32, the element is L.spec.dtype's
hipError_t launch_rois_sized_tensor(Mode mode, OutKind out, bool vec, bool staged, const SizedLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream,
                                    char *name, size_t name_len, bool dry_run);

} // namespace tsvpp
