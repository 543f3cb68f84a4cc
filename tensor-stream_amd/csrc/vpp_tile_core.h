// vpp_tile_core.h -- what the three tile kernels share on the device (vpp_rois_core.h, vpp_rois_area_core.h, vpp_letterbox_core.h): one 32 x 32 output tile of one
// item (a box, a frame) per workgroup, the item's record read with scalar loads out of the kernarg segment, the tile's source footprint staged in LDS or gathered
// from global memory, the store through the colour back end or the tensor store.  Every piece is a template over the launch block (RoiLaunch / LbLaunch) or the
// record (RoiRec / LbRec), which share the fields read here, and is forced inline.  A kernel uses a piece only where it compiles to the instructions of the code
// written out in place: profiles/tile_core_resources.txt compares all 280 kernels with the parent's and says which piece stayed inline in which kernel.
#pragma once
#include "vpp_device.h"
#include "vpp_rois.h"
#include "vpp_tensor_store.h"

#pragma clang fp contract(off)

namespace tsvpp {

// workgroup -> (item, tile): all tiles of an item are neighbours in the grid, so the lines that adjacent tiles share meet in L2.  The caller returns where
// `item` is not below the launch's count.
struct TileIndex {
    int item, txi, tyi;
};
__device__ __forceinline__ TileIndex tile_index(int tiles_x, int tiles_y) {
    TileIndex t;
    const int tiles = tiles_x * tiles_y;
    t.item = (int)blockIdx.x / tiles;
    const int rem = (int)blockIdx.x - t.item * tiles;
    t.tyi = rem / tiles_x;
    t.txi = rem - t.tyi * tiles_x;
    return t;
}

// The samplers and the colour back end read their request from a LaunchDesc: this item's source and ratios, the launch's output.  `d` is zero-initialised by the
// caller (returned by value, the descriptor commuted operands in half of the kernels).
template <int OUT, bool VEC, class LAUNCH, class REC> __device__ __forceinline__ void tile_desc(const LAUNCH &L, const REC &r, LaunchDesc &d) {
    d.src_w = r.src_w;
    d.src_h = r.src_h;
    d.pitch_y = r.pitch_y;
    d.pitch_uv = r.pitch_uv;
    d.dst_w = L.dst_w;
    d.dst_h = L.dst_h;
    d.xr = r.xr;
    d.yr = r.yr;
    d.swap_rb = L.swap_rb;
    d.color_g = L.color_g;
    d.k = L.k;
    d.tx = ROI_TX;
    d.ty = ROI_TY;
    d.tx_shift = ROI_TX_SHIFT;
    d.rpt = 1;
    d.nt_stores = L.nt_stores;
    d.last_col0 = VEC ? L.last_col0 : 0;
    d.u8_xchg = L.u8_xchg;
    d.luma_only = kLumaOnly<OUT> ? 1 : 0;
}

// The source of a tile that gathers its taps from global memory
template <class REC> __device__ __forceinline__ void tile_global_src(GlobalSrc &s, const REC &r, const uint8_t *plane_y, const uint8_t *plane_uv) {
    s.y = plane_y;
    s.uv = plane_uv;
    s.py = r.pitch_y;
    s.puv = r.pitch_uv;
    s.w = r.src_w;
    s.h = r.src_h;
}

// What is NOT here although all three kernels spell it out (profiles/tile_core_resources.txt has the figures): the first output column / row of the tile and of the
// lane's thread tile with `active` (as a helper, in four forms, it moved VGPRs in vpp_rois_kernel and vpp_letterbox_kernel), and the staging block from
// d.lds_cpr_y through stage_planes<2, 1> (as a helper it kept every VGPR count but changed the instructions, and the calls measured slower than the parent's).
// vpp_rois_kernel also keeps its descriptor and GlobalSrc fill (two of its kernels compile to other instructions with either helper), vpp_rois_area_kernel its
// index arithmetic (16 of its 24 kernels).

// A thread tile's samples to its output: the library's colour back end (EL_LIB, with the typed pointer) or the tensor store with the launch's spec
template <int OUT, bool VEC, int EL>
__device__ __forceinline__ void store_tile(const float Yf[PXH][PXW], const float Uf[2], const float Vf[2], const LaunchDesc &d, const tsvpp_tensor_spec &a,
                                           typename OutT<OUT>::type *out, int i0, int j0, int ncol) {
    if constexpr (EL == EL_LIB) color_store_tile<OUT, VEC>(Yf, Uf, Vf, d, out, i0, j0, ncol);
    else tensor_store_tile<OUT, EL, VEC>(Yf, Uf, Vf, d, a, (uint8_t *)out, i0, j0, ncol);
}

} // namespace tsvpp
