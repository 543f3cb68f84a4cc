// vpp_warp_core.h -- the affine-warp kernel itself (see vpp_warp.hip for what it does), as a template that two translation units instantiate: vpp_warp.hip with the
// library's colour back end (EL_LIB: every flavour of tsvpp_convert_warp) and vpp_warp_tensor.hip with the tensor store (EL_F32 / EL_HALF:
// tsvpp_convert_warp_tensor, vpp_tensor_store.h).  Nothing but the store call differs between them: a border sample goes through whichever it is, like every other.
//
// The sampler, and the two things weighed for it:
//   - Row-incremental coordinates (fx of column j + 1 from column j by one addition) are NOT used: the contract's coordinate is fmaf(u, m0, fmaf(v, m1, tx)),
//     rounded twice, and a running sum has other bits.  Every pixel evaluates the contract's expression.
//   - The inner fmaf(v, m1, tx) / fmaf(v, m4, ty) depends on the row only: a thread tile evaluates it once per row (2 + 2 instead of 8 + 8), then one fmaf per
//     pixel and axis.  The two rows of a thread tile differ only in v.  The chroma pairs have their own coordinates on the pair grid (ctx / cty), never derived
//     from the luma ones.
#pragma once
#include "vpp_tile_core.h"
#include "vpp_warp.h"

#pragma clang fp contract(off)

namespace tsvpp {

// One luma sample at source coordinate (fx, fy): the four taps through the library's bilerp, or the border sample
template <bool BORDER, class S> __device__ __forceinline__ float warp_luma(const S &s, float fx, float fy, float border) {
    int x, x2, y, y2;
    float wx, wy;
    warp_axis(fx, s.w, x, x2, wx);
    warp_axis(fy, s.h, y, y2, wy);
    const float v = (float)(bilerp(s.Y(y, x), s.Y(y, x2), s.Y(y2, x), s.Y(y2, x2), wx, wy) & 0xff);
    if constexpr (BORDER) return (warp_outside(fx, s.w) || warp_outside(fy, s.h)) ? border : v;
    else return v;
}
// One chroma pair at pair-grid coordinate (fx, fy): U and V from byte columns 2 p and 2 p + 1
template <bool BORDER, class S> __device__ __forceinline__ void warp_chroma(const S &s, float fx, float fy, float border_u, float border_v, float &U, float &V) {
    const int cw = s.w >> 1, ch = s.h >> 1;
    int x, x2, y, y2;
    float wx, wy;
    warp_axis(fx, cw, x, x2, wx);
    warp_axis(fy, ch, y, y2, wy);
    U = (float)(bilerp(s.UV(y, 2 * x), s.UV(y, 2 * x2), s.UV(y2, 2 * x), s.UV(y2, 2 * x2), wx, wy) & 0xff);
    V = (float)(bilerp(s.UV(y, 2 * x + 1), s.UV(y, 2 * x2 + 1), s.UV(y2, 2 * x + 1), s.UV(y2, 2 * x2 + 1), wx, wy) & 0xff);
    if constexpr (BORDER) {
        const bool outside = warp_outside(fx, cw) || warp_outside(fy, ch);
        U = outside ? border_u : U;
        V = outside ? border_v : V;
    }
}

// convert_thread_tile (vpp_device.h) with the warp's sampler: 2 x 4 luma samples and 2 chroma pairs of the virtual NV12 frame, then the one colour back end
template <int OUT, bool VEC, bool BORDER, int EL, class S>
__device__ __forceinline__ void warp_thread_tile(const S &s, const LaunchDesc &d, const WarpRec &r, const WarpLaunch &L, typename OutT<OUT>::type *out, int i0, int j0) {
    // VEC: the thread tile has its four columns.  Element-wise flavour: 2 or 4; a column that does not exist is sampled at the row's last one and never stored.
    const int ncol = VEC ? PXW : min(PXW, d.dst_w - j0);
    const int ci = i0 >> 1, cj0 = j0 >> 1, jmax = d.dst_w - 1, cjmax = (d.dst_w >> 1) - 1;
    float Uf[2] = { 128.0f, 128.0f }, Vf[2] = { 128.0f, 128.0f }, Yf[PXH][PXW];
    if constexpr (!kLumaOnly<OUT>) {
        const float v = (float)ci + 0.5f;
        const float ax = warp_inner(v, r.m1, r.ctx), ay = warp_inner(v, r.m4, r.cty);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const float u = (float)(VEC ? cj0 + c : min(cj0 + c, cjmax)) + 0.5f;
            warp_chroma<BORDER>(s, warp_coord(u, r.m0, ax), warp_coord(u, r.m3, ay), L.border_u, L.border_v, Uf[c], Vf[c]);
        }
    }
#pragma unroll
    for (int rr = 0; rr < PXH; rr++) {
        // the chroma pairs, then one luma row at a time: with every tap of the thread tile in flight at once (48 byte loads, each with its own address) the
        // kernels took up to 142 VGPRs; a row's 16 taps are consumed before the next row's are issued
        __builtin_amdgcn_sched_barrier(0);
        const float v = (float)(i0 + rr) + 0.5f;
        const float ax = warp_inner(v, r.m1, r.tx), ay = warp_inner(v, r.m4, r.ty);
#pragma unroll
        for (int c = 0; c < PXW; c++) {
            const float u = (float)(VEC ? j0 + c : min(j0 + c, jmax)) + 0.5f;
            Yf[rr][c] = warp_luma<BORDER>(s, warp_coord(u, r.m0, ax), warp_coord(u, r.m3, ay), L.border_y);
        }
    }
    store_tile<OUT, VEC, EL>(Yf, Uf, Vf, d, L.spec, out, i0, j0, ncol);
}

// (launch bounds: at least four waves per SIMD, i.e. at most 128 VGPRs -- four workgroups of the 40 KiB LDS budget per CU.  With the rows fenced as above no
// instantiation spills: profiles/warp_resources.txt)
// This function and vpp_persp_kernel (vpp_persp_core.h) read alike and stay TWO functions.  As one kernel template over the thread-tile function -- and as one
// over all four coordinate paths -- the compiler emitted other code: about 830 fewer instruction lines in each colour unit and about 900 lines with another
// opcode (cross-compiled for gfx950 and diffed, never measured on a device: profiles/coord_paths_resources.txt).  Not to be tried again without a GPU to
// measure on; the coordinate-map and control-grid kernels did fold into one (vpp_remap_core.h).
template <int OUT, bool VEC, bool STAGED, bool BORDER, int EL = EL_LIB>
__global__ __launch_bounds__(ROI_THREADS, 4) void vpp_warp_kernel(const WarpLaunch L) {
    using T = typename OutT<OUT>::type;
    typedef __attribute__((address_space(1))) uint8_t *GP; // the records hold GLOBAL addresses (PtrCol, vpp_kernels.h)
    // workgroup -> (warp, tile): all tiles of an output are neighbours in the grid, so the lines that adjacent tiles share meet in L2
    const TileIndex tix = tile_index(L.tiles_x, L.tiles_y);
    const int item = tix.item, tyi = tix.tyi, txi = tix.txi;
    if (item >= L.n) return;
    const WarpRec &r = L.r[item]; // wave-uniform index: scalar loads

    // the colour back end and the staging loop read their request from a LaunchDesc (the samplers' fields -- ratios, weights -- stay zero: the warp has its own)
    LaunchDesc d = {};
    d.src_w = r.src_w;
    d.src_h = r.src_h;
    d.pitch_y = r.pitch_y;
    d.pitch_uv = r.pitch_uv;
    d.dst_w = L.dst_w;
    d.dst_h = L.dst_h;
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

    const uint8_t *const plane_y = (const uint8_t *)(GP)(uintptr_t)r.y, *const plane_uv = (const uint8_t *)(GP)(uintptr_t)r.uv;
    T *const out = (T *)(GP)(uintptr_t)r.out;
    const int lx = threadIdx.x & (ROI_TX - 1), ly = threadIdx.x >> ROI_TX_SHIFT;
    const int j_first = roi_tile_col0(txi, L.dst_w, d.last_col0), i_first = tyi * ROI_TILE_H;
    const int j0 = j_first + lx * PXW, i0 = i_first + ly * PXH;
    const bool active = j0 < L.dst_w && i0 < L.dst_h && !(VEC && is_row_tail(d, j0));

    if constexpr (STAGED) {
        // the tile's source bounding box, from the coordinates of its four corner pixels (warp_footprint: the numbers the host sized the launch's LDS with)
        RoiFootprint f;
        warp_footprint(r, j_first, tile_last(j_first, ROI_TILE_W, L.dst_w), i_first, tile_last(i_first, ROI_TILE_H, L.dst_h), f);
        if (roi_stageable(f) && roi_lds_need(f, kLumaOnly<OUT>) <= L.lds_bytes) { // (wave-uniform)
            const int span_y = f.xhi - f.xlo + 1, span_uv = 2 * (f.cxhi - f.cxlo + 1);
            const int ny = f.yhi - f.ylo + 1, nuv = kLumaOnly<OUT> ? 0 : f.cyhi - f.cylo + 1;
            d.lds_cpr_y = roi_chunks(span_y);
            d.lds_cpr_uv = roi_chunks(span_uv);
            d.lds_slot_y = 32 - __builtin_clz(((unsigned)d.lds_cpr_y - 1u) | 1u); // log2 of the lanes that serve one staged row (>= chunks per row)
            d.lds_slot_uv = 32 - __builtin_clz(((unsigned)d.lds_cpr_uv - 1u) | 1u);
            uint8_t *lds_y = lds_raw, *lds_uv = lds_raw + ny * d.lds_cpr_y * 16;
            const uint8_t *ay, *auv;
            LdsSrc s;
            s.py_ = describe_plane(lds_y, plane_y, r.pitch_y, f.ylo, f.xlo, d.lds_cpr_y, ay);
            s.puv_ = describe_plane(lds_uv, plane_uv, r.pitch_uv, f.cylo, 2 * f.cxlo, d.lds_cpr_uv, auv);
            s.w = r.src_w;
            s.h = r.src_h;
            stage_planes<2, 1>(d, lds_y, ay, s.py_, ny, span_y, lds_uv, auv, s.puv_, nuv, span_uv, ROI_THREADS); // (in flight per lane: as measured for vpp_rois.hip)
            __syncthreads();
            if (active) warp_thread_tile<OUT, VEC, BORDER, EL>(s, d, r, L, out, i0, j0);
            return;
        }
    }
    if (!active) return;
    GlobalSrc s;
    tile_global_src(s, r, plane_y, plane_uv);
    warp_thread_tile<OUT, VEC, BORDER, EL>(s, d, r, L, out, i0, j0);
}

// The path's tag for launch_coord / launch_coord_tensor (vpp_tile_launch.h)
struct WarpKernels {
    using Launch = WarpLaunch;
    static constexpr const char *kName = "vpp_warp";
    template <int OUT, bool VEC, bool STAGED, bool BORDER, int EL> static constexpr auto kernel() { return &vpp_warp_kernel<OUT, VEC, STAGED, BORDER, EL>; }
};

} // namespace tsvpp
