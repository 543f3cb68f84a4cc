// vpp_persp_core.h -- the perspective-warp kernel itself (see vpp_persp.hip for what it does), as a template that two translation units instantiate:
// vpp_persp.hip with the library's colour back end (EL_LIB: every flavour of tsvpp_convert_perspective) and vpp_persp_tensor.hip with the tensor store (EL_F32 /
// EL_HALF: tsvpp_convert_perspective_tensor, vpp_tensor_store.h).  Nothing but the store call differs between them.
//
// The sampler is the affine warp's (warp_luma, warp_chroma, vpp_warp_core.h) from the coordinate on.  The coordinate:
//   - The three inner fmafs -- of the X numerator, the Y numerator and the denominator -- depend on the row only: a thread tile evaluates them once per row, then
//     three fmafs, ONE reciprocal and two products per sample.  Two divisions would expand the division sequence twice per sample and have other bits.
//   - The chroma pairs have their own terms on the pair grid (PerspRec::chroma), never derived from the luma coordinates.
#pragma once
#include "vpp_warp_core.h"
#include "vpp_persp.h"

#pragma clang fp contract(off)

namespace tsvpp {

// convert_thread_tile (vpp_device.h) with the perspective sampler: 2 x 4 luma samples and 2 chroma pairs of the virtual NV12 frame, then the one colour back end
template <int OUT, bool VEC, bool BORDER, int EL, class S>
__device__ __forceinline__ void persp_thread_tile(const S &s, const LaunchDesc &d, const PerspRec &r, const PerspLaunch &L, typename OutT<OUT>::type *out, int i0, int j0) {
    // VEC: the thread tile has its four columns.  Element-wise flavour: 2 or 4; a column that does not exist is sampled at the row's last one and never stored.
    const int ncol = VEC ? PXW : min(PXW, d.dst_w - j0);
    const int ci = i0 >> 1, cj0 = j0 >> 1, jmax = d.dst_w - 1, cjmax = (d.dst_w >> 1) - 1;
    float Uf[2] = { 128.0f, 128.0f }, Vf[2] = { 128.0f, 128.0f }, Yf[PXH][PXW];
    if constexpr (!kLumaOnly<OUT>) {
        const PerspGrid &t = r.chroma;
        const float v = (float)ci + 0.5f;
        const float ix = warp_inner(v, t.bx, t.cx), iy = warp_inner(v, t.by, t.cy), iw = warp_inner(v, t.hh, t.k);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const float u = (float)(VEC ? cj0 + c : min(cj0 + c, cjmax)) + 0.5f;
            const float rw = persp_recip(warp_coord(u, t.g, iw));
            warp_chroma<BORDER>(s, warp_coord(u, t.ax, ix) * rw, warp_coord(u, t.ay, iy) * rw, L.border_u, L.border_v, Uf[c], Vf[c]);
        }
    }
#pragma unroll
    for (int rr = 0; rr < PXH; rr++) {
        // the chroma pairs, then one luma row at a time: a row's 16 taps are consumed before the next row's are issued (as warp_thread_tile, and for its reason)
        __builtin_amdgcn_sched_barrier(0);
        const PerspGrid &t = r.luma;
        const float v = (float)(i0 + rr) + 0.5f;
        const float ix = warp_inner(v, t.bx, t.cx), iy = warp_inner(v, t.by, t.cy), iw = warp_inner(v, t.hh, t.k);
#pragma unroll
        for (int c = 0; c < PXW; c++) {
            const float u = (float)(VEC ? j0 + c : min(j0 + c, jmax)) + 0.5f;
            const float rw = persp_recip(warp_coord(u, t.g, iw));
            Yf[rr][c] = warp_luma<BORDER>(s, warp_coord(u, t.ax, ix) * rw, warp_coord(u, t.ay, iy) * rw, L.border_y);
        }
    }
    store_tile<OUT, VEC, EL>(Yf, Uf, Vf, d, L.spec, out, i0, j0, ncol);
}

// (launch bounds: at least four waves per SIMD, i.e. at most 128 VGPRs -- four workgroups of the 40 KiB LDS budget per CU: profiles/persp_resources.txt)
// A function of its own beside vpp_warp_kernel, whose lines it repeats: as one kernel template the two compile to other code -- about 830 fewer instruction
// lines in each colour unit, about 900 with another opcode; the figures and the warning are at vpp_warp_kernel (vpp_warp_core.h).
template <int OUT, bool VEC, bool STAGED, bool BORDER, int EL = EL_LIB>
__global__ __launch_bounds__(ROI_THREADS, 4) void vpp_persp_kernel(const PerspLaunch L) {
    using T = typename OutT<OUT>::type;
    typedef __attribute__((address_space(1))) uint8_t *GP; // the records hold GLOBAL addresses (PtrCol, vpp_kernels.h)
    // workgroup -> (output, tile): all tiles of an output are neighbours in the grid, so the lines that adjacent tiles share meet in L2
    const TileIndex tix = tile_index(L.tiles_x, L.tiles_y);
    const int item = tix.item, tyi = tix.tyi, txi = tix.txi;
    if (item >= L.n) return;
    const PerspRec &r = L.r[item]; // wave-uniform index: scalar loads

    // the colour back end and the staging loop read their request from a LaunchDesc (the samplers' fields -- ratios, weights -- stay zero)
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
        // the tile's interval box (persp_footprint: the numbers the host sized the launch's LDS with); it lies inside the frame whatever the matrix
        RoiFootprint f;
        persp_footprint(r, j_first, tile_last(j_first, ROI_TILE_W, L.dst_w), i_first, tile_last(i_first, ROI_TILE_H, L.dst_h), f);
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
            if (active) persp_thread_tile<OUT, VEC, BORDER, EL>(s, d, r, L, out, i0, j0);
            return;
        }
    }
    if (!active) return;
    GlobalSrc s;
    tile_global_src(s, r, plane_y, plane_uv);
    persp_thread_tile<OUT, VEC, BORDER, EL>(s, d, r, L, out, i0, j0);
}

// The path's tag for launch_coord / launch_coord_tensor (vpp_tile_launch.h)
struct PerspKernels {
    using Launch = PerspLaunch;
    static constexpr const char *kName = "vpp_persp";
    template <int OUT, bool VEC, bool STAGED, bool BORDER, int EL> static constexpr auto kernel() { return &vpp_persp_kernel<OUT, VEC, STAGED, BORDER, EL>; }
};

} // namespace tsvpp
