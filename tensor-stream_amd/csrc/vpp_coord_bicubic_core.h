// vpp_coord_bicubic_core.h -- BICUBIC through a coordinate: the kernel of tsvpp_convert_warp_bicubic and tsvpp_convert_perspective_bicubic (include/tsvpp.h), as ONE
// template over the path (WarpCubic, PerspCubic below) that four translation units instantiate: vpp_warp_bicubic.hip / vpp_persp_bicubic.hip with the library's
// colour back end (EL_LIB) and their *_tensor.hip twins with the tensor store (EL_F32 / EL_HALF).  The existing kernels (vpp_warp_core.h, vpp_persp_core.h) are
// not touched: their units compile to the code they had.
//
// What is the BILINEAR kernels': the tile and its index (tile_index), the records and launch blocks, the coordinate expressions (warp_inner / warp_coord /
// persp_recip, evaluated in the same order: the coordinate has the BILINEAR call's bits), staging (describe_plane, stage_planes), the staged-or-gather decision
// per tile, the border test (warp_outside) and the store (store_tile).  What is new:
//   - the sampler: 16 taps per luma sample and per chroma component through S::Y / S::UV, the taps by the reference's edge rule (bicubic_offsets) from the
//     centre tap of warp_cubic_axis, the sums by the library's mixed-precision cubic (cubic_coeffs_f, cubic4_pair: fp32, recomputed in fp64 within CUBIC_DELTA
//     of a tie, so the result is the fp64 one).  Unlike the resize kernels neighbours share no weights: the coefficients are per sample and axis.  cubic4_pair
//     takes two sums with their own weights: two neighbouring luma samples go through it together, and so do U and V of a chroma pair (which share theirs).
//   - the footprint: warp_bicubic_footprint / persp_bicubic_footprint (vpp_coord_bicubic.h), the BILINEAR box with the 4-tap halo.
#pragma once
#include "vpp_persp_core.h"
#include "vpp_coord_bicubic.h"

#pragma clang fp contract(off)

namespace tsvpp {

// Centre tap, tap offsets and coefficients of one axis of one sample
struct CubicAxis {
    int p, lo, hi;
    float w, c[4];
};
__device__ __forceinline__ void cubic_axis_of(float f, int limit, CubicAxis &a) {
    warp_cubic_axis(f, limit, a.p, a.w);
    bicubic_offsets(a.p, 1, limit, a.lo, a.hi);
    cubic_coeffs_f(a.w, a.c);
}

// Two luma samples at source coordinates (fx[k], fy[k]): per tap row the two horizontal sums as one pair, then the vertical sums as one pair
template <bool BORDER, class S> __device__ __forceinline__ void cubic_luma2(const S &s, const float fx[2], const float fy[2], float border, float &out0, float &out1) {
    CubicAxis X[2], Y[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        cubic_axis_of(fx[k], s.w, X[k]);
        cubic_axis_of(fy[k], s.h, Y[k]);
    }
    const int xo0[4] = { X[0].p - X[0].lo, X[0].p, X[0].p + X[0].hi, X[0].p + 2 * X[0].hi }, xo1[4] = { X[1].p - X[1].lo, X[1].p, X[1].p + X[1].hi, X[1].p + 2 * X[1].hi };
    const int yo0[4] = { Y[0].p - Y[0].lo, Y[0].p, Y[0].p + Y[0].hi, Y[0].p + 2 * Y[0].hi }, yo1[4] = { Y[1].p - Y[1].lo, Y[1].p, Y[1].p + Y[1].hi, Y[1].p + 2 * Y[1].hi };
    f2 b[4];
    int b0[4], b1[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        int q0[4], q1[4];
        f2 p[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            q0[t] = s.Y(yo0[r], xo0[t]);
            q1[t] = s.Y(yo1[r], xo1[t]);
            p[t] = (f2){ (float)q0[t], (float)q1[t] };
        }
        b[r] = cubic4_pair(X[0].w, X[1].w, X[0].c, X[1].c, p, q0, q1);
        b0[r] = (int)b[r].x;
        b1[r] = (int)b[r].y;
    }
    const f2 v = cubic4_pair(Y[0].w, Y[1].w, Y[0].c, Y[1].c, b, b0, b1);
    out0 = v.x;
    out1 = v.y;
    if constexpr (BORDER) {
        out0 = (warp_outside(fx[0], s.w) || warp_outside(fy[0], s.h)) ? border : out0;
        out1 = (warp_outside(fx[1], s.w) || warp_outside(fy[1], s.h)) ? border : out1;
    }
}
// One chroma pair at pair-grid coordinate (fx, fy): the edge rule on pairs (limits w / 2, h / 2), U and V from byte columns 2 p and 2 p + 1 with the same weights
template <bool BORDER, class S> __device__ __forceinline__ void cubic_chroma(const S &s, float fx, float fy, float border_u, float border_v, float &U, float &V) {
    const int cw = s.w >> 1, ch = s.h >> 1;
    CubicAxis X, Y;
    cubic_axis_of(fx, cw, X);
    cubic_axis_of(fy, ch, Y);
    const int xo[4] = { 2 * (X.p - X.lo), 2 * X.p, 2 * (X.p + X.hi), 2 * (X.p + 2 * X.hi) };
    const int yo[4] = { Y.p - Y.lo, Y.p, Y.p + Y.hi, Y.p + 2 * Y.hi };
    f2 b[4];
    int bu[4], bv[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        int qu[4], qv[4];
        f2 p[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            qu[t] = s.UV(yo[r], xo[t]);
            qv[t] = s.UV(yo[r], xo[t] + 1);
            p[t] = (f2){ (float)qu[t], (float)qv[t] };
        }
        b[r] = cubic4_pair(X.w, X.w, X.c, X.c, p, qu, qv);
        bu[r] = (int)b[r].x;
        bv[r] = (int)b[r].y;
    }
    const f2 v = cubic4_pair(Y.w, Y.w, Y.c, Y.c, b, bu, bv);
    U = v.x;
    V = v.y;
    if constexpr (BORDER) {
        const bool outside = warp_outside(fx, cw) || warp_outside(fy, ch);
        U = outside ? border_u : U;
        V = outside ? border_v : V;
    }
}

// The two paths: launch block, record, footprint, and the coordinate as the BILINEAR thread tiles evaluate it (warp_thread_tile, persp_thread_tile) -- what
// depends on the row alone once per row, then per sample
struct WarpCubic {
    using Launch = WarpLaunch;
    using Rec = WarpRec;
    struct Row {
        float ax, ay;
    };
    static __device__ __forceinline__ void footprint(const Rec &r, int j0, int j1, int i0, int i1, RoiFootprint &f) { warp_bicubic_footprint(r, j0, j1, i0, i1, f); }
    static __device__ __forceinline__ Row luma_row(const Rec &r, float v) { return { warp_inner(v, r.m1, r.tx), warp_inner(v, r.m4, r.ty) }; }
    static __device__ __forceinline__ Row chroma_row(const Rec &r, float v) { return { warp_inner(v, r.m1, r.ctx), warp_inner(v, r.m4, r.cty) }; }
    static __device__ __forceinline__ void luma_at(const Rec &r, const Row &row, float u, float &fx, float &fy) {
        fx = warp_coord(u, r.m0, row.ax);
        fy = warp_coord(u, r.m3, row.ay);
    }
    static __device__ __forceinline__ void chroma_at(const Rec &r, const Row &row, float u, float &fx, float &fy) { luma_at(r, row, u, fx, fy); }
};
struct PerspCubic {
    using Launch = PerspLaunch;
    using Rec = PerspRec;
    struct Row {
        float ix, iy, iw;
    };
    static __device__ __forceinline__ void footprint(const Rec &r, int j0, int j1, int i0, int i1, RoiFootprint &f) { persp_bicubic_footprint(r, j0, j1, i0, i1, f); }
    static __device__ __forceinline__ Row grid_row(const PerspGrid &t, float v) { return { warp_inner(v, t.bx, t.cx), warp_inner(v, t.by, t.cy), warp_inner(v, t.hh, t.k) }; }
    static __device__ __forceinline__ void grid_at(const PerspGrid &t, const Row &row, float u, float &fx, float &fy) {
        const float rw = persp_recip(warp_coord(u, t.g, row.iw));
        fx = warp_coord(u, t.ax, row.ix) * rw;
        fy = warp_coord(u, t.ay, row.iy) * rw;
    }
    static __device__ __forceinline__ Row luma_row(const Rec &r, float v) { return grid_row(r.luma, v); }
    static __device__ __forceinline__ Row chroma_row(const Rec &r, float v) { return grid_row(r.chroma, v); }
    static __device__ __forceinline__ void luma_at(const Rec &r, const Row &row, float u, float &fx, float &fy) { grid_at(r.luma, row, u, fx, fy); }
    static __device__ __forceinline__ void chroma_at(const Rec &r, const Row &row, float u, float &fx, float &fy) { grid_at(r.chroma, row, u, fx, fy); }
};

// warp_thread_tile with the cubic sampler: 2 x 4 luma samples and 2 chroma pairs of the virtual NV12 frame, then the one colour back end
template <class PATH, int OUT, bool VEC, bool BORDER, int EL, class S>
__device__ __forceinline__ void cubic_thread_tile(const S &s, const LaunchDesc &d, const typename PATH::Rec &r, const typename PATH::Launch &L, typename OutT<OUT>::type *out,
                                                  int i0, int j0) {
    // VEC: the thread tile has its four columns.  Element-wise flavour: 2 or 4; a column that does not exist is sampled at the row's last one and never stored.
    const int ncol = VEC ? PXW : min(PXW, d.dst_w - j0);
    const int ci = i0 >> 1, cj0 = j0 >> 1, jmax = d.dst_w - 1, cjmax = (d.dst_w >> 1) - 1;
    float Uf[2] = { 128.0f, 128.0f }, Vf[2] = { 128.0f, 128.0f }, Yf[PXH][PXW];
    if constexpr (!kLumaOnly<OUT>) {
        const typename PATH::Row row = PATH::chroma_row(r, (float)ci + 0.5f);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            // one pair's 32 taps at a time (below)
            __builtin_amdgcn_sched_barrier(0);
            const float u = (float)(VEC ? cj0 + c : min(cj0 + c, cjmax)) + 0.5f;
            float fx, fy;
            PATH::chroma_at(r, row, u, fx, fy);
            cubic_chroma<BORDER>(s, fx, fy, L.border_u, L.border_v, Uf[c], Vf[c]);
        }
    }
#pragma unroll
    for (int rr = 0; rr < PXH; rr++) {
        const typename PATH::Row row = PATH::luma_row(r, (float)(i0 + rr) + 0.5f);
#pragma unroll
        for (int c = 0; c < PXW; c += 2) {
            // two samples' 32 taps are consumed before the next two samples' are issued: the BILINEAR kernels fence a row's 16 taps for the same reason
            // (warp_thread_tile), and a row here has 64
            __builtin_amdgcn_sched_barrier(0);
            float fx[2], fy[2];
#pragma unroll
            for (int k = 0; k < 2; k++) PATH::luma_at(r, row, (float)(VEC ? j0 + c + k : min(j0 + c + k, jmax)) + 0.5f, fx[k], fy[k]);
            cubic_luma2<BORDER>(s, fx, fy, L.border_y, Yf[rr][c], Yf[rr][c + 1]);
        }
    }
    store_tile<OUT, VEC, EL>(Yf, Uf, Vf, d, L.spec, out, i0, j0, ncol);
}

// vpp_warp_kernel / vpp_persp_kernel with the cubic thread tile and footprint, once for both paths (those two stay two functions for the code the compiler made of
// their union; nothing is pinned here).  Launch bounds as theirs: at least four waves per SIMD, i.e. at most 128 VGPRs.  With two samples' 32 taps fenced as above
// the instantiations take 75 to 107 and none spills: profiles/coord_bicubic_resources.txt.
template <class PATH, int OUT, bool VEC, bool STAGED, bool BORDER, int EL>
__global__ __launch_bounds__(ROI_THREADS, 4) void vpp_coord_bicubic_kernel(const typename PATH::Launch L) {
    using T = typename OutT<OUT>::type;
    typedef __attribute__((address_space(1))) uint8_t *GP; // the records hold GLOBAL addresses (PtrCol, vpp_kernels.h)
    const TileIndex tix = tile_index(L.tiles_x, L.tiles_y);
    const int item = tix.item, tyi = tix.tyi, txi = tix.txi;
    if (item >= L.n) return;
    const typename PATH::Rec &r = L.r[item]; // wave-uniform index: scalar loads

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
        // the tile's box with the 4-tap halo (the numbers the host sized the launch's LDS with); it lies inside the frame whatever the matrix
        RoiFootprint f;
        PATH::footprint(r, j_first, tile_last(j_first, ROI_TILE_W, L.dst_w), i_first, tile_last(i_first, ROI_TILE_H, L.dst_h), f);
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
            stage_planes<2, 1>(d, lds_y, ay, s.py_, ny, span_y, lds_uv, auv, s.puv_, nuv, span_uv, ROI_THREADS);
            __syncthreads();
            if (active) cubic_thread_tile<PATH, OUT, VEC, BORDER, EL>(s, d, r, L, out, i0, j0);
            return;
        }
    }
    if (!active) return;
    GlobalSrc s;
    tile_global_src(s, r, plane_y, plane_uv);
    cubic_thread_tile<PATH, OUT, VEC, BORDER, EL>(s, d, r, L, out, i0, j0);
}

// The paths' tags for launch_coord / launch_coord_tensor (vpp_tile_launch.h)
struct WarpBicubicKernels {
    using Launch = WarpLaunch;
    static constexpr const char *kName = "vpp_warp_bicubic";
    template <int OUT, bool VEC, bool STAGED, bool BORDER, int EL> static constexpr auto kernel() { return &vpp_coord_bicubic_kernel<WarpCubic, OUT, VEC, STAGED, BORDER, EL>; }
};
struct PerspBicubicKernels {
    using Launch = PerspLaunch;
    static constexpr const char *kName = "vpp_persp_bicubic";
    template <int OUT, bool VEC, bool STAGED, bool BORDER, int EL> static constexpr auto kernel() { return &vpp_coord_bicubic_kernel<PerspCubic, OUT, VEC, STAGED, BORDER, EL>; }
};

} // namespace tsvpp
