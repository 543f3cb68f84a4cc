// vpp_letterbox_core.h -- the letterbox kernel itself (see vpp_letterbox.hip for what it does), as a template that two translation units instantiate:
// vpp_letterbox.hip with the library's colour back end (EL_LIB: every flavour of tsvpp_convert_letterbox) and vpp_letterbox_tensor.hip with the tensor store
// (EL_F32 / EL_HALF: tsvpp_convert_letterbox_tensor, vpp_tensor_store.h).  Nothing but the store call differs between them: the pad sample goes through
// whichever it is, like every other sample.
#pragma once
#include "vpp_letterbox.h"
#include "vpp_tile_core.h"

#pragma clang fp contract(off)

namespace tsvpp {

// The part of the rectangle one workgroup's tile covers, in inner indices (wave-uniform)
struct LbPart {
    int a0, a1, b0, b1;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// convert_thread_tile (vpp_device.h) for a thread tile of the canvas: samples at the inner coordinates, pad outside the rectangle.
template <int MODE, int OUT, bool VEC, int EL, class S>
__device__ __forceinline__ void letterbox_thread_tile(const S &s, const LaunchDesc &d, const LbRec &r, const LbPart &t, const LbLaunch &L, typename OutT<OUT>::type *out, int i0,
                                                      int j0) {
    const float pad_y = L.pad_y, pad_u = L.pad_u, pad_v = L.pad_v;
    // VEC: the thread tile has its four columns.  Element-wise flavour: 2 or 4; a column that does not exist lies outside the rectangle and is never stored.
    const int ncol = VEC ? PXW : min(PXW, d.dst_w - j0);
    const bool rows_in = i0 >= r.top && i0 < r.top + r.height;
    bool in[2];
#pragma unroll
    for (int c = 0; c < 2; c++) in[c] = rows_in && j0 + 2 * c >= r.left && j0 + 2 * c < r.left + r.width;
    float Uf[2] = { pad_u, pad_u }, Vf[2] = { pad_v, pad_v }, Yf[PXH][PXW];
#pragma unroll
    for (int rr = 0; rr < PXH; rr++)
#pragma unroll
        for (int c = 0; c < PXW; c++) Yf[rr][c] = pad_y;
    if (in[0] || in[1]) { // a thread tile wholly outside the rectangle samples nothing
        const int ci = clampi((i0 - r.top) >> 1, t.b0 >> 1, t.b1 >> 1), cj0 = (j0 - r.left) >> 1;
#pragma unroll
        for (int c = 0; c < 2; c++) {
            int U = 128, V = 128;
            if constexpr (!kLumaOnly<OUT>) sample_chroma<MODE>(s, d, ci, clampi(cj0 + c, t.a0 >> 1, t.a1 >> 1), U, V);
            Uf[c] = in[c] ? (float)U : pad_u;
            Vf[c] = in[c] ? (float)V : pad_v;
        }
#pragma unroll
        for (int rr = 0; rr < PXH; rr++)
#pragma unroll
            for (int c = 0; c < PXW; c++) {
                const int v = sample_luma<MODE>(s, d, clampi(i0 - r.top + rr, t.b0, t.b1), clampi(j0 - r.left + c, t.a0, t.a1));
                Yf[rr][c] = in[c >> 1] ? (float)v : pad_y;
            }
    }
    store_tile<OUT, VEC, EL>(Yf, Uf, Vf, d, L.spec, out, i0, j0, ncol);
}

template <int MODE, int OUT, bool VEC, bool STAGED, int EL = EL_LIB>
__global__ __launch_bounds__(ROI_THREADS) void vpp_letterbox_kernel(const LbLaunch L) {
    using T = typename OutT<OUT>::type;
    typedef __attribute__((address_space(1))) uint8_t *GP; // the records hold GLOBAL addresses (PtrCol, vpp_kernels.h)
    // workgroup -> (frame, canvas tile): all tiles of a canvas are neighbours in the grid
    const TileIndex tix = tile_index(L.tiles_x, L.tiles_y);
    const int frame = tix.item, tyi = tix.tyi, txi = tix.txi;
    if (frame >= L.n_frames) return;
    const LbRec &r = L.r[frame]; // wave-uniform index: scalar loads

    // the samplers and the colour back end read their request from a LaunchDesc: this frame's source and ratios, the CANVAS as the output
    LaunchDesc d = {};
    tile_desc<OUT, VEC>(L, r, d);

    const uint8_t *const plane_y = (const uint8_t *)(GP)(uintptr_t)r.y, *const plane_uv = (const uint8_t *)(GP)(uintptr_t)r.uv;
    T *const out = (T *)(GP)(uintptr_t)r.out;
    // (the coordinates are written out in all three tile kernels: as a helper of vpp_tile_core.h they moved VGPRs in vpp_rois_kernel and vpp_letterbox_kernel)
    const int lx = threadIdx.x & (ROI_TX - 1), ly = threadIdx.x >> ROI_TX_SHIFT;
    const int j_first = roi_tile_col0(txi, L.dst_w, d.last_col0), i_first = tyi * ROI_TILE_H;
    const int j0 = j_first + lx * PXW, i0 = i_first + ly * PXH;
    const bool active = j0 < L.dst_w && i0 < L.dst_h && !(VEC && is_row_tail(d, j0));

    // the part of the rectangle this tile covers (wave-uniform)
    LbPart t;
    tile_inner_range(j_first, tile_last(j_first, ROI_TILE_W, L.dst_w), r.left, r.width, t.a0, t.a1);
    tile_inner_range(i_first, tile_last(i_first, ROI_TILE_H, L.dst_h), r.top, r.height, t.b0, t.b1);
    if (t.a0 > t.a1 || t.b0 > t.b1) { // none of it: pad, through the colour back end
        if (!active) return;
        const float Uf[2] = { L.pad_u, L.pad_u }, Vf[2] = { L.pad_v, L.pad_v };
        float Yf[PXH][PXW];
#pragma unroll
        for (int rr = 0; rr < PXH; rr++)
#pragma unroll
            for (int c = 0; c < PXW; c++) Yf[rr][c] = L.pad_y;
        const int ncol = VEC ? PXW : min(PXW, L.dst_w - j0);
        store_tile<OUT, VEC, EL>(Yf, Uf, Vf, d, L.spec, out, i0, j0, ncol);
        return;
    }

    if constexpr (STAGED) {
        RoiFootprint f;
        tile_span_x(MODE, t.a0, t.a1, r.src_w, r.xr, f);
        tile_span_y(MODE, t.b0, t.b1, r.src_h, r.yr, f);
        if (roi_stageable(f) && roi_lds_need(f, kLumaOnly<OUT>) <= L.lds_bytes) { // (wave-uniform)
            // (the staging block is written out in all three tile kernels: as a helper it changed their instructions and measured slower, profiles/tile_core_ab.txt)
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
            if (active) letterbox_thread_tile<MODE, OUT, VEC, EL>(s, d, r, t, L, out, i0, j0);
            return;
        }
    }
    if (!active) return;
    GlobalSrc s;
    tile_global_src(s, r, plane_y, plane_uv);
    letterbox_thread_tile<MODE, OUT, VEC, EL>(s, d, r, t, L, out, i0, j0);
}

} // namespace tsvpp
