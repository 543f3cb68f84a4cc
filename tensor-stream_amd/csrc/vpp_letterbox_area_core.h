// vpp_letterbox_area_core.h -- the AREA letterbox kernel itself (see vpp_letterbox_area.hip for what it does), as a template that two translation units
// instantiate: vpp_letterbox_area.hip with the library's colour back end (EL_LIB: every flavour of tsvpp_convert_letterbox_area without a spec) and
// vpp_letterbox_area_tensor.hip with the tensor store (EL_F32 / EL_HALF: the same call with a spec, vpp_tensor_store.h).  Nothing but the store call differs between
// them: the pad sample goes through whichever it is, like every other sample.
#pragma once
#include "vpp_letterbox_area.h"
#include "vpp_letterbox_core.h"
#include "vpp_rois_area_core.h"

#pragma clang fp contract(off)

namespace tsvpp {

// letterbox_thread_tile (vpp_letterbox_core.h) with the samplers of the weighted box (area_luma / area_chroma, vpp_rois_area_core.h): samples at the inner
// coordinates clamped into the tile's part of the rectangle -- the indices the tile holds weight rows and a footprint for --, pad outside the rectangle.
template <int OUT, bool VEC, int EL, class S>
__device__ __forceinline__ void letterbox_area_thread_tile(const S &s, const LaunchDesc &d, const RoiAreaRows &w, const LbRec &r, const LbPart &t, const LbLaunch &L,
                                                           typename OutT<OUT>::type *out, int i0, int j0) {
    const float pad_y = L.pad_y, pad_u = L.pad_u, pad_v = L.pad_v;
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
            if constexpr (!kLumaOnly<OUT>) area_chroma(s, d, w, ci, clampi(cj0 + c, t.a0 >> 1, t.a1 >> 1), U, V);
            Uf[c] = in[c] ? (float)U : pad_u;
            Vf[c] = in[c] ? (float)V : pad_v;
        }
#pragma unroll
        for (int rr = 0; rr < PXH; rr++)
#pragma unroll
            for (int c = 0; c < PXW; c++) {
                const int v = area_luma(s, d, w, clampi(i0 - r.top + rr, t.b0, t.b1), clampi(j0 - r.left + c, t.a0, t.a1));
                Yf[rr][c] = in[c >> 1] ? (float)v : pad_y;
            }
    }
    store_tile<OUT, VEC, EL>(Yf, Uf, Vf, d, L.spec, out, i0, j0, ncol);
}

template <int OUT, bool VEC, bool STAGED, int EL = EL_LIB>
__global__ __launch_bounds__(ROI_THREADS) void vpp_letterbox_area_kernel(const LbAreaLaunch L) {
    using T = typename OutT<OUT>::type;
    typedef __attribute__((address_space(1))) uint8_t *GP; // the records hold GLOBAL addresses (PtrCol, vpp_kernels.h)
    // workgroup -> (frame, canvas tile): all tiles of a canvas are neighbours in the grid
    const TileIndex tix = tile_index(L.tiles_x, L.tiles_y);
    const int frame = tix.item, tyi = tix.tyi, txi = tix.txi;
    if (frame >= L.n_frames) return;
    const LbRec &r = L.r[frame]; // wave-uniform index: scalar loads

    LaunchDesc d = {};
    tile_desc<OUT, VEC>(L, r, d);

    const uint8_t *const plane_y = (const uint8_t *)(GP)(uintptr_t)r.y, *const plane_uv = (const uint8_t *)(GP)(uintptr_t)r.uv;
    T *const out = (T *)(GP)(uintptr_t)r.out;
    const int lx = threadIdx.x & (ROI_TX - 1), ly = threadIdx.x >> ROI_TX_SHIFT;
    const int j_first = roi_tile_col0(txi, L.dst_w, d.last_col0), i_first = tyi * ROI_TILE_H;
    const int j0 = j_first + lx * PXW, i0 = i_first + ly * PXH;
    const bool active = j0 < L.dst_w && i0 < L.dst_h && !(VEC && is_row_tail(d, j0));

    // the part of the rectangle this tile covers (wave-uniform)
    LbPart t;
    tile_inner_range(j_first, tile_last(j_first, ROI_TILE_W, L.dst_w), r.left, r.width, t.a0, t.a1);
    tile_inner_range(i_first, tile_last(i_first, ROI_TILE_H, L.dst_h), r.top, r.height, t.b0, t.b1);
    if (t.a0 > t.a1 || t.b0 > t.b1) { // none of it: pad, through the colour back end; no rows, no chain
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
    const bool down = roi_area_mode(r.xr, r.yr) == M_AREA_DOWN; // wave-uniform: the record's ratios

    // the weight rows of inner columns [a0, a1] and inner rows [b0, b1]: in front of the staged footprint, laid out as vpp_rois_area.hip's
    float *const rows = (float *)lds_raw;
    RoiAreaRows w = {};
    if (down) {
        w.tx = roi_area_taps(r.xr);
        w.ty = roi_area_taps(r.yr);
        w.sx = roi_area_stride(w.tx);
        w.sy = roi_area_stride(w.ty);
        w.j_first = t.a0;
        w.cj_first = t.a0 >> 1;
        w.i_first = t.b0;
        w.ci_first = t.b0 >> 1;
        w.xl = rows;
        w.xc = rows + ROI_TILE_W * w.sx;
        w.yl = rows + ROI_AREA_ROWS * w.sx;
        w.yc = w.yl + ROI_TILE_H * w.sy;
        if (threadIdx.x >= 64) { // the second wave, whole: the periods of both axes by ballot, then four of its lanes run the four chains side by side
            const int px = lb_area_period(r.xr, t.a0), py = lb_area_period(r.yr, t.b0);
            const int c = (int)threadIdx.x - 64;
            if (c < 4) { // x luma, y luma, x chroma, y chroma
                const int axis = c & 1, chroma = c >> 1;
                const float scale = axis ? r.yr : r.xr;
                const int lo = (axis ? t.b0 : t.a0) >> chroma, hi = (axis ? t.b1 : t.a1) >> chroma;
                RoiAreaRow *const recs = (RoiAreaRow *)(rows + roi_area_rows_floats(w.tx, w.ty)) + axis * (ROI_AREA_ROWS + 1) + chroma * ROI_TILE_W;
                RoiAreaGen g; // (0, 0): the state behind every reset, so the state at any multiple of the period
                for (int k = lb_area_start_of(axis ? py : px, lo); k <= hi; k++) {
                    const RoiAreaRow row = roi_area_step(scale, g);
                    if (k >= lo) recs[k - lo] = row;
                }
            }
        }
    }

    bool staged = false;
    LdsSrc ls = {};
    if constexpr (STAGED) {
        const int mode = down ? M_AREA_DOWN : M_AREA_UP;
        RoiFootprint f;
        tile_span_x(mode, t.a0, t.a1, r.src_w, r.xr, f);
        tile_span_y(mode, t.b0, t.b1, r.src_h, r.yr, f);
        if (roi_stageable(f) && roi_lds_need(f, kLumaOnly<OUT>) <= L.lds_bytes) { // (wave-uniform)
            const int span_y = f.xhi - f.xlo + 1, span_uv = 2 * (f.cxhi - f.cxlo + 1);
            const int ny = f.yhi - f.ylo + 1, nuv = kLumaOnly<OUT> ? 0 : f.cyhi - f.cylo + 1;
            d.lds_cpr_y = roi_chunks(span_y);
            d.lds_cpr_uv = roi_chunks(span_uv);
            d.lds_slot_y = 32 - __builtin_clz(((unsigned)d.lds_cpr_y - 1u) | 1u);
            d.lds_slot_uv = 32 - __builtin_clz(((unsigned)d.lds_cpr_uv - 1u) | 1u);
            uint8_t *lds_y = lds_raw + L.area_lds, *lds_uv = lds_y + ny * d.lds_cpr_y * 16;
            const uint8_t *ay, *auv;
            ls.py_ = describe_plane(lds_y, plane_y, r.pitch_y, f.ylo, f.xlo, d.lds_cpr_y, ay);
            ls.puv_ = describe_plane(lds_uv, plane_uv, r.pitch_uv, f.cylo, 2 * f.cxlo, d.lds_cpr_uv, auv);
            ls.w = r.src_w;
            ls.h = r.src_h;
            stage_planes<2, 1>(d, lds_y, ay, ls.py_, ny, span_y, lds_uv, auv, ls.puv_, nuv, span_uv, ROI_THREADS);
            staged = true;
        }
    }
    __syncthreads(); // row records and footprint are in LDS
    if (down) {
        // every row of both axes by a lane of its own: record -> taps floats
        const int e = (int)threadIdx.x, axis = e >= ROI_AREA_ROWS ? 1 : 0, row = e - axis * ROI_AREA_ROWS;
        const int first = axis ? t.b0 : t.a0, last = axis ? t.b1 : t.a1;
        const int n_rows = row < ROI_TILE_W ? last - first + 1 : ROI_TILE_W + (last >> 1) - (first >> 1) + 1; // rows of this range the chains have written
        if (e < 2 * ROI_AREA_ROWS && row < n_rows) {
            const RoiAreaRow rec = ((const RoiAreaRow *)(rows + roi_area_rows_floats(w.tx, w.ty)))[axis * (ROI_AREA_ROWS + 1) + row];
            const int taps = axis ? w.ty : w.tx;
            float *const dst = rows + (axis ? ROI_AREA_ROWS * w.sx : 0) + row * (axis ? w.sy : w.sx);
            for (int b = 0; b < taps; b++) dst[b] = roi_area_weight(rec, b);
        }
        __syncthreads(); // (wave-uniform branch: every lane of the workgroup is here)
    }
    if (!active) return;
    GlobalSrc gs;
    tile_global_src(gs, r, plane_y, plane_uv);
    if (down) {
        if (STAGED && staged) letterbox_area_thread_tile<OUT, VEC, EL>(ls, d, w, r, t, L, out, i0, j0);
        else letterbox_area_thread_tile<OUT, VEC, EL>(gs, d, w, r, t, L, out, i0, j0);
    } else {
        if (STAGED && staged) letterbox_thread_tile<M_AREA_UP, OUT, VEC, EL>(ls, d, r, t, L, out, i0, j0);
        else letterbox_thread_tile<M_AREA_UP, OUT, VEC, EL>(gs, d, r, t, L, out, i0, j0);
    }
}

} // namespace tsvpp
