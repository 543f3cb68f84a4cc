// vpp_rois_area_core.h -- the AREA region-of-interest kernel itself (see vpp_rois_area.hip for what it does and what was tried), as a template that two translation
// units instantiate: vpp_rois_area.hip with the library's colour back end (EL_LIB: every flavour of tsvpp_convert_rois_area) and vpp_rois_area_tensor.hip with the
// tensor store (EL_F32 / EL_HALF: tsvpp_convert_rois_tensor with TSVPP_AREA, vpp_tensor_store.h).  Nothing but the store call differs between them.
#pragma once
#include "vpp_tile_core.h"

#pragma clang fp contract(off)

namespace tsvpp {

// The weight rows of one tile in LDS (addresses of index `first` of each range) and the tap counts of the box
struct RoiAreaRows {
    const float *xl, *xc, *yl, *yc; // luma / chroma rows of the x axis, of the y axis
    int j_first, cj_first, i_first, ci_first;
    int tx, ty, sx, sy; // taps and row strides (floats)
};

// Luma of output (i, j): src/Resize.cu:160-178, 186-201 with the operation order of sample_luma<M_AREA_DOWN>
template <class S> __device__ __forceinline__ int area_luma(const S &s, const LaunchDesc &d, const RoiAreaRows &w, int i, int j) {
    const int y = (int)(d.yr * (float)i), x = (int)(d.xr * (float)j);
    const float *px = w.xl + (j - w.j_first) * w.sx, *py = w.yl + (i - w.i_first) * w.sy;
    float sum = 0.f, div = 0.f;
    for (int a = 0; a < w.ty; a++) {
        const float wy = py[a];
        const int row = min(y + a, s.h - 1);
        for (int b = 0; b < w.tx; b++) {
            const float wgt = px[b] * wy;
            div = div + wgt;
            sum = __builtin_fmaf((float)s.Y(row, min(x + b, s.w - 1)), wgt, sum);
        }
    }
    sum = sum / div;
    return (int)sum & 0xff;
}
// Chroma pair of chroma-grid (ci, cj): src/Resize.cu:204-210 -- the same rows of the same patterns, on the chroma grid's own indices
template <class S> __device__ __forceinline__ void area_chroma(const S &s, const LaunchDesc &d, const RoiAreaRows &w, int ci, int cj, int &U, int &V) {
    const int y = (int)(d.yr * (float)ci), x = (int)(d.xr * (float)cj);
    const float *px = w.xc + (cj - w.cj_first) * w.sx, *py = w.yc + (ci - w.ci_first) * w.sy;
    const int ch = s.h >> 1, cw = s.w >> 1;
    float su = 0.f, sv = 0.f, div = 0.f;
    for (int a = 0; a < w.ty; a++) {
        const float wy = py[a];
        const int row = min(y + a, ch - 1);
        for (int b = 0; b < w.tx; b++) {
            const float wgt = px[b] * wy;
            const int col = 2 * min(x + b, cw - 1);
            div = div + wgt;
            su = __builtin_fmaf((float)s.UV(row, col), wgt, su);
            sv = __builtin_fmaf((float)s.UV(row, col + 1), wgt, sv);
        }
    }
    su = su / div;
    sv = sv / div;
    U = (int)su & 0xff;
    V = (int)sv & 0xff;
}
// convert_thread_tile (vpp_device.h) with the two samplers above
template <int OUT, bool VEC, int EL, class S>
__device__ __forceinline__ void area_thread_tile(const S &s, const LaunchDesc &d, const RoiAreaRows &w, const tsvpp_tensor_spec &a, typename OutT<OUT>::type *out, int i0,
                                                 int j0) {
    const int ncol = VEC ? PXW : min(PXW, d.dst_w - j0);
    const int ci = i0 >> 1, cj0 = j0 >> 1, jmax = d.dst_w - 1, cjmax = (d.dst_w >> 1) - 1;
    float Uf[2], Vf[2], Yf[PXH][PXW];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        int U = 128, V = 128;
        if constexpr (!kLumaOnly<OUT>) area_chroma(s, d, w, ci, VEC ? cj0 + c : min(cj0 + c, cjmax), U, V);
        Uf[c] = (float)U;
        Vf[c] = (float)V;
    }
#pragma unroll
    for (int r = 0; r < PXH; r++)
#pragma unroll
        for (int c = 0; c < PXW; c++) Yf[r][c] = (float)area_luma(s, d, w, i0 + r, VEC ? j0 + c : min(j0 + c, jmax));
    store_tile<OUT, VEC, EL>(Yf, Uf, Vf, d, a, out, i0, j0, ncol);
}

template <int OUT, bool VEC, bool STAGED, int EL = EL_LIB>
__global__ __launch_bounds__(ROI_THREADS) void vpp_rois_area_kernel(const RoiLaunch L) {
    using T = typename OutT<OUT>::type;
    typedef __attribute__((address_space(1))) uint8_t *GP;
    // (written out: with tile_index of vpp_tile_core.h 16 of the 24 kernels of vpp_rois_area.hip compile to other instructions)
    const int tiles = L.tiles_x * L.tiles_y;
    const int box = (int)blockIdx.x / tiles;
    const int rem = (int)blockIdx.x - box * tiles;
    const int tyi = rem / L.tiles_x, txi = rem - tyi * L.tiles_x;
    if (box >= L.n_rois) return;
    const RoiRec &r = L.r[box]; // wave-uniform index: scalar loads

    LaunchDesc d = {};
    tile_desc<OUT, VEC>(L, r, d);

    const uint8_t *const plane_y = (const uint8_t *)(GP)(uintptr_t)r.y, *const plane_uv = (const uint8_t *)(GP)(uintptr_t)r.uv;
    T *const out = (T *)(GP)(uintptr_t)r.out;
    // (the coordinates are written out in all three tile kernels: as a helper of vpp_tile_core.h they moved VGPRs in vpp_rois_kernel and vpp_letterbox_kernel)
    const int lx = threadIdx.x & (ROI_TX - 1), ly = threadIdx.x >> ROI_TX_SHIFT;
    const int j_first = roi_tile_col0(txi, L.dst_w, d.last_col0), i_first = tyi * ROI_TILE_H;
    const int j_last = min(j_first + ROI_TILE_W, L.dst_w) - 1, i_last = min(i_first + ROI_TILE_H, L.dst_h) - 1;
    const int j0 = j_first + lx * PXW, i0 = i_first + ly * PXH;
    const bool active = j0 < L.dst_w && i0 < L.dst_h && !(VEC && is_row_tail(d, j0));
    const bool down = roi_area_mode(r.xr, r.yr) == M_AREA_DOWN; // wave-uniform: the record's ratios

    // the weight rows: in front of the staged footprint
    float *const rows = (float *)lds_raw;
    RoiAreaRows w = {};
    if (down) {
        w.tx = roi_area_taps(r.xr);
        w.ty = roi_area_taps(r.yr);
        w.sx = roi_area_stride(w.tx);
        w.sy = roi_area_stride(w.ty);
        w.j_first = j_first;
        w.cj_first = j_first >> 1;
        w.i_first = i_first;
        w.ci_first = i_first >> 1;
        w.xl = rows;
        w.xc = rows + ROI_TILE_W * w.sx;
        w.yl = rows + ROI_AREA_ROWS * w.sx;
        w.yc = w.yl + ROI_TILE_H * w.sy;
        if ((threadIdx.x >> 1) == 32) { // lanes 0 and 1 of the second wave: the x chain and the y chain, side by side, branch-free
            const int axis = threadIdx.x & 1;
            const float scale = axis ? r.yr : r.xr;
            RoiAreaRow *const recs = (RoiAreaRow *)(rows + roi_area_rows_floats(w.tx, w.ty)) + axis * (ROI_AREA_ROWS + 1);
            const int first = axis ? i_first : j_first, last = axis ? i_last : j_last;
            const int cfirst = first >> 1, clast = last >> 1;
            RoiAreaGen g;
            for (int k = 0; k <= last; k++) {
                const RoiAreaRow row = roi_area_step(scale, g);
                recs[k >= first ? k - first : ROI_AREA_ROWS] = row;                                          // (slot ROI_AREA_ROWS: never read)
                recs[(k >= cfirst && k <= clast) ? ROI_TILE_W + k - cfirst : ROI_AREA_ROWS] = row;
            }
        }
    }

    bool staged = false;
    LdsSrc ls = {};
    if constexpr (STAGED) {
        const int mode = down ? M_AREA_DOWN : M_AREA_UP;
        RoiFootprint f;
        tile_span_x(mode, j_first, j_last, r.src_w, r.xr, f);
        tile_span_y(mode, i_first, i_last, r.src_h, r.yr, f);
        if (roi_stageable(f) && roi_lds_need(f, kLumaOnly<OUT>) <= L.lds_bytes) { // (wave-uniform)
            // (the staging block is written out in all three tile kernels: as a helper it changed their instructions and measured slower, profiles/tile_core_ab.txt)
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
        const int t = (int)threadIdx.x, axis = t >= ROI_AREA_ROWS ? 1 : 0, row = t - axis * ROI_AREA_ROWS;
        const int first = axis ? i_first : j_first, last = axis ? i_last : j_last;
        const int n_rows = row < ROI_TILE_W ? last - first + 1 : ROI_TILE_W + (last >> 1) - (first >> 1) + 1; // rows of this range the chain has written
        if (t < 2 * ROI_AREA_ROWS && row < n_rows) {
            const RoiAreaRow rec = ((const RoiAreaRow *)(rows + roi_area_rows_floats(w.tx, w.ty)))[axis * (ROI_AREA_ROWS + 1) + row];
            const int taps = axis ? w.ty : w.tx;
            float *const dst = rows + (axis ? ROI_AREA_ROWS * w.sx : 0) + row * (axis ? w.sy : w.sx);
            for (int e = 0; e < taps; e++) dst[e] = roi_area_weight(rec, e);
        }
        __syncthreads(); // (wave-uniform branch: every lane of the workgroup is here)
    }
    if (!active) return;
    GlobalSrc gs;
    tile_global_src(gs, r, plane_y, plane_uv);
    if (down) {
        if (STAGED && staged) area_thread_tile<OUT, VEC, EL>(ls, d, w, L.spec, out, i0, j0);
        else area_thread_tile<OUT, VEC, EL>(gs, d, w, L.spec, out, i0, j0);
    } else if constexpr (EL == EL_LIB) {
        if (STAGED && staged) convert_thread_tile<M_AREA_UP, OUT, VEC>(ls, d, out, i0, j0);
        else convert_thread_tile<M_AREA_UP, OUT, VEC>(gs, d, out, i0, j0);
    } else {
        if (STAGED && staged) tensor_thread_tile<M_AREA_UP, OUT, VEC, EL>(ls, d, L.spec, (uint8_t *)out, i0, j0);
        else tensor_thread_tile<M_AREA_UP, OUT, VEC, EL>(gs, d, L.spec, (uint8_t *)out, i0, j0);
    }
}

} // namespace tsvpp
