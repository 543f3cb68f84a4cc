// vpp_rois.hip -- many regions of interest, each resized to ONE output size, in one launch (tsvpp_convert_rois, include/tsvpp.h).
//
// The output side is uniform -- every box becomes dst_w x dst_h -- so a workgroup finds its (box, output tile) with one division and stores its tile through the
// library's colour back end (color_store_tile: vector stores for 16-byte aligned outputs, element-wise stores otherwise, the shifted last tile column for widths
// 4 k + 2).  What differs per box -- plane origins, pitches, size, ratios, output pointer -- is a 48-byte record indexed by the workgroup's box: wave-uniform, read
// with scalar loads out of the kernarg segment, never re-derived per lane.  The per-pixel arithmetic is the shared samplers' (vpp_device.h: coordinates from
// vpp_axis.h, bilerp, the mixed-precision cubic with its tie test); this file adds the per-box geometry around them.
//
// Source side: a tile's footprint is small and neighbouring lanes tap overlapping bytes, so the workgroup stages the luma and chroma footprints of its tile in LDS
// with 16-byte loads (stage_planes) and samples through LdsSrc.  The footprint follows from the box's ratios, i.e. it differs per box: it is computed in the
// kernel from wave-uniform values (roi_span_x / roi_span_y: the numbers the host sized the launch's LDS with), and a tile whose footprint does not fit the
// launch's LDS -- a large box against the LDS budget -- gathers its taps from global memory instead (GlobalSrc), a wave-uniform branch.
//
// Arithmetic contract as everywhere: single IEEE-754 operations in the reference's order, contraction off; the only fused operations are the explicit ones of the
// shared samplers.  Written for wave64 / CDNA4 only.

#include "vpp_device.h"
#include "vpp_rois.h"

#pragma clang fp contract(off)

namespace tsvpp {

template <int MODE, int OUT, bool VEC, bool STAGED>
__global__ __launch_bounds__(ROI_THREADS) void vpp_rois_kernel(const RoiLaunch L) {
    using T = typename OutT<OUT>::type;
    typedef __attribute__((address_space(1))) uint8_t *GP; // the records hold GLOBAL addresses (PtrCol, vpp_kernels.h)
    // workgroup -> (box, tile): all tiles of a box are neighbours in the grid, so the lines that adjacent tiles share meet in L2
    const int tiles = L.tiles_x * L.tiles_y;
    const int box = (int)blockIdx.x / tiles;
    const int rem = (int)blockIdx.x - box * tiles;
    const int tyi = rem / L.tiles_x, txi = rem - tyi * L.tiles_x;
    if (box >= L.n_rois) return;
    const RoiRec &r = L.r[box]; // wave-uniform index: scalar loads

    // the samplers and the colour back end read their request from a LaunchDesc: this box's
    LaunchDesc d = {};
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

    const uint8_t *const plane_y = (const uint8_t *)(GP)(uintptr_t)r.y, *const plane_uv = (const uint8_t *)(GP)(uintptr_t)r.uv;
    T *const out = (T *)(GP)(uintptr_t)r.out;
    const int lx = threadIdx.x & (ROI_TX - 1), ly = threadIdx.x >> ROI_TX_SHIFT;
    const int j_first = roi_tile_col0(txi, L.dst_w, d.last_col0), i_first = tyi * ROI_TILE_H;
    const int j0 = j_first + lx * PXW, i0 = i_first + ly * PXH;
    const bool active = j0 < L.dst_w && i0 < L.dst_h && !(VEC && is_row_tail(d, j0));

    if constexpr (STAGED) {
        RoiFootprint f;
        roi_span_x(MODE, j_first, L.dst_w, r.src_w, r.xr, f);
        roi_span_y(MODE, i_first, L.dst_h, r.src_h, r.yr, f);
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
            // two luma + one chroma chunk per lane in flight per round.  More was measured and not kept: with 16 + 8 in flight a single 112 x 112 box (16 tiles of up to
            // 36 KiB) went from 6.8 to 6.4 us, but the kernels grew from ~100 to 186 VGPRs and a 224 x 224 box (49 small tiles) from 5.1 to 6.1 us, 64 of them from 15.8 to 22 us
            stage_planes<2, 1>(d, lds_y, ay, s.py_, ny, span_y, lds_uv, auv, s.puv_, nuv, span_uv, ROI_THREADS);
            __syncthreads();
            if (active) convert_thread_tile<MODE, OUT, VEC>(s, d, out, i0, j0);
            return;
        }
    }
    if (!active) return;
    GlobalSrc s;
    s.y = plane_y;
    s.uv = plane_uv;
    s.py = r.pitch_y;
    s.puv = r.pitch_uv;
    s.w = r.src_w;
    s.h = r.src_h;
    convert_thread_tile<MODE, OUT, VEC>(s, d, out, i0, j0);
}

namespace {

const char *const kModeNames[M_COUNT] = { "M_NONE", "M_NEAREST", "M_BILINEAR", "M_BICUBIC", "M_AREA_DOWN", "M_AREA_UP" };
const char *const kOutNames[O_COUNT] = { "O_U8_PLANAR", "O_U8_MERGED", "O_F32_PLANAR", "O_F32_MERGED", "O_NV12_U8", "O_NV12_F32", "O_Y800_U8", "O_Y800_F32", "O_HSV_F32" };

template <int MODE, int OUT, bool VEC, bool STAGED>
hipError_t launch_k(const RoiLaunch &L, unsigned grid, size_t lds, hipStream_t stream) {
    hipLaunchKernelGGL((vpp_rois_kernel<MODE, OUT, VEC, STAGED>), dim3(grid), dim3(ROI_THREADS), lds, stream, L);
    return hipGetLastError();
}
template <int MODE, int OUT>
hipError_t launch_mo(bool vec, bool staged, const RoiLaunch &L, unsigned grid, size_t lds, hipStream_t stream) {
    if (vec) return staged ? launch_k<MODE, OUT, true, true>(L, grid, lds, stream) : launch_k<MODE, OUT, true, false>(L, grid, 0, stream);
    return staged ? launch_k<MODE, OUT, false, true>(L, grid, lds, stream) : launch_k<MODE, OUT, false, false>(L, grid, 0, stream);
}
// the flavours this kernel is instantiated for: RGB / BGR planar and merged, Y800
constexpr bool roi_flavour(int out) { return out == O_U8_PLANAR || out == O_U8_MERGED || out == O_F32_PLANAR || out == O_F32_MERGED || out == O_Y800_U8 || out == O_Y800_F32; }
template <int MODE>
hipError_t launch_m(OutKind out, bool vec, bool staged, const RoiLaunch &L, unsigned grid, size_t lds, hipStream_t stream) {
    return with_out_kind(out, [&](auto O) {
        constexpr int OUT = decltype(O)::value;
        if constexpr (roi_flavour(OUT)) return launch_mo<MODE, OUT>(vec, staged, L, grid, lds, stream);
        else return hipErrorNotSupported; // a missing kernel is an error, never a fallback
    });
}

} // namespace

hipError_t launch_rois(Mode mode, OutKind out, bool vec, bool staged, const RoiLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                       size_t name_len, bool dry_run) {
    const bool known = (mode == M_NEAREST || mode == M_BILINEAR || mode == M_BICUBIC) && roi_flavour(out);
    if (!known) return hipErrorNotSupported;
    if (name && name_len) snprintf(name, name_len, "vpp_rois<%s,%s,%s,%s>", kModeNames[mode], kOutNames[out], vec ? "vec" : "elem", staged ? "staged" : "gather");
    if (dry_run) return hipSuccess;
    switch (mode) {
    case M_NEAREST: return launch_m<M_NEAREST>(out, vec, staged, L, grid, lds_bytes, stream);
    case M_BILINEAR: return launch_m<M_BILINEAR>(out, vec, staged, L, grid, lds_bytes, stream);
    default: return launch_m<M_BICUBIC>(out, vec, staged, L, grid, lds_bytes, stream);
    }
}

} // namespace tsvpp
