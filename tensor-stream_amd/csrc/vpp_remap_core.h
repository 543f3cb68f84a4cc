// vpp_remap_core.h -- the coordinate-map kernel itself (see vpp_remap.hip for what it does), as a template that two translation units instantiate: vpp_remap.hip
// with the library's colour back end (EL_LIB: every flavour of tsvpp_convert_remap) and vpp_remap_tensor.hip with the tensor store (EL_F32 / EL_HALF:
// tsvpp_convert_remap_tensor, vpp_tensor_store.h).  Nothing but the store call differs between them.
//
// The kernel function is a template over a small policy -- the launch block and load(), which fills a thread tile's coordinates: RemapCoordLoad below READS
// them (remap_load), MeshCoordLoad (vpp_mesh_core.h) COMPUTES them from control points (mesh_load).  Everything else is stated once for both calls.
//
// A thread's coordinates are read once -- the eight map entries of its 4 x 2 thread tile, 32 contiguous bytes per row, which also give its two chroma pairs --
// clamped once, and kept in registers (20 values) across the footprint reduction and the staging barrier.  From the clamped coordinate on the sampler is the
// affine kernel's (warp_luma / warp_chroma, vpp_warp_core.h).
#pragma once
#include "vpp_warp_core.h"
#include "vpp_remap.h"

#pragma clang fp contract(off)

namespace tsvpp {

// the clamped coordinates of one thread tile: luma per pixel, chroma per pair
struct RemapCoords {
    float x[PXH][PXW], y[PXH][PXW];
    float cx[2], cy[2];
};

// From the entries of a thread tile to its coordinates: the chroma pairs from the UNCLAMPED luma entries, then THE clamp.  Whoever fills ex / ey -- a map that
// is read (remap_load), a control grid that is interpolated (mesh_load, vpp_mesh_core.h) -- everything behind the entries is this function.
template <bool VEC> __device__ __forceinline__ void remap_coords(const float (&ex)[PXH][PXW], const float (&ey)[PXH][PXW], int dst_w, int src_w, int src_h, int j0, RemapCoords &c) {
    const int cw = src_w >> 1, ch = src_h >> 1;
#pragma unroll
    for (int p = 0; p < 2; p++) {
        c.cx[p] = remap_clamp(remap_chroma(ex[0][2 * p], ex[0][2 * p + 1], ex[1][2 * p], ex[1][2 * p + 1]), cw);
        c.cy[p] = remap_clamp(remap_chroma(ey[0][2 * p], ey[0][2 * p + 1], ey[1][2 * p], ey[1][2 * p + 1]), ch);
    }
    if (!VEC && dst_w - j0 < PXW) { // the second pair does not exist: it is sampled where the first one is, and never stored
        c.cx[1] = c.cx[0];
        c.cy[1] = c.cy[0];
    }
#pragma unroll
    for (int rr = 0; rr < PXH; rr++)
#pragma unroll
        for (int k = 0; k < PXW; k++) {
            c.x[rr][k] = remap_clamp(ex[rr][k], src_w);
            c.y[rr][k] = remap_clamp(ey[rr][k], src_h);
        }
}

// Map entries of the thread tile at output (i0, j0), clamped.  Row and column indices are clamped into the output, so no load leaves dst_h rows x 8 * dst_w bytes
// of the map whatever the thread: a lane without pixels reads entries of others (and takes no part in the reduction), a column that does not exist (element-wise
// flavour, 4 k + 2 columns) repeats the row's last one, as the samplers of the other tile kernels do.
template <bool VEC> __device__ __forceinline__ void remap_load(const uint8_t *xy, int map_pitch, int dst_w, int dst_h, int src_w, int src_h, int i0, int j0, RemapCoords &c) {
    static_assert(PXH == 2 && PXW == 4, "a thread tile holds two chroma pairs, each a 2 x 2 block of map entries");
    struct __attribute__((aligned(8))) Row { float v[2 * PXW]; }; // four entries: 32 contiguous bytes, 8-byte aligned
    const int ic = min(i0, dst_h - PXH); // (dst_h is even, i0 is even)
    float ex[PXH][PXW], ey[PXH][PXW];
#pragma unroll
    for (int rr = 0; rr < PXH; rr++) {
        const uint8_t *row = xy + (size_t)(ic + rr) * (size_t)map_pitch;
        if constexpr (VEC) { // every thread tile has its four columns (dst_w >= 4)
            const Row e = *(const Row *)(row + 8 * (size_t)min(j0, dst_w - PXW));
#pragma unroll
            for (int k = 0; k < PXW; k++) {
                ex[rr][k] = e.v[2 * k];
                ey[rr][k] = e.v[2 * k + 1];
            }
        } else {
#pragma unroll
            for (int k = 0; k < PXW; k++) {
                const float2 e = *(const float2 *)(row + 8 * (size_t)min(j0 + k, dst_w - 1));
                ex[rr][k] = e.x;
                ey[rr][k] = e.y;
            }
        }
    }
    remap_coords<VEC>(ex, ey, dst_w, src_w, src_h, j0, c);
}

// ---- the footprint reduction: min / max over the workgroup's 128 lanes -------------------------------------------------------------------------------------
// Within a row of 16 lanes by data-parallel primitives (quad permutes, then the two row mirrors: after each step every lane of the group holds the group's
// extreme), across the four rows of the wave by two exchanges, across the two waves through REMAP_REDUCE_LDS bytes.
template <int CTRL> __device__ __forceinline__ float remap_dpp(float v) {
    const int b = __builtin_bit_cast(int, v);
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(b, b, CTRL, 0xf, 0xf, false));
}
template <bool MAX> __device__ __forceinline__ float remap_pick(float a, float b) { return MAX ? fmaxf(a, b) : fminf(a, b); }
template <bool MAX> __device__ __forceinline__ float remap_wave_extreme(float v) {
    v = remap_pick<MAX>(v, remap_dpp<0xB1>(v));  // quad_perm [1, 0, 3, 2]
    v = remap_pick<MAX>(v, remap_dpp<0x4E>(v));  // quad_perm [2, 3, 0, 1]
    v = remap_pick<MAX>(v, remap_dpp<0x141>(v)); // row_half_mirror
    v = remap_pick<MAX>(v, remap_dpp<0x140>(v)); // row_mirror
    v = remap_pick<MAX>(v, __shfl_xor(v, 16));
    v = remap_pick<MAX>(v, __shfl_xor(v, 32));
    return v;
}
__device__ __forceinline__ float remap_uniform(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); }

// The extremes of the clamped coordinates of the workgroup's pixels and pairs that exist.  Every lane of the workgroup calls it (one barrier inside); a lane
// without pixels contributes the neutral elements.  The result is wave-uniform and held in scalar registers.
__device__ __forceinline__ RemapExtremes remap_reduce(const RemapCoords &c, bool active, float (*red)[8]) {
    float lo[4] = { c.x[0][0], c.y[0][0], c.cx[0], c.cy[0] }, hi[4] = { c.x[0][0], c.y[0][0], c.cx[0], c.cy[0] };
#pragma unroll
    for (int rr = 0; rr < PXH; rr++)
#pragma unroll
        for (int k = 0; k < PXW; k++) {
            lo[0] = fminf(lo[0], c.x[rr][k]);
            hi[0] = fmaxf(hi[0], c.x[rr][k]);
            lo[1] = fminf(lo[1], c.y[rr][k]);
            hi[1] = fmaxf(hi[1], c.y[rr][k]);
        }
    lo[2] = fminf(lo[2], c.cx[1]);
    hi[2] = fmaxf(hi[2], c.cx[1]);
    lo[3] = fminf(lo[3], c.cy[1]);
    hi[3] = fmaxf(hi[3], c.cy[1]);
    float v[8];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        v[2 * q] = remap_wave_extreme<false>(active ? lo[q] : __builtin_inff());
        v[2 * q + 1] = remap_wave_extreme<true>(active ? hi[q] : -__builtin_inff());
    }
    const int wave = (int)(threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 8; q++) red[wave][q] = v[q];
    }
    __syncthreads();
    static_assert(ROI_THREADS == 128, "two waves");
#pragma unroll
    for (int q = 0; q < 8; q++) v[q] = remap_uniform((q & 1) ? fmaxf(red[0][q], red[1][q]) : fminf(red[0][q], red[1][q]));
    return RemapExtremes{ v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7] };
}

// convert_thread_tile (vpp_device.h) with the map's coordinates: 2 x 4 luma samples and 2 chroma pairs of the virtual NV12 frame, then the one colour back end
// (LT: the launch block that carries the border sample and the tensor spec -- RemapLaunch, or MeshLaunch of vpp_mesh.h)
template <int OUT, bool VEC, bool BORDER, int EL, class S, class LT>
__device__ __forceinline__ void remap_thread_tile(const S &s, const LaunchDesc &d, const LT &L, const RemapCoords &c, typename OutT<OUT>::type *out, int i0, int j0) {
    const int ncol = VEC ? PXW : min(PXW, d.dst_w - j0);
    float Uf[2] = { 128.0f, 128.0f }, Vf[2] = { 128.0f, 128.0f }, Yf[PXH][PXW];
    if constexpr (!kLumaOnly<OUT>) {
#pragma unroll
        for (int p = 0; p < 2; p++) warp_chroma<BORDER>(s, c.cx[p], c.cy[p], L.border_u, L.border_v, Uf[p], Vf[p]);
    }
#pragma unroll
    for (int rr = 0; rr < PXH; rr++) {
        __builtin_amdgcn_sched_barrier(0); // the chroma pairs, then one luma row at a time (warp_thread_tile: the taps of a whole thread tile in flight cost VGPRs)
#pragma unroll
        for (int k = 0; k < PXW; k++) Yf[rr][k] = warp_luma<BORDER>(s, c.x[rr][k], c.y[rr][k], L.border_y);
    }
    store_tile<OUT, VEC, EL>(Yf, Uf, Vf, d, L.spec, out, i0, j0, ncol);
}

// The coordinate-map call's policy: the coordinates of the thread tile at output (i0, j0) of record r are map entries
struct RemapCoordLoad {
    using Launch = RemapLaunch;
    template <bool VEC> static __device__ __forceinline__ void load(const RemapRec &r, const uint8_t *xy, int dst_w, int dst_h, int i0, int j0, RemapCoords &c) {
        remap_load<VEC>(xy, r.map_pitch, dst_w, dst_h, r.src_w, r.src_h, i0, j0, c);
    }
};

// The kernel of both calls: COORD is RemapCoordLoad or MeshCoordLoad (vpp_mesh_core.h).  An earlier attempt with the body behind a common FUNCTION changed the
// dense kernels' register allocation; as a template over the policy the mesh kernels compile to the same instruction lines as the two functions did, and the
// dense kernels to the same opcode sequence with two scalar registers exchanged in 50 lines (profiles/coord_paths_resources.txt).
// (launch bounds: at least four waves per SIMD, i.e. at most 128 VGPRs, as the affine kernel's: profiles/remap_resources.txt, profiles/mesh_resources.txt)
template <class COORD, int OUT, bool VEC, bool STAGED, bool BORDER, int EL = EL_LIB>
__global__ __launch_bounds__(ROI_THREADS, 4) void vpp_coord_map_kernel(const typename COORD::Launch L) {
    using T = typename OutT<OUT>::type;
    typedef __attribute__((address_space(1))) uint8_t *GP; // the records hold GLOBAL addresses (PtrCol, vpp_kernels.h)
    const TileIndex tix = tile_index(L.tiles_x, L.tiles_y);
    const int item = tix.item, tyi = tix.tyi, txi = tix.txi;
    if (item >= L.n) return;
    const auto &r = L.r[item]; // wave-uniform index: scalar loads

    // the colour back end and the staging loop read their request from a LaunchDesc (the samplers' fields stay zero: the map, or the mesh, is the sampler)
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
    const uint8_t *const map_xy = (const uint8_t *)(GP)(uintptr_t)r.xy;
    T *const out = (T *)(GP)(uintptr_t)r.out;
    const int lx = threadIdx.x & (ROI_TX - 1), ly = threadIdx.x >> ROI_TX_SHIFT;
    const int j_first = roi_tile_col0(txi, L.dst_w, d.last_col0), i_first = tyi * ROI_TILE_H;
    const int j0 = j_first + lx * PXW, i0 = i_first + ly * PXH;
    const bool active = j0 < L.dst_w && i0 < L.dst_h && !(VEC && is_row_tail(d, j0));

    RemapCoords c;
    COORD::template load<VEC>(r, map_xy, L.dst_w, L.dst_h, i0, j0, c);

    if constexpr (STAGED) {
        // the tile's source bounding box, from the extremes of its own coordinates (remap_footprint: the function tsvpp_remap_footprint evaluates on the host; a
        // mesh's are those of its expanded map E(mesh))
        __shared__ float red[2][8];
        static_assert(sizeof(red) == REMAP_REDUCE_LDS, "the budget accounts for the reduction's words");
        const RemapExtremes e = remap_reduce(c, active, red);
        RoiFootprint f;
        remap_footprint(e, r.src_w, r.src_h, f);
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
            if (active) remap_thread_tile<OUT, VEC, BORDER, EL>(s, d, L, c, out, i0, j0);
            return;
        }
    }
    if (!active) return;
    GlobalSrc s;
    tile_global_src(s, r, plane_y, plane_uv);
    remap_thread_tile<OUT, VEC, BORDER, EL>(s, d, L, c, out, i0, j0);
}

// The path's tag for launch_coord / launch_coord_tensor (vpp_tile_launch.h)
struct RemapKernels {
    using Launch = RemapLaunch;
    static constexpr const char *kName = "vpp_remap";
    template <int OUT, bool VEC, bool STAGED, bool BORDER, int EL> static constexpr auto kernel() { return &vpp_coord_map_kernel<RemapCoordLoad, OUT, VEC, STAGED, BORDER, EL>; }
};

} // namespace tsvpp
