// vpp_tensor_store.h -- the output side of the tensor entry points (tsvpp_convert_rois_tensor, tsvpp_convert_letterbox_tensor; include/tsvpp.h): what a network
// takes instead of what the reference returns.  tensor_store_tile stands next to color_store_tile (vpp_device.h): the same inputs -- the resized samples of a
// 2 x 4 thread tile as integer-valued floats -- and the same arithmetic up to the normalised fp32 value q = k / 255 (chroma_terms, trunc_clamp255, norm255,
// unchanged), then, per stored channel c,
//     v = (q - mean[c]) * scale[c]          two packed fp32 operations, each rounded once, nothing fused
// and ONE conversion per pair of values to the element type (fp16 / bf16: round to nearest even, v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32 -- plain casts; the
// round-toward-zero pack builtin would be wrong here), one 8-byte (half) or 16-byte (fp32) store per row per plane from the uniform plane base with a 32-bit
// byte offset per lane, as st4o.  Planar RGB / BGR (NCHW) and Y800 only.  The element-wise flavour (outputs that are not 16-byte aligned, outputs narrower than
// a tile with 4 k + 2 columns) stores element by element; which thread tiles exist and where the last tile column starts depends on columns, not on the
// element size: the rules are color_store_tile's.
//
// mean / scale / dtype are the launch's (RoiLaunch::spec, LbLaunch::spec): wave-uniform, read with scalar loads out of the kernarg segment.  fp16 and bf16 share
// ONE instantiation (EL_HALF) that branches on the launch's dtype -- a scalar branch around the conversions and stores of a tile -- which keeps the kernel count
// of the three tensor translation units at two thirds of what a dtype template parameter would make it; fp32 (EL_F32) has its own because its stores differ.
#pragma once
#include "vpp_device.h"

#pragma clang fp contract(off)

namespace tsvpp {

typedef _Float16 tensor_h2 __attribute__((ext_vector_type(2)));
typedef __bf16 tensor_b2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f2 tensor_affine(f2 q, float mean, float scale) {
    const f2 v = q - (f2){ mean, mean };
    return v * (f2){ scale, scale };
}
// two values -> one dword of two 2-byte elements (DT: TSVPP_F16 | TSVPP_BF16), the first in the low half
template <int DT> __device__ __forceinline__ uint32_t tensor_cvt_pair(f2 v) {
    if constexpr (DT == TSVPP_F16) return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, tensor_h2));
    else return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, tensor_b2));
}

// Four values of one row of one plane (pairs a, b), converted and stored at element `pix` of the plane that starts at `base` (wave-uniform).
template <int DT, bool VEC> __device__ __forceinline__ void tensor_store4(uint8_t *base, uint32_t pix, f2 a, f2 b, int ncol, int nt) {
    if constexpr (DT == TSVPP_F32) {
        if constexpr (VEC) st4o(base, pix * 4u, a.x, a.y, b.x, b.y, nt);
        else {
            const float v[4] = { a.x, a.y, b.x, b.y };
            float *o = (float *)base;
            for (int c = 0; c < ncol; c++) o[pix + c] = v[c];
        }
    } else {
        const uint32_t lo = tensor_cvt_pair<DT>(a), hi = tensor_cvt_pair<DT>(b);
        if constexpr (VEC) {
            if (nt) st8_nt(base, pix * 2u, lo, hi, nt); // (the hint as inline asm: see st8_nt)
            else *(nt_u32x2 *)(base + pix * 2u) = (nt_u32x2){ lo, hi };
        } else {
            uint16_t *o = (uint16_t *)base;
            for (int c = 0; c < ncol; c++) o[pix + c] = (uint16_t)((c < 2 ? lo : hi) >> (16 * (c & 1)));
        }
    }
}

template <int OUT, int DT, bool VEC>
__device__ __forceinline__ void tensor_store_tile_dt(const float Yf[PXH][PXW], const float Uf[2], const float Vf[2], const LaunchDesc &d, const tsvpp_tensor_spec &a,
                                                     uint8_t *out, int i0, int j0, int ncol) {
    constexpr uint32_t ESZ = DT == TSVPP_F32 ? 4u : 2u;
    const int nt = d.nt_stores;
    if constexpr (kLumaOnly<OUT>) { // Y800: the resized samples themselves, / 255
#pragma unroll
        for (int r = 0; r < PXH; r++) {
            const uint32_t pix = (uint32_t)(i0 + r) * (uint32_t)d.dst_w + (uint32_t)j0;
            const f2 p0 = tensor_affine(norm255((f2){ Yf[r][0], Yf[r][1] }), a.mean[0], a.scale[0]);
            const f2 p1 = tensor_affine(norm255((f2){ Yf[r][2], Yf[r][3] }), a.mean[0], a.scale[0]);
            tensor_store4<DT, VEC>(out, pix, p0, p1, ncol, nt);
        }
    } else {
        float t0[2], tg[2], t2[2];
#pragma unroll
        for (int c = 0; c < 2; c++) chroma_terms(Uf[c], Vf[c], d.k, d.swap_rb, d.color_g, t0[c], tg[c], t2[c]);
        // uniform plane bases + one 32-bit offset per lane (the host guarantees 3 * W * H * 4 < 4 GiB)
        const size_t plane_bytes = (size_t)((uint32_t)d.dst_w * (uint32_t)d.dst_h) * ESZ;
        uint8_t *const b0 = out, *const b1 = out + plane_bytes, *const b2 = out + 2 * plane_bytes;
#pragma unroll
        for (int r = 0; r < PXH; r++) {
            const uint32_t pix = (uint32_t)(i0 + r) * (uint32_t)d.dst_w + (uint32_t)j0;
            f2 c0[2], c1[2], c2[2];
#pragma unroll
            for (int p = 0; p < 2; p++) {
                f2 y = { Yf[r][2 * p], Yf[r][2 * p + 1] };
                y = y - (f2){ d.k.y_offset, d.k.y_offset };
                y.x = __builtin_fmaxf(0.0f, y.x);
                y.y = __builtin_fmaxf(0.0f, y.y);
                y = y * (f2){ d.k.y_scale, d.k.y_scale };
                c0[p] = tensor_affine(norm255(trunc_clamp255(y + (f2){ t0[p], t0[p] })), a.mean[0], a.scale[0]);
                c1[p] = tensor_affine(norm255(trunc_clamp255(y + (f2){ tg[p], tg[p] })), a.mean[1], a.scale[1]);
                c2[p] = tensor_affine(norm255(trunc_clamp255(y + (f2){ t2[p], t2[p] })), a.mean[2], a.scale[2]);
            }
            tensor_store4<DT, VEC>(b0, pix, c0[0], c0[1], ncol, nt);
            tensor_store4<DT, VEC>(b1, pix, c1[0], c1[1], ncol, nt);
            tensor_store4<DT, VEC>(b2, pix, c2[0], c2[1], ncol, nt);
        }
    }
}

// OUT: O_F32_PLANAR or O_Y800_F32 (what the samplers and the launch geometry see: three planes or one); EL: EL_F32 | EL_HALF (vpp_kernels.h)
template <int OUT, int EL, bool VEC>
__device__ __forceinline__ void tensor_store_tile(const float Yf[PXH][PXW], const float Uf[2], const float Vf[2], const LaunchDesc &d, const tsvpp_tensor_spec &a,
                                                  uint8_t *out, int i0, int j0, int ncol) {
    static_assert(OUT == O_F32_PLANAR || OUT == O_Y800_F32, "tensor outputs are planar RGB / BGR or Y800");
    static_assert(EL == EL_F32 || EL == EL_HALF, "tensor element");
    if constexpr (EL == EL_F32) tensor_store_tile_dt<OUT, TSVPP_F32, VEC>(Yf, Uf, Vf, d, a, out, i0, j0, ncol);
    else if (a.dtype == TSVPP_F16) tensor_store_tile_dt<OUT, TSVPP_F16, VEC>(Yf, Uf, Vf, d, a, out, i0, j0, ncol); // (wave-uniform)
    else tensor_store_tile_dt<OUT, TSVPP_BF16, VEC>(Yf, Uf, Vf, d, a, out, i0, j0, ncol);
}

// How a kernel with both kinds of instantiation chooses -- ONE pattern in vpp_rois_core.h, vpp_rois_area_core.h and vpp_letterbox_core.h: the kernel keeps its typed
// output pointer and, at each place it used to reach the colour back end, writes
//     if constexpr (EL == EL_LIB) <the call it always made, word for word>;   else <the tensor call with (uint8_t *)out>;
// The ROI kernels reach the back end through convert_thread_tile (vpp_device.h: sampling and store in one function that every kernel of the library shares), so
// their tensor call is tensor_thread_tile below; the letterbox and the AREA thread tiles sample themselves and call color_store_tile, so theirs is
// tensor_store_tile.  There is deliberately no wrapper that hides the choice: the EL_LIB instantiations must compile to the code they compiled to before
// (profiles/tensor_resources.txt has the comparison and what a wrapper did to it).

// convert_thread_tile (vpp_device.h) for the tensor instantiations: the same samples, the tensor store.  KEEP IN STEP with convert_thread_tile: the sampling loop
// is a copy, because splitting convert_thread_tile into a sampling and a storing half changed the registers of kernels all over the library.
template <int MODE, int OUT, bool VEC, int EL, class S>
__device__ __forceinline__ void tensor_thread_tile(const S &s, const LaunchDesc &d, const tsvpp_tensor_spec &a, uint8_t *out, int i0, int j0) {
    const int ncol = VEC ? PXW : min(PXW, d.dst_w - j0);
    const int ci = i0 >> 1, cj0 = j0 >> 1, jmax = d.dst_w - 1, cjmax = (d.dst_w >> 1) - 1;
    float Uf[2], Vf[2], Yf[PXH][PXW];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        int U = 128, V = 128;
        if constexpr (!kLumaOnly<OUT>) sample_chroma<MODE>(s, d, ci, VEC ? cj0 + c : min(cj0 + c, cjmax), U, V);
        Uf[c] = (float)U;
        Vf[c] = (float)V;
    }
#pragma unroll
    for (int r = 0; r < PXH; r++)
#pragma unroll
        for (int c = 0; c < PXW; c++) Yf[r][c] = (float)sample_luma<MODE>(s, d, i0 + r, VEC ? j0 + c : min(j0 + c, jmax));
    tensor_store_tile<OUT, EL, VEC>(Yf, Uf, Vf, d, a, out, i0, j0, ncol);
}

} // namespace tsvpp
