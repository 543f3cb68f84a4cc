// vpp_letterbox_p010_core.h -- the P010 letterbox kernel (see vpp_letterbox_p010.hip for what it does), as a template that two translation units instantiate:
// vpp_letterbox_p010.hip with the library's output flavours (EL_LIB) and vpp_letterbox_p010_tensor.hip with the tensor store (EL_F32 / EL_HALF).
//
// Called, not copied: the canvas grid (tile_index), the descriptor fill (tile_desc), the rectangle's part of a tile (tile_inner_range) and its footprint in samples
// (tile_span_x / tile_span_y), the shifted last tile column (roi_tile_col0), describe_plane and the LDS-DMA loop (stage_plane_dma), the blend (bilerp2), the
// chroma terms (chroma_terms, with the two offsets scaled by four), the byte packers and store primitives (pack_u8x12_rtz, pack_u8x4, st1o, st4o, st16_nt,
// merged_run) and the tensor conversion (tensor_affine, tensor_store4).
// Written out, because the shared piece would have to change and with it the instructions of the 8-bit kernels: the thread tile (letterbox_thread_tile ends in the
// 8-bit store and samples through sample_luma / sample_chroma, which mask to a byte), and the row stores behind the channel values (color_store_row and
// tensor_store_tile_dt clamp to 255 and divide by 255 in their middle).  Their structure is kept: pad outside the rectangle per chroma pair, taps clamped into the
// part of the rectangle the workgroup's tile covers, the lanes of a run exchanging merged rows through LDS.
#pragma once
#include "vpp_letterbox_p010.h"
#include "vpp_letterbox_core.h"

#pragma clang fp contract(off)

namespace tsvpp {

// ---- source readers: 16-bit words, the sample in the ten high bits -----------------------------------------------------------------------------------------
// Y2: the words of luma samples (row, x) and (row, x + xd) in one register, low half first.  UV: the (U, V) words of chroma pair (row, cx), U in the low half --
// ONE dword read where every pair of the plane is 4-byte aligned (`uv4`: plane address and pitch are, wave-uniform), two 16-bit reads otherwise.
__device__ __forceinline__ uint32_t p010_words(const uint8_t *p, int step) {
    return (uint32_t) * (const uint16_t *)p | (uint32_t) * (const uint16_t *)(p + step) << 16;
}
__device__ __forceinline__ uint32_t p010_pair(const uint8_t *p, bool uv4) { return uv4 ? *(const uint32_t *)p : p010_words(p, 2); }

struct P010Global {
    const uint8_t *y, *uv;
    int py, puv; // pitches in bytes
    int w, h;    // the frame in luma samples
    bool uv4;
    // (coordinates are clamped into the frame so that no input can fault; for every valid request the clamps never fire)
    __device__ __forceinline__ uint32_t Y2(int row, int x, int xd) const {
        row = min(max(row, 0), h - 1);
        x = min(max(x, 0), w - 1 - xd);
        return p010_words(y + (uint32_t)row * (uint32_t)py + 2u * (uint32_t)x, 2 * xd);
    }
    __device__ __forceinline__ uint32_t UV(int row, int cx) const {
        row = min(max(row, 0), (h >> 1) - 1);
        cx = min(max(cx, 0), (w >> 1) - 1);
        return p010_pair(uv + (uint32_t)row * (uint32_t)puv + 4u * (uint32_t)cx, uv4);
    }
};
// The staged footprint: LdsPlane (vpp_device.h) with byte columns -- x0 is 2 * the first luma sample, 4 * the first chroma pair
struct P010Lds {
    LdsPlane py_, puv_;
    int w, h;
    bool uv4;
    __device__ __forceinline__ static const uint8_t *at(const LdsPlane &lp, int row, int bytecol) {
        const int r = row - lp.y0;
        return lp.base + r * lp.lp + ((lp.m0 + r * lp.pm) & 15) + (bytecol - lp.x0);
    }
    __device__ __forceinline__ uint32_t Y2(int row, int x, int xd) const { return p010_words(at(py_, row, 2 * x), 2 * xd); }
    __device__ __forceinline__ uint32_t UV(int row, int cx) const { return p010_pair(at(puv_, row, 4 * cx), uv4); }
};
// the contract's `word >> 6` of either half: v_bfe_u32 (w, 6, 10) / (w, 22, 10) -- the six low bits drop out by construction
__device__ __forceinline__ float p010_lo(uint32_t w) { return (float)((w >> 6) & 1023u); }
__device__ __forceinline__ float p010_hi(uint32_t w) { return (float)(w >> 22); }

// ---- sampling ------------------------------------------------------------------------------------------------------------------------------------------------
// One axis of one output index: first tap, step to the second tap (0 at the edge), weight.  The formulas and edge rules are sample_luma's / sample_chroma's
// (vpp_device.h) word for word; `limit` is what bilinear_axis clamps to, `taps` the samples the second tap may not leave (chroma columns: pairs, counted as
// 2 * p + 2 >= w there).
struct P010Tap {
    int p, step;
    float w;
};
template <int MODE> __device__ __forceinline__ P010Tap p010_axis(int idx, float ratio, int limit, int taps) {
    P010Tap t;
    if constexpr (MODE == M_NEAREST) {
        t.p = (int)(ratio * (float)idx);
        t.step = 0;
        t.w = 0.0f;
    } else {
        bilinear_axis(idx, ratio, limit, t.p, t.w);
        t.step = (t.p + 1 >= taps) ? 0 : 1;
    }
    return t;
}

// letterbox_thread_tile (vpp_letterbox_core.h) for 16-bit sources: the canvas thread tile at (i0, j0) samples at the inner coordinates, clamped into the part of
// the rectangle its workgroup's tile covers; a chroma pair outside the rectangle takes the pad sample.  The axis terms are computed once per column / row of the
// thread tile; U and V share their weights and run as one pair through bilerp2, luma columns pair up the same way (packed arithmetic is switched off for these
// translation units -- csrc/Makefile -- so each half is its own scalar operation, in the contract's order either way).
template <int MODE, int OUT, bool VEC, class S>
__device__ __forceinline__ void p010_sample_tile(const S &s, const LbRec &r, const LbPart &t, const LbLaunch &L, int i0, int j0, float Yf[PXH][PXW], float Uf[2],
                                                 float Vf[2]) {
    const float pad_y = L.pad_y, pad_u = L.pad_u, pad_v = L.pad_v;
    const bool rows_in = i0 >= r.top && i0 < r.top + r.height;
    bool in[2];
#pragma unroll
    for (int c = 0; c < 2; c++) in[c] = rows_in && j0 + 2 * c >= r.left && j0 + 2 * c < r.left + r.width;
#pragma unroll
    for (int c = 0; c < 2; c++) {
        Uf[c] = pad_u;
        Vf[c] = pad_v;
    }
#pragma unroll
    for (int rr = 0; rr < PXH; rr++)
#pragma unroll
        for (int c = 0; c < PXW; c++) Yf[rr][c] = pad_y;
    if (!(in[0] || in[1])) return; // a thread tile wholly outside the rectangle samples nothing
    if constexpr (!kLumaOnly<OUT>) {
        const int ci = clampi((i0 - r.top) >> 1, t.b0 >> 1, t.b1 >> 1), cj0 = (j0 - r.left) >> 1;
        const P010Tap ty = p010_axis<MODE>(ci, r.yr, s.h, s.h >> 1);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            P010Tap tx = p010_axis<MODE>(clampi(cj0 + c, t.a0 >> 1, t.a1 >> 1), r.xr, s.w, 0);
            if constexpr (MODE != M_NEAREST) tx.step = (2 * tx.p + 2 >= s.w) ? 0 : 1;
            f2 uv;
            if constexpr (MODE == M_NEAREST) {
                const uint32_t a = s.UV(ty.p, tx.p);
                uv = (f2){ p010_lo(a), p010_hi(a) };
            } else {
                const uint32_t a = s.UV(ty.p, tx.p), b = s.UV(ty.p, tx.p + tx.step), cc = s.UV(ty.p + ty.step, tx.p), dd = s.UV(ty.p + ty.step, tx.p + tx.step);
                const f2 wx = { tx.w, tx.w }, wy = { ty.w, ty.w };
                uv = trunc2(bilerp2((f2){ p010_lo(a), p010_hi(a) }, (f2){ p010_lo(b), p010_hi(b) }, (f2){ p010_lo(cc), p010_hi(cc) }, (f2){ p010_lo(dd), p010_hi(dd) }, wx,
                                    (f2){ 1.0f, 1.0f } - wx, wy, (f2){ 1.0f, 1.0f } - wy));
            }
            Uf[c] = in[c] ? uv.x : pad_u;
            Vf[c] = in[c] ? uv.y : pad_v;
        }
    }
    P010Tap tx[PXW];
#pragma unroll
    for (int c = 0; c < PXW; c++) tx[c] = p010_axis<MODE>(clampi(j0 - r.left + c, t.a0, t.a1), r.xr, s.w, s.w);
#pragma unroll
    for (int rr = 0; rr < PXH; rr++) {
        const P010Tap ty = p010_axis<MODE>(clampi(i0 - r.top + rr, t.b0, t.b1), r.yr, s.h, s.h);
#pragma unroll
        for (int c = 0; c < PXW; c += 2) {
            f2 v;
            if constexpr (MODE == M_NEAREST) {
                v = (f2){ p010_lo(s.Y2(ty.p, tx[c].p, 0)), p010_lo(s.Y2(ty.p, tx[c + 1].p, 0)) };
            } else {
                // taps A / B and C / D of a column are neighbouring words: one register each
                const uint32_t ab0 = s.Y2(ty.p, tx[c].p, tx[c].step), cd0 = s.Y2(ty.p + ty.step, tx[c].p, tx[c].step);
                const uint32_t ab1 = s.Y2(ty.p, tx[c + 1].p, tx[c + 1].step), cd1 = s.Y2(ty.p + ty.step, tx[c + 1].p, tx[c + 1].step);
                const f2 wx = { tx[c].w, tx[c + 1].w }, wy = { ty.w, ty.w };
                v = trunc2(bilerp2((f2){ p010_lo(ab0), p010_lo(ab1) }, (f2){ p010_hi(ab0), p010_hi(ab1) }, (f2){ p010_lo(cd0), p010_lo(cd1) },
                                   (f2){ p010_hi(cd0), p010_hi(cd1) }, wx, (f2){ 1.0f, 1.0f } - wx, wy, (f2){ 1.0f, 1.0f } - wy));
            }
            Yf[rr][c] = in[c >> 1] ? v.x : pad_y;
            Yf[rr][c + 1] = in[c >> 1] ? v.y : pad_y;
        }
    }
}

// ---- the 10-bit output side ----------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ f2 trunc_clamp1023(f2 v) {
    f2 r;
    r.x = __builtin_amdgcn_fmed3f(__builtin_truncf(v.x), 0.0f, 1023.0f);
    r.y = __builtin_amdgcn_fmed3f(__builtin_truncf(v.y), 0.0f, 1023.0f);
    return r;
}
// k / 1023 for an integer-valued k in [0, 1023], correctly rounded (all 1024 inputs are checked by the tests): 1 / 1023 = hi + lo, e = k * lo, q = fma(k, hi, e)
// -- norm255's form (vpp_device.h); no division per pixel.
__device__ __forceinline__ f2 norm1023(f2 v) {
    const float hi = 0x1.00401p-10f, lo = 0x1.00401p-40f;
    const f2 e = v * (f2){ lo, lo };
    f2 q;
    q.x = __builtin_fmaf(v.x, hi, e.x);
    q.y = __builtin_fmaf(v.y, hi, e.y);
    return q;
}
// The byte of k as a float in front of a truncating, saturating pack: (k + 2) / 4, exact; the pack's truncation is the contract's `>> 2`, its saturation the
// `min(255, ...)` (k >= 1022 alone reaches 256)
__device__ __forceinline__ f2 p010_byte(f2 k) { return (f2){ __builtin_fmaf(k.x, 0.25f, 0.5f), __builtin_fmaf(k.y, 0.25f, 0.5f) }; }

// The three channel values of one output row of a thread tile (pairs 0 and 1 of each), as fp32, to their places: color_store_row's stores (vpp_device.h)
template <int OUT, bool VEC>
__device__ __forceinline__ void p010_store_row_f32(const f2 c0[2], const f2 c1[2], const f2 c2[2], float *o, uint32_t pix, uint32_t plane, int ncol, int nt,
                                                   const MergedRun &run) {
    constexpr bool PLANAR = OUT == O_F32_PLANAR;
    if constexpr (VEC && PLANAR) {
        const uint32_t boff = pix * 4u;
        st4o((uint8_t *)o, boff, c0[0].x, c0[0].y, c0[1].x, c0[1].y, nt);
        st4o((uint8_t *)(o + plane), boff, c1[0].x, c1[0].y, c1[1].x, c1[1].y, nt);
        st4o((uint8_t *)(o + 2 * (size_t)plane), boff, c2[0].x, c2[0].y, c2[1].x, c2[1].y, nt);
    } else if constexpr (VEC) {
        // merged: the lanes of a run exchange their 48-byte pixel quads through LDS so that each store instruction of the run writes one contiguous span (MergedRun)
        uint8_t *w = run.lds;
        *(vf4 *)(w + 48 * run.m) = (vf4){ c0[0].x, c1[0].x, c2[0].x, c0[0].y };
        *(vf4 *)(w + 48 * run.m + 16) = (vf4){ c1[0].y, c2[0].y, c0[1].x, c1[1].x };
        *(vf4 *)(w + 48 * run.m + 32) = (vf4){ c2[1].x, c0[1].y, c1[1].y, c2[1].y };
        __builtin_amdgcn_wave_barrier();
        const uint32_t q = (pix - 4u * (uint32_t)run.m) * 12u; // first byte of the run in this row
#pragma unroll
        for (int kk = 0; kk < 3; kk++) {
            const uint32_t off = (uint32_t)(kk * run.a + run.m) * 16u;
            const vf4 v = *(const vf4 *)(w + off);
            st4o((uint8_t *)o, q + off, v.x, v.y, v.z, v.w, nt);
        }
        __builtin_amdgcn_wave_barrier();
    } else {
        const float v0[4] = { c0[0].x, c0[0].y, c0[1].x, c0[1].y }, v1[4] = { c1[0].x, c1[0].y, c1[1].x, c1[1].y }, v2[4] = { c2[0].x, c2[0].y, c2[1].x, c2[1].y };
        for (int c = 0; c < ncol; c++) {
            if constexpr (PLANAR) {
                o[pix + c] = v0[c];
                o[plane + pix + c] = v1[c];
                o[2 * plane + pix + c] = v2[c];
            } else {
                o[3 * (pix + c)] = v0[c];
                o[3 * (pix + c) + 1] = v1[c];
                o[3 * (pix + c) + 2] = v2[c];
            }
        }
    }
}
// ... and as bytes: c0 / c1 / c2 hold p010_byte values
template <int OUT, bool VEC>
__device__ __forceinline__ void p010_store_row_u8(const f2 c0[2], const f2 c1[2], const f2 c2[2], uint8_t *o, uint32_t pix, uint32_t plane, int ncol, int nt,
                                                  const MergedRun &run) {
    constexpr bool PLANAR = OUT == O_U8_PLANAR;
    if constexpr (VEC) {
        uint32_t pa, pb, pc;
        if constexpr (PLANAR) {
            pack_u8x12_rtz(c0[0].x, c0[0].y, c0[1].x, c0[1].y, c1[0].x, c1[0].y, c1[1].x, c1[1].y, c2[0].x, c2[0].y, c2[1].x, c2[1].y, pa, pb, pc);
            st1o(o, pix, pa, nt);
            st1o(o + plane, pix, pb, nt);
            st1o(o + 2 * (size_t)plane, pix, pc, nt);
        } else {
            pack_u8x12_rtz(c0[0].x, c1[0].x, c2[0].x, c0[0].y, c1[0].y, c2[0].y, c0[1].x, c1[1].x, c2[1].x, c0[1].y, c1[1].y, c2[1].y, pa, pb, pc);
            if (run.lds && (run.a & 3) == 0) { // the run's three 4-byte stores at a 12-byte stride become one 16-byte store by three quarters of its lanes
                uint32_t *w = (uint32_t *)(run.lds + 12 * run.m);
                w[0] = pa;
                w[1] = pb;
                w[2] = pc;
                __builtin_amdgcn_wave_barrier();
                if (4 * run.m < 3 * run.a) {
                    typedef uint32_t u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));
                    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                    const u32x4 v = *(const u32x4 *)(run.lds + 16 * run.m);
                    const uint32_t off16 = 3u * (pix - 4u * (uint32_t)run.m) + 16u * (uint32_t)run.m; // rows start on 4-byte boundaries only
                    if (nt) st16_nt(o, off16, (nt_u32x4){ v.x, v.y, v.z, v.w }, nt);
                    else *(u32x4a4 *)(o + off16) = v;
                }
                __builtin_amdgcn_wave_barrier();
            } else {
                st1o(o, 3u * pix, pa, nt);
                st1o(o, 3u * pix + 4u, pb, nt);
                st1o(o, 3u * pix + 8u, pc, nt);
            }
        }
    } else {
        const f2 a0 = trunc2(c0[0]), a1 = trunc2(c0[1]), b0 = trunc2(c1[0]), b1 = trunc2(c1[1]), e0 = trunc2(c2[0]), e1 = trunc2(c2[1]);
        const uint32_t p0 = pack_u8x4(a0.x, a0.y, a1.x, a1.y), p1 = pack_u8x4(b0.x, b0.y, b1.x, b1.y), p2 = pack_u8x4(e0.x, e0.y, e1.x, e1.y);
        for (int c = 0; c < ncol; c++) {
            const uint8_t v0 = (uint8_t)(p0 >> (8 * c)), v1 = (uint8_t)(p1 >> (8 * c)), v2 = (uint8_t)(p2 >> (8 * c));
            if constexpr (PLANAR) {
                o[pix + c] = v0;
                o[plane + pix + c] = v1;
                o[2 * plane + pix + c] = v2;
            } else {
                o[3 * (pix + c)] = v0;
                o[3 * (pix + c) + 1] = v1;
                o[3 * (pix + c) + 2] = v2;
            }
        }
    }
}

// One row of one plane of a tensor output: q -> (q - mean) * scale -> the element (vpp_tensor_store.h)
template <int EL, bool VEC>
__device__ __forceinline__ void p010_tensor_row(uint8_t *base, uint32_t pix, const f2 k[2], const tsvpp_tensor_spec &a, int ch, int ncol, int nt) {
    const f2 v0 = tensor_affine(norm1023(k[0]), a.mean[ch], a.scale[ch]), v1 = tensor_affine(norm1023(k[1]), a.mean[ch], a.scale[ch]);
    if constexpr (EL == EL_F32) tensor_store4<TSVPP_F32, VEC>(base, pix, v0, v1, ncol, nt);
    else if (a.dtype == TSVPP_F16) tensor_store4<TSVPP_F16, VEC>(base, pix, v0, v1, ncol, nt); // (wave-uniform)
    else tensor_store4<TSVPP_BF16, VEC>(base, pix, v0, v1, ncol, nt);
}

// A thread tile's samples (integer-valued floats 0..1023) to its output.  `d.k` carries y_offset and c_offset ALREADY scaled by four (the kernel does it once): the
// luma expression and chroma_terms are then the library's own.
template <int OUT, bool VEC, int EL>
__device__ __forceinline__ void p010_store_tile(const float Yf[PXH][PXW], const float Uf[2], const float Vf[2], const LaunchDesc &d, const tsvpp_tensor_spec &a,
                                                typename OutT<OUT>::type *out, int i0, int j0, int ncol) {
    using T = typename OutT<OUT>::type;
    const int nt = d.nt_stores;
    const uint32_t plane = (uint32_t)d.dst_w * (uint32_t)d.dst_h;
    if constexpr (kLumaOnly<OUT>) { // Y800: the luma sample itself
#pragma unroll
        for (int r = 0; r < PXH; r++) {
            const uint32_t pix = (uint32_t)(i0 + r) * (uint32_t)d.dst_w + (uint32_t)j0;
            const f2 k[2] = { { Yf[r][0], Yf[r][1] }, { Yf[r][2], Yf[r][3] } };
            if constexpr (EL != EL_LIB) p010_tensor_row<EL, VEC>((uint8_t *)out, pix, k, a, 0, ncol, nt);
            else if constexpr (sizeof(T) == 4) tensor_store4<TSVPP_F32, VEC>((uint8_t *)out, pix, norm1023(k[0]), norm1023(k[1]), ncol, nt);
            else {
                const f2 b0 = trunc2(p010_byte(k[0])), b1 = trunc2(p010_byte(k[1]));
                const uint32_t p = pack_u8x4(b0.x, b0.y, b1.x, b1.y);
                uint8_t *o = (uint8_t *)out;
                if constexpr (VEC) st1o(o, pix, p, nt);
                else
                    for (int c = 0; c < ncol; c++) o[pix + c] = (uint8_t)(p >> (8 * c));
            }
        }
        return;
    } else {
        float t0[2], tg[2], t2[2];
#pragma unroll
        for (int c = 0; c < 2; c++) chroma_terms(Uf[c], Vf[c], d.k, d.swap_rb, d.color_g, t0[c], tg[c], t2[c]);
        MergedRun run{ nullptr, 0, 1 };
        if constexpr (EL == EL_LIB) run = merged_run<OUT, VEC>(d, j0);
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
                c0[p] = trunc_clamp1023(y + (f2){ t0[p], t0[p] });
                c1[p] = trunc_clamp1023(y + (f2){ tg[p], tg[p] });
                c2[p] = trunc_clamp1023(y + (f2){ t2[p], t2[p] });
            }
            if constexpr (EL != EL_LIB) {
                const size_t plane_bytes = (size_t)plane * (EL == EL_F32 ? 4u : 2u);
                p010_tensor_row<EL, VEC>((uint8_t *)out, pix, c0, a, 0, ncol, nt);
                p010_tensor_row<EL, VEC>((uint8_t *)out + plane_bytes, pix, c1, a, 1, ncol, nt);
                p010_tensor_row<EL, VEC>((uint8_t *)out + 2 * plane_bytes, pix, c2, a, 2, ncol, nt);
            } else if constexpr (sizeof(T) == 4) {
#pragma unroll
                for (int p = 0; p < 2; p++) {
                    c0[p] = norm1023(c0[p]);
                    c1[p] = norm1023(c1[p]);
                    c2[p] = norm1023(c2[p]);
                }
                p010_store_row_f32<OUT, VEC>(c0, c1, c2, (float *)out, pix, plane, ncol, nt, run);
            } else {
#pragma unroll
                for (int p = 0; p < 2; p++) {
                    c0[p] = p010_byte(c0[p]);
                    c1[p] = p010_byte(c1[p]);
                    c2[p] = p010_byte(c2[p]);
                }
                p010_store_row_u8<OUT, VEC>(c0, c1, c2, (uint8_t *)out, pix, plane, ncol, nt, run);
            }
        }
    }
}

// ---- the kernel ----------------------------------------------------------------------------------------------------------------------------------------------
template <int MODE, int OUT, bool VEC, bool STAGED, int EL = EL_LIB>
__global__ __launch_bounds__(ROI_THREADS) void vpp_letterbox_p010_kernel(const LbLaunch L) {
    using T = typename OutT<OUT>::type;
    typedef __attribute__((address_space(1))) uint8_t *GP; // the records hold GLOBAL addresses
    const TileIndex tix = tile_index(L.tiles_x, L.tiles_y);
    const int frame = tix.item, tyi = tix.tyi, txi = tix.txi;
    if (frame >= L.n_frames) return;
    const LbRec &r = L.r[frame]; // wave-uniform index: scalar loads

    LaunchDesc d = {};
    tile_desc<OUT, VEC>(L, r, d);
    d.k.y_offset = 4.0f * d.k.y_offset; // the contract's scaled offsets (exact)
    d.k.c_offset = 4.0f * d.k.c_offset;

    const uint8_t *const plane_y = (const uint8_t *)(GP)(uintptr_t)r.y, *const plane_uv = (const uint8_t *)(GP)(uintptr_t)r.uv;
    const bool uv4 = (((uint32_t)r.uv | (uint32_t)r.pitch_uv) & 3u) == 0u;
    T *const out = (T *)(GP)(uintptr_t)r.out;
    const int lx = threadIdx.x & (ROI_TX - 1), ly = threadIdx.x >> ROI_TX_SHIFT;
    const int j_first = roi_tile_col0(txi, L.dst_w, d.last_col0), i_first = tyi * ROI_TILE_H;
    const int j0 = j_first + lx * PXW, i0 = i_first + ly * PXH;
    const bool active = j0 < L.dst_w && i0 < L.dst_h && !(VEC && is_row_tail(d, j0));
    const int ncol = VEC ? PXW : min(PXW, L.dst_w - j0);

    // the part of the rectangle this tile covers (wave-uniform)
    LbPart t;
    tile_inner_range(j_first, tile_last(j_first, ROI_TILE_W, L.dst_w), r.left, r.width, t.a0, t.a1);
    tile_inner_range(i_first, tile_last(i_first, ROI_TILE_H, L.dst_h), r.top, r.height, t.b0, t.b1);
    float Uf[2] = { L.pad_u, L.pad_u }, Vf[2] = { L.pad_v, L.pad_v }, Yf[PXH][PXW];
    if (t.a0 > t.a1 || t.b0 > t.b1) { // none of it: pad, through the colour expression and store of every sample
        if (!active) return;
#pragma unroll
        for (int rr = 0; rr < PXH; rr++)
#pragma unroll
            for (int c = 0; c < PXW; c++) Yf[rr][c] = L.pad_y;
        p010_store_tile<OUT, VEC, EL>(Yf, Uf, Vf, d, L.spec, out, i0, j0, ncol);
        return;
    }

    if constexpr (STAGED) {
        RoiFootprint f;
        tile_span_x(MODE, t.a0, t.a1, r.src_w, r.xr, f);
        tile_span_y(MODE, t.b0, t.b1, r.src_h, r.yr, f);
        if (p010_stageable(f) && p010_lds_need(f, kLumaOnly<OUT>) <= L.lds_bytes) { // (wave-uniform)
            // the footprint as raw words, 16-byte chunks straight from global memory into LDS: 8 luma samples or 4 chroma pairs per chunk
            const int span_y = p010_span_y(f.xhi - f.xlo + 1), span_uv = p010_span_uv(f.cxhi - f.cxlo + 1);
            const int ny = f.yhi - f.ylo + 1, nuv = kLumaOnly<OUT> ? 0 : f.cyhi - f.cylo + 1;
            const int cpr_y = roi_chunks(span_y), cpr_uv = roi_chunks(span_uv);
            uint8_t *lds_y = lds_raw, *lds_uv = lds_raw + 16 * p010_slots(ny * cpr_y);
            const uint8_t *ay, *auv;
            P010Lds s;
            s.py_ = describe_plane(lds_y, plane_y, r.pitch_y, f.ylo, 2 * f.xlo, cpr_y, ay);
            s.puv_ = describe_plane(lds_uv, plane_uv, r.pitch_uv, f.cylo, 4 * f.cxlo, cpr_uv, auv);
            s.w = r.src_w;
            s.h = r.src_h;
            s.uv4 = uv4;
            // slot -> (row, chunk) by multiply-high: one division per workgroup, on wave-uniform values
            stage_plane_dma(lds_y, ay, s.py_, r.pitch_y, ny, span_y, 0xFFFFFFFFu / (uint32_t)cpr_y + 1u, ROI_THREADS);
            if constexpr (!kLumaOnly<OUT>) stage_plane_dma(lds_uv, auv, s.puv_, r.pitch_uv, nuv, span_uv, 0xFFFFFFFFu / (uint32_t)cpr_uv + 1u, ROI_THREADS);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // LDS-DMA chunks have landed
            __syncthreads();
            if (!active) return;
            p010_sample_tile<MODE, OUT, VEC>(s, r, t, L, i0, j0, Yf, Uf, Vf);
            p010_store_tile<OUT, VEC, EL>(Yf, Uf, Vf, d, L.spec, out, i0, j0, ncol);
            return;
        }
    }
    if (!active) return;
    const P010Global s = { plane_y, plane_uv, r.pitch_y, r.pitch_uv, r.src_w, r.src_h, uv4 };
    p010_sample_tile<MODE, OUT, VEC>(s, r, t, L, i0, j0, Yf, Uf, Vf);
    p010_store_tile<OUT, VEC, EL>(Yf, Uf, Vf, d, L.spec, out, i0, j0, ncol);
}

} // namespace tsvpp
