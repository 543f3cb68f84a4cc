// vpp_cubic_p010.h -- the arithmetic of tsvpp_convert_rois_p010_bicubic (include/tsvpp.h), once, for the kernel
// (vpp_rois_p010_bicubic_core.h), the host path (tsvpp_rois_p010_bicubic.cpp) and the host's executable form of the contract (tsvpp_cubic_p010_plane): a
// separable Keys cubic (a = -3/4) in signed 32-bit integers.  One axis with N source and n output samples; output j: t = (2 j + 1) N - n (the pixel-centre
// alignment (j + 1/2) N / n - 1/2 over the denominator 2 n), p = floor(t / (2 n)) (-1 exactly when t < 0), rem = t - 2 n p, phase F = floor(32 rem / n) in 0..63,
// G = 64 - F; taps clamp(p - 1 + k, 0, N - 1), k = 0..3, with the weights w_k below, integers that sum to 2^20.  Horizontal pass h = (sum w s + 2^19) >> 20, not
// clamped, -192..1215; vertical pass k = clamp((sum w h + 2^19) >> 20, 0, 1023).  |sum| <= 1215.5 * 1.375 * 2^20 < 2^31 in both.  No float reaches a result:
// the fp32 reciprocal of box_quot only GUESSES a quotient.  Product code -- never includes anything from oracle/.
#pragma once
#include <stdint.h>

#include "vpp_box_p010.h"

namespace tsvpp {

constexpr int CUBIC_P010_MAX_SIDE = TSVPP_CUBIC_P010_MAX_SIDE;   // of a box and of the output: t < 2^30 needs it
constexpr int CUBIC_P010_MAX_RATIO = TSVPP_CUBIC_P010_MAX_RATIO; // N <= 8 n per axis and plane: the kernel's bound on a tile's intermediate rows, not the arithmetic's

// The two divisors of one axis
struct CubicDiv {
    BoxDiv d2n, dn;
    int N, n;
};
__host__ __device__ __forceinline__ CubicDiv cubic_div_of(int N, int n) { return CubicDiv{ box_div_of(2u * (uint32_t)n), box_div_of((uint32_t)n), N, n }; }

// One axis of one output index: p (the taps are p - 1 .. p + 2 before the clamp) and the phase.  box_quot's preconditions: t < 2^30 and p < N <= 2^14;
// 32 rem < 64 n <= 2^20 and F < 64.  t < 0 is handled apart: t >= N - n > -2 n, so p = -1 and rem = t + 2 n.
struct CubicTerm {
    int p, F;
};
__host__ __device__ __forceinline__ CubicTerm cubic_term(int j, const CubicDiv &a) {
    const int t = (2 * j + 1) * a.N - a.n;
    CubicTerm c;
    c.p = t < 0 ? -1 : (int)box_quot((uint32_t)t, a.d2n);
    const int rem = t - 2 * a.n * c.p;
    c.F = (int)box_quot(32u * (uint32_t)rem, a.dn);
    return c;
}
// Keys' cubic with a = -3/4 at x = F / 64, times 2^20: exact integers, |w| <= 2^20, sum 2^20
__host__ __device__ __forceinline__ void cubic_weights(int F, int w[4]) {
    const int G = 64 - F;
    w[0] = -3 * F * G * G;
    w[1] = 5 * F * F * F - 576 * F * F + (1 << 20);
    w[2] = 5 * G * G * G - 576 * G * G + (1 << 20);
    w[3] = -3 * F * F * G;
}
// tap k of an axis term, clamped to the axis
__host__ __device__ __forceinline__ int cubic_tap(int p, int k, int N) {
    const int i = p - 1 + k;
    return i < 0 ? 0 : (i > N - 1 ? N - 1 : i);
}
// A weight times a sample or an h value: both fit 24 signed bits (v_mad_i32_i24 on the device, the same product on the host)
__host__ __device__ __forceinline__ int cubic_mul(int w, int s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(w, s);
#else
    return w * s;
#endif
}
__host__ __device__ __forceinline__ int cubic_sum(const int w[4], int s0, int s1, int s2, int s3) {
    return cubic_mul(w[0], s0) + cubic_mul(w[1], s1) + cubic_mul(w[2], s2) + cubic_mul(w[3], s3) + (1 << 19);
}
// the two roundings: an arithmetic shift, i.e. a floor; only the vertical one clamps
__host__ __device__ __forceinline__ int cubic_round_h(int sum) { return sum >> 20; }
__host__ __device__ __forceinline__ int cubic_round_v(int sum) {
    const int k = sum >> 20;
    return k < 0 ? 0 : (k > 1023 ? 1023 : k);
}

// The source footprint of output indices [o0, o1] of an axis: first tap of o0, last tap of o1, clamped to the axis (p is monotone in j).  Host and device
// alike: the host sizes the launch's LDS with the numbers the kernel computes.
__host__ __device__ inline void cubic_span(int o0, int o1, const CubicDiv &a, int &lo, int &hi) {
    lo = cubic_tap(cubic_term(o0, a).p, 0, a.N);
    hi = cubic_tap(cubic_term(o1, a).p, 3, a.N);
}

// ---- the walk's LDS (host: the launch's dynamic LDS and band=; kernel: its carve-up) -------------------------------------------------------------------
// In front: Hbuf, the tile's horizontally filtered rows, `hrows` rows of 32 16-bit integers (chroma: 16 pairs x (U, V)).  Behind it: two band buffers of raw
// words, each `band` rows of `cpr` 16-byte chunks rounded up to the 64 slots a wave instruction of the LDS-DMA loop fills (box_band_buffer).
constexpr int CUBIC_HROW_BYTES = 64;
constexpr int CUBIC_TILE_MAX_HROWS = 32 * CUBIC_P010_MAX_RATIO + 3; // 259 rows, 16576 bytes
__host__ __device__ inline int cubic_hbuf_bytes(int hrows) { return CUBIC_HROW_BYTES * hrows; }
__host__ __device__ inline int cubic_lds(int hrows, int band, int cpr) { return cubic_hbuf_bytes(hrows) + 2 * box_band_buffer(band, cpr); }
// the most rows per band that fit `budget` bytes behind Hbuf; 0 where not even one-row bands fit
__host__ __device__ inline int cubic_band_rows(int budget, int hrows, int cpr) {
    int rows = hrows < BOX_BAND_MAX_ROWS ? hrows : BOX_BAND_MAX_ROWS;
    while (rows > 0 && cubic_lds(hrows, rows, cpr) > budget) rows--;
    return rows;
}

} // namespace tsvpp
