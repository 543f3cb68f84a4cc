// vpp_box_p010.h -- the arithmetic of tsvpp_convert_letterbox_p010_area and tsvpp_convert_rois_p010_area (include/tsvpp.h), once, for the
// kernels (vpp_box_p010_walk.h: vpp_letterbox_p010_area_core.h, vpp_rois_p010_area_core.h), the host paths (tsvpp_letterbox_p010_area.cpp) and the host's executable form of the contract (tsvpp_box_p010_plane): an exact
// box filter in unsigned 32-bit integers.  One axis with N source samples and n output samples, in units in which a source sample is n wide: output j covers
// [j N, (j + 1) N), its taps are i = floor(j N / n) .. floor(((j + 1) N - 1) / n), tap i weighs o(i, j) = min((i + 1) n, (j + 1) N) - max(i n, j N); the weights
// are positive and sum to N.  Horizontal pass per source row: hx = sum o_x s, r = (64 hx + N_x / 2) / N_x (the row mean in 1/64 sample steps); vertical pass:
// v = sum o_y r, k = (v + 32 N_y) / (64 N_y).  Every division is a floor division.  No float reaches a result: the fp32 reciprocals below only GUESS a quotient,
// which an integer step corrects.  Product code -- never includes anything from oracle/.
#pragma once
#include <stdint.h>

#include "vpp_kernels.h"

namespace tsvpp {

constexpr int BOX_P010_MAX_SIDE = TSVPP_BOX_P010_MAX_SIDE; // of a frame and of its rectangle: n N <= 2^28, 64 hx <= 2^30 and v < 2^30 all need it
constexpr int BOX_P010_MAX_TAPS = TSVPP_BOX_P010_MAX_TAPS; // per axis

// A divisor that stays the same for many numerators: the divisor and the fp32 reciprocal that guesses the quotient
struct BoxDiv {
    uint32_t d;
    float rcp;
};
__host__ __device__ __forceinline__ BoxDiv box_div_of(uint32_t d) { return BoxDiv{ d, 1.0f / (float)d }; }
// floor(num / dv.d), exact wherever the quotient is below 2^16 and num + d below 2^32 -- which the two limits above give every division of this file (first taps
// are below 2^14, r is at most 65472, k at most 1023).  (float)num and rcp are each within 2^-24 relative of their value and the product rounds once more, so the
// guess is within q 2^-22 + 1 < 2 of num / d before truncation: it is q - 1, q or q + 1, and the remainder says which.
__host__ __device__ __forceinline__ uint32_t box_quot(uint32_t num, const BoxDiv &dv) {
    uint32_t q = (uint32_t)((float)num * dv.rcp);
    const int32_t rem = (int32_t)(num - q * dv.d);
    q -= rem < 0 ? 1u : 0u;
    q += rem >= (int32_t)dv.d ? 1u : 0u;
    return q;
}

// One axis of one output index j: first tap, tap count, and the weights of the first and the last tap -- every tap between them weighs n
struct BoxTaps {
    uint32_t first, count, w_first, w_last;
};
__host__ __device__ __forceinline__ BoxTaps box_taps(uint32_t j, uint32_t N, uint32_t n, const BoxDiv &dn) {
    BoxTaps t;
    const uint32_t lo = j * N, hi = lo + N; // the interval of j
    t.first = box_quot(lo, dn);
    const uint32_t last = box_quot(hi - 1u, dn);
    t.count = last - t.first + 1u;
    const uint32_t e = (t.first + 1u) * n;
    t.w_first = (e < hi ? e : hi) - lo;
    t.w_last = hi - last * n; // (count == 1: never read)
    return t;
}
// o(i, j), or 0 where tap i does not touch output j: the vertical pass asks for the rows of a band, which need not all belong to its lane's outputs
__host__ __device__ __forceinline__ uint32_t box_overlap(uint32_t i, uint32_t j, uint32_t N, uint32_t n) {
    const uint32_t a0 = i * n, a1 = a0 + n, b0 = j * N, b1 = b0 + N;
    const uint32_t lo = a0 > b0 ? a0 : b0, hi = a1 < b1 ? a1 : b1;
    return hi > lo ? hi - lo : 0u;
}
// the largest tap count of an axis: j N mod n runs through every multiple of g = gcd(N, n), and output j has floor((j N mod n + N - 1) / n) + 1 taps
__host__ __device__ inline int box_max_taps(int N, int n) {
    int a = N, b = n;
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return (int)(((long)n - a + N - 1) / n) + 1;
}
// The exact source footprint of output indices [o0, o1] of an axis N -> n: first tap of o0, last tap of o1 (host and device alike: the host sizes the band
// buffers with the numbers the kernel computes)
__host__ __device__ inline void box_span(int o0, int o1, int N, int n, int &lo, int &hi) {
    const BoxDiv dn = box_div_of((uint32_t)n);
    lo = (int)box_quot((uint32_t)o0 * (uint32_t)N, dn);
    hi = (int)box_quot(((uint32_t)o1 + 1u) * (uint32_t)N - 1u, dn);
}
// the two normalising divisions
__host__ __device__ __forceinline__ uint32_t box_row_mean(uint32_t hx, const BoxDiv &dN) { return box_quot(64u * hx + (dN.d >> 1), dN); }
__host__ __device__ __forceinline__ uint32_t box_sample(uint32_t v, uint32_t N, const BoxDiv &d64N) { return box_quot(v + 32u * N, d64N); }

// ---- the band walk's LDS (host: the launch's dynamic LDS and band=; kernel: its carve-up) ----------------------------------------------------------------
// A workgroup walks its tile's source footprint in bands of `rows` source rows: two band buffers of raw words (the next band lands while the current one is
// reduced), each `rows` rows of `cpr` 16-byte chunks rounded up to the 64 slots a wave instruction of the LDS-DMA loop fills, and in front of them the row means
// r of one band, rows x 32 output columns (chroma: 16 pairs x (U, V)) as 32-bit words.
constexpr int BOX_BAND_MAX_ROWS = 32;
__host__ __device__ inline int box_band_buffer(int rows, int cpr) { return 16 * ((rows * cpr + 63) & ~63); }
__host__ __device__ inline int box_band_lds(int rows, int cpr) { return rows * 32 * 4 + 2 * box_band_buffer(rows, cpr); }
// the most rows whose bands fit `budget` bytes at `cpr` chunks per row; one row where not even that fits (4.7 KiB at the widest footprint the tap limit allows)
__host__ __device__ inline int box_band_rows(int budget, int cpr) {
    int rows = BOX_BAND_MAX_ROWS;
    while (rows > 1 && box_band_lds(rows, cpr) > budget) rows--;
    return rows;
}

} // namespace tsvpp
