// vpp_twins.cpp -- the DEVICE compile of the AREA weight generator and of the jump-start search against their host compile and the C ABI.
//
// roi_area_step / roi_area_weight (csrc/vpp_rois.h) and lb_area_period / lb_area_chain_start (csrc/vpp_letterbox_area.h) are __host__ __device__ functions.  The
// CPU tests pin the HOST compile against the library's table and the oracle, bit for bit, through tsvpp_roi_area_rows and tsvpp_letterbox_area_rows; the device
// compile runs only inside vpp_rois_area and vpp_letterbox_area, where the suite sees it through 8-bit outputs -- and lb_area_period has a device branch (a ballot
// search) the host never executes.  This program includes the two headers -- it holds no copy of their arithmetic --, is compiled with csrc's flags, runs the
// functions in three trivial kernels (plain vector stores, no LDS) and compares raw bits:
//
//   gen_rows      one lane per scale runs roi_area_step from index 0 over N_INDEX indices; every RoiAreaRow record against the host's run of the same function
//   gen_weights   the records of 32 indices at 0, 1000 and 4064 expanded through roi_area_weight on the device, against tsvpp_roi_area_rows
//   period        one full wave per (scale, first) calls lb_area_period and lb_area_chain_start with wave-uniform arguments, as the kernel does; every lane's
//                 answers against the host scan, and the start against the one tsvpp_letterbox_area_rows returns
//   jump_rows     one lane per (scale, first) begins a generator at the device's own start with the initial state and expands the rows first .. first + 31 (as far
//                 as index 65535), against tsvpp_roi_area_rows: the chain from 0
//   host_weights  (host) the host's records expanded, against tsvpp_roi_area_rows
//   host_period   (host) the host scan's start against tsvpp_letterbox_area_rows', and that call's rows against tsvpp_roi_area_rows'
//
// One line per group: name cases mismatches first-mismatch ("-" without one).  Exit status 1 on any mismatch, 2 on a failed call.
//   vpp_twins          every group
//   vpp_twins --host   the two host groups only: touches no HIP runtime call
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "vpp_rois.h"
#include "vpp_letterbox_area.h"

using namespace tsvpp;

namespace {

constexpr int N_INDEX = 4096;                       // indices of a generator run
constexpr int N_SUB = 32, N_SUBSETS = 3, N_FIRST = 12;
// first index of each 32-index subset the C ABI is asked for
__host__ __device__ inline int subset_first(int k) {
    constexpr int t[N_SUBSETS] = { 0, 1000, 4064 };
    return t[k];
}
// the `first` of the jump-start groups
__host__ __device__ inline int first_of(int k) {
    constexpr int t[N_FIRST] = { 0, 1, 31, 32, 63, 64, 65, 127, 128, 1000, 4095, 65535 };
    return t[k];
}
constexpr int MAX_T = ROI_AREA_MAX_TAPS;

struct Scale {
    int src, dst;
    float v;
};

// float32(src) / float32(dst): the named ratios, then 200 seeded pairs with src in 2 .. 4096 and 1 < src / dst <= 40
std::vector<Scale> scales() {
    const int named[][2] = { { 1920, 640 }, { 1920, 608 }, { 1366, 640 }, { 1920, 48 }, { 448, 224 }, { 336, 224 }, { 300, 224 }, { 226, 224 }, { 322, 70 }, { 182, 66 },
                             { 250, 64 }, { 240, 100 }, { 180, 76 } };
    std::vector<Scale> out;
    for (const auto &p : named) out.push_back({ p[0], p[1], (float)p[0] / (float)p[1] });
    std::mt19937 rng(20261022u);  // (the engine's output is fixed by the standard; the ranges are taken with % below, not with a distribution)
    while (out.size() < 13 + 200) {
        const int src = 2 + (int)(rng() % 4095u);
        const int lo = (src + MAX_T - 1) / MAX_T, hi = src - 1;  // src / dst <= 40 and > 1
        const int dst = lo + (int)(rng() % (unsigned)(hi - lo + 1));
        out.push_back({ src, dst, (float)src / (float)dst });
    }
    return out;
}

uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
bool same(const RoiAreaRow &a, const RoiAreaRow &b) { return bits(a.lead) == bits(b.lead) && a.ones == b.ones && bits(a.tail) == bits(b.tail); }

struct Group {
    std::string name;
    long cases = 0, bad = 0;
    std::string first = "-";
    void check(bool ok, const char *fmt, ...) __attribute__((format(printf, 3, 4))) {
        cases++;
        if (ok) return;
        if (bad++ == 0) {
            char buf[256];
            va_list ap;
            va_start(ap, fmt);
            vsnprintf(buf, sizeof buf, fmt, ap);
            va_end(ap);
            first = buf;
        }
    }
    bool report() const {
        printf("%s %ld %ld %s\n", name.c_str(), cases, bad, first.c_str());
        return bad == 0;
    }
};

// rows of indices first .. first + n - 1 by the C ABI (the chain from 0): n * taps floats
bool abi_rows(float scale, int first, int n, std::vector<float> &out, int &taps) {
    out.assign((size_t)n * MAX_T, 0.0f);
    return tsvpp_roi_area_rows(scale, first, n, out.data(), (int)out.size(), &taps) == n && taps == roi_area_taps(scale);
}
int rows_at(int first) { return first + N_SUB <= ROI_AREA_MAX_DST ? N_SUB : ROI_AREA_MAX_DST - first; }

// ---- device side: the functions of the two headers, nothing else ------------------------------------------------------------------------------------------
__global__ void twin_rows(const float *scale, int n_scales, RoiAreaRow *rows) {
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= n_scales) return;
    RoiAreaGen g;
    for (int j = 0; j < N_INDEX; j++) rows[(size_t)s * N_INDEX + j] = roi_area_step(scale[s], g);
}
// element (s, subset row i, entry e) of the expansion; entries past the scale's taps are written as 0
__global__ void twin_weights(const float *scale, int n_scales, const RoiAreaRow *rows, float *w) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= n_scales * N_SUBSETS * N_SUB * MAX_T) return;
    const int e = k % MAX_T, i = (k / MAX_T) % (N_SUBSETS * N_SUB), s = k / (MAX_T * N_SUBSETS * N_SUB);
    const int j = subset_first(i / N_SUB) + i % N_SUB;
    w[k] = e < roi_area_taps(scale[s]) ? roi_area_weight(rows[(size_t)s * N_INDEX + j], e) : 0.0f;
}
// one wave of 64 per (scale, first); every lane stores its own two answers
__global__ void twin_period(const float *scale, int n_scales, int2 *out) {
    const int b = (int)blockIdx.x;
    if (b >= n_scales * N_FIRST) return;
    const float sc = scale[b / N_FIRST];
    const int first = first_of(b % N_FIRST);
    const int period = lb_area_period(sc, first);
    const int start = lb_area_chain_start(sc, first);
    out[(size_t)b * 64 + threadIdx.x] = make_int2(period, start);
}
// one lane per (scale, first): the generator begun at `start` (lane 0's of twin_period) with the initial state, the rows first .. first + n - 1 expanded
__global__ void twin_jump(const float *scale, int n_scales, const int2 *period, float *w) {
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= n_scales * N_FIRST) return;
    const float sc = scale[b / N_FIRST];
    const int first = first_of(b % N_FIRST), taps = roi_area_taps(sc);
    const int n = first + N_SUB <= ROI_AREA_MAX_DST ? N_SUB : ROI_AREA_MAX_DST - first;
    int start = period[(size_t)b * 64].y;
    start = start < 0 ? 0 : (start > first ? first : start);  // (a wrong start is reported by the period group; here it must not lengthen the loop)
    RoiAreaGen g;
    for (int k = start; k < first + n; k++) {
        const RoiAreaRow r = roi_area_step(sc, g);
        if (k >= first)
            for (int e = 0; e < MAX_T; e++) w[((size_t)b * N_SUB + (k - first)) * MAX_T + e] = e < taps ? roi_area_weight(r, e) : 0.0f;
    }
}

#define HIP_OK(call)                                                                      \
    do {                                                                                  \
        const hipError_t e_ = (call);                                                     \
        if (e_ != hipSuccess) {                                                           \
            fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));                    \
            return 2;                                                                     \
        }                                                                                 \
    } while (0)

// ---- the host half ----------------------------------------------------------------------------------------------------------------------------------------
int host_half(const std::vector<Scale> &sc, const std::vector<RoiAreaRow> &rows, bool &ok) {
    Group hw{ "host_weights" }, hp{ "host_period" };
    std::vector<float> abi, jump;
    int taps = 0;
    for (size_t s = 0; s < sc.size(); s++) {
        for (int sub = 0; sub < N_SUBSETS; sub++) {
            if (!abi_rows(sc[s].v, subset_first(sub), N_SUB, abi, taps)) return 2;
            for (int i = 0; i < N_SUB; i++) {
                const int j = subset_first(sub) + i;
                bool eq = true;
                for (int e = 0; e < taps; e++) eq = eq && bits(roi_area_weight(rows[s * N_INDEX + j], e)) == bits(abi[(size_t)i * taps + e]);
                hw.check(eq, "%d/%d index %d", sc[s].src, sc[s].dst, j);
            }
        }
        for (int f = 0; f < N_FIRST; f++) {
            const int first = first_of(f), n = rows_at(first);
            int start = -1, t2 = 0;
            jump.assign((size_t)n * MAX_T, 0.0f);
            if (tsvpp_letterbox_area_rows(sc[s].v, first, n, jump.data(), (int)jump.size(), &t2, &start) != n || !abi_rows(sc[s].v, first, n, abi, taps) || t2 != taps) return 2;
            hp.check(start == lb_area_chain_start(sc[s].v, first) && start == lb_area_start_of(lb_area_period(sc[s].v, first), first), "%d/%d first %d: start %d", sc[s].src,
                     sc[s].dst, first, start);
            hp.check(memcmp(jump.data(), abi.data(), (size_t)n * taps * 4) == 0, "%d/%d first %d: rows from %d differ from the chain from 0", sc[s].src, sc[s].dst, first, start);
        }
    }
    const bool a = hw.report(), b = hp.report();  // (both lines are printed whatever the first says)
    ok = a && b;
    return 0;
}

int device_half(const std::vector<Scale> &sc, const std::vector<RoiAreaRow> &rows, bool &ok) {
    const int S = (int)sc.size();
    std::vector<float> v(S);
    for (int s = 0; s < S; s++) v[s] = sc[s].v;
    float *d_scale = nullptr, *d_w = nullptr, *d_jump = nullptr;
    RoiAreaRow *d_rows = nullptr;
    int2 *d_period = nullptr;
    const size_t n_rows = (size_t)S * N_INDEX, n_w = (size_t)S * N_SUBSETS * N_SUB * MAX_T, n_p = (size_t)S * N_FIRST * 64, n_j = (size_t)S * N_FIRST * N_SUB * MAX_T;
    HIP_OK(hipMalloc(&d_scale, S * sizeof(float)));
    HIP_OK(hipMalloc(&d_rows, n_rows * sizeof(RoiAreaRow)));
    HIP_OK(hipMalloc(&d_w, n_w * sizeof(float)));
    HIP_OK(hipMalloc(&d_period, n_p * sizeof(int2)));
    HIP_OK(hipMalloc(&d_jump, n_j * sizeof(float)));
    HIP_OK(hipMemcpy(d_scale, v.data(), S * sizeof(float), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_rows, 0xFF, n_rows * sizeof(RoiAreaRow)));
    HIP_OK(hipMemset(d_w, 0xFF, n_w * sizeof(float)));
    HIP_OK(hipMemset(d_period, 0xFF, n_p * sizeof(int2)));
    HIP_OK(hipMemset(d_jump, 0xFF, n_j * sizeof(float)));
    hipLaunchKernelGGL(twin_rows, dim3((S + 63) / 64), dim3(64), 0, 0, d_scale, S, d_rows);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(twin_weights, dim3((unsigned)((n_w + 255) / 256)), dim3(256), 0, 0, d_scale, S, d_rows, d_w);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(twin_period, dim3(S * N_FIRST), dim3(64), 0, 0, d_scale, S, d_period);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(twin_jump, dim3((S * N_FIRST + 63) / 64), dim3(64), 0, 0, d_scale, S, d_period, d_jump);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    std::vector<RoiAreaRow> g_rows(n_rows);
    std::vector<float> g_w(n_w), g_jump(n_j), abi;
    std::vector<int2> g_p(n_p);
    HIP_OK(hipMemcpy(g_rows.data(), d_rows, n_rows * sizeof(RoiAreaRow), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(g_w.data(), d_w, n_w * sizeof(float), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(g_p.data(), d_period, n_p * sizeof(int2), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(g_jump.data(), d_jump, n_j * sizeof(float), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_scale));
    HIP_OK(hipFree(d_rows));
    HIP_OK(hipFree(d_w));
    HIP_OK(hipFree(d_period));
    HIP_OK(hipFree(d_jump));

    Group gr{ "gen_rows" }, gw{ "gen_weights" }, pe{ "period" }, ju{ "jump_rows" };
    int taps = 0;
    for (int s = 0; s < S; s++) {
        for (int j = 0; j < N_INDEX; j++) {
            const RoiAreaRow &d = g_rows[(size_t)s * N_INDEX + j], &h = rows[(size_t)s * N_INDEX + j];
            gr.check(same(d, h), "%d/%d index %d: device (%a, %d, %a) host (%a, %d, %a)", sc[s].src, sc[s].dst, j, d.lead, d.ones, d.tail, h.lead, h.ones, h.tail);
        }
        for (int sub = 0; sub < N_SUBSETS; sub++) {
            if (!abi_rows(sc[s].v, subset_first(sub), N_SUB, abi, taps)) return 2;
            for (int i = 0; i < N_SUB; i++) {
                const float *d = &g_w[(((size_t)s * N_SUBSETS + sub) * N_SUB + i) * MAX_T];
                bool eq = true;
                for (int e = 0; e < MAX_T; e++) eq = eq && bits(d[e]) == (e < taps ? bits(abi[(size_t)i * taps + e]) : 0u);
                gw.check(eq, "%d/%d index %d", sc[s].src, sc[s].dst, subset_first(sub) + i);
            }
        }
        for (int f = 0; f < N_FIRST; f++) {
            const int first = first_of(f), n = rows_at(first);
            const int period = lb_area_period(sc[s].v, first), start = lb_area_start_of(period, first);  // the host scan
            int abi_start = -1, t2 = 0;
            std::vector<float> scratch((size_t)n * MAX_T);
            if (tsvpp_letterbox_area_rows(sc[s].v, first, n, scratch.data(), (int)scratch.size(), &t2, &abi_start) != n) return 2;
            const int2 *d = &g_p[((size_t)s * N_FIRST + f) * 64];
            bool eq = abi_start == start;
            for (int lane = 0; lane < 64; lane++) eq = eq && d[lane].x == period && d[lane].y == start;
            pe.check(eq, "%d/%d first %d: device lane 0 (period %d, start %d) host (%d, %d) C ABI start %d", sc[s].src, sc[s].dst, first, d[0].x, d[0].y, period, start,
                     abi_start);
            if (!abi_rows(sc[s].v, first, n, abi, taps)) return 2;
            for (int i = 0; i < n; i++) {
                const float *w = &g_jump[(((size_t)s * N_FIRST + f) * N_SUB + i) * MAX_T];
                bool same_row = true;
                for (int e = 0; e < MAX_T; e++) same_row = same_row && bits(w[e]) == (e < taps ? bits(abi[(size_t)i * taps + e]) : 0u);
                ju.check(same_row, "%d/%d first %d index %d (start %d)", sc[s].src, sc[s].dst, first, first + i, d[0].y);
            }
        }
    }
    const bool a = gr.report(), b = gw.report(), c = pe.report(), d = ju.report();
    ok = a && b && c && d;
    return 0;
}

} // namespace

int main(int argc, char **argv) {
    const bool host_only = argc > 1 && strcmp(argv[1], "--host") == 0;
    if (argc > 1 && !host_only) {
        fprintf(stderr, "usage: vpp_twins [--host]\n");
        return 2;
    }
    const std::vector<Scale> sc = scales();
    for (const Scale &s : sc)
        if (!(s.v > 1.0f) || roi_area_taps(s.v) > MAX_T) {
            fprintf(stderr, "scale %d/%d is outside the generator's domain\n", s.src, s.dst);
            return 2;
        }
    // the host's run of the generator: what both halves compare with
    std::vector<RoiAreaRow> rows(sc.size() * N_INDEX);
    for (size_t s = 0; s < sc.size(); s++) {
        RoiAreaGen g;
        for (int j = 0; j < N_INDEX; j++) rows[s * N_INDEX + j] = roi_area_step(sc[s].v, g);
    }
    bool host_ok = false, device_ok = true;
    int rc = host_half(sc, rows, host_ok);
    if (rc == 0 && !host_only) rc = device_half(sc, rows, device_ok);
    if (rc != 0) {
        fprintf(stderr, "a call failed\n");
        return rc;
    }
    return host_ok && device_ok ? 0 : 1;
}
