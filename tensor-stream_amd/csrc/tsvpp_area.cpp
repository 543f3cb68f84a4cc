// tsvpp_area.cpp -- the AREA down-scale on the host: the weight table of a scale, the tables of a context on its device, and the AREA fields of a launch
// descriptor.  The reference rebuilds its tables on every frame (src/Resize.cu:436-452 mallocs, copies and leaks them per frame); this library builds them once.
#include <cfloat>
#include <cmath>
#include <cstring>

#include "tsvpp_host.h"

using namespace tsvpp;

namespace {

// Largest E such that taps 1 .. E - 1 weigh exactly 1.0f in every row of a weight table (the reference's rows are [rest] 1 ... 1 [last
// fraction]: E >= taps - 1 or taps - 2).
int area_ones_end(const std::vector<float> &tab, int rows, int taps) {
    int end = taps;
    for (int r = 0; r < rows; r++) {
        int k = 1;
        while (k < end && tab[(size_t)r * taps + k] == 1.0f) k++;
        end = k;
    }
    return end;
}

// Integer form of a weight table if all weights are dyadic: w * 2^shift integral, shift <= 6.
bool quantise_area_rows(const std::vector<float> &tab, int rows, int taps, std::vector<AreaQRow> &q, int &shift) {
    if (taps > 8) return false;
    for (shift = 0; shift <= 6; shift++) {
        bool ok = true;
        for (float w : tab) {
            const float s = w * (float)(1 << shift);
            if (s != std::floor(s) || s > 255.0f) { ok = false; break; }
        }
        if (ok) break;
    }
    if (shift > 6) return false;
    q.assign((size_t)rows, AreaQRow{});
    for (int r = 0; r < rows; r++) {
        AreaQRow &e = q[(size_t)r];
        for (int k = 0; k < taps; k++) {
            const uint32_t wi = (uint32_t)(tab[(size_t)r * taps + k] * (float)(1 << shift));
            e.sum += (int32_t)wi;
            e.w[k >> 2] |= wi << (8 * (k & 3));
            e.wu[k >> 1] |= wi << (16 * (k & 1));
        }
    }
    return true;
}

constexpr int kMaxPatternRows = 65536; // the reference's generator has no bound (can spin forever)

// Weight rows of the AREA down-scale, semantics of generateResizePattern (reference
// src/Resize.cu:359-386) in plain float arithmetic.  Each row is emitted with exactly
// taps = ceil(scale) entries: the device code never reads further (src/Resize.cu:162-169),
// so a row's optional (taps+1)-th entry is dropped here instead of being uploaded.
bool build_area_rows(float scale, std::vector<float> &tab, int &rows, int &taps) {
    taps = (int)std::ceil((double)scale);
    rows = 0;
    tab.clear();
    if (!(scale > 1.0f) || taps < 1) return false;
    float carry = 0.0f; // part of the next source pixel already consumed by the previous row
    for (int k = 0;; k++) {
        const float pos = (float)k * scale;
        const bool more = (pos == 0.0f) || (pos - (float)(int)pos > FLT_EPSILON);
        if (!more) break;
        if (rows >= kMaxPatternRows) return false;
        std::vector<float> row;
        float left = scale;
        if (carry != 0.0f) {
            row.push_back(carry);
            left = left - carry;
        }
        while (left - 1.0f > 0.0f) {
            row.push_back(1.0f);
            left = left - 1.0f;
        }
        if (left > FLT_EPSILON) {
            row.push_back(left);
            carry = 1.0f - left;
        }
        row.resize((size_t)taps, 0.0f); // pads short rows with 0, truncates long ones
        tab.insert(tab.end(), row.begin(), row.end());
        rows++;
    }
    return rows > 0;
}

// The axis record of a scale; `tab` / `q` receive the float rows and, if dyadic, the integer rows (for the uploads of get_area_table).
bool area_axis(float scale, AreaAxis &a, std::vector<float> &tab, std::vector<AreaQRow> &q) {
    if (!build_area_rows(scale, tab, a.rows, a.taps)) return false;
    a.nk = (a.taps + 3) / 4;
    a.ones_end = area_ones_end(tab, a.rows, a.taps);
    a.dyadic = quantise_area_rows(tab, a.rows, a.taps, q, a.shift);
    if (a.dyadic) {
        a.uniform_sum = q[0].sum;
        for (const AreaQRow &row : q)
            if (row.sum != q[0].sum) a.uniform_sum = 0;
    }
    return true;
}

// Integer box sums are exact (and equal to the reference's float accumulation) while 255 * sum(wx) * sum(wy) stays
// below 2^24; one divisor for the whole frame allows an exact integer division by a constant in the kernel.
bool dyadic_usable(float xr, float yr, int shift_x, int shift_y) {
    return (double)255 * ((double)xr * (1 << shift_x) + 1) * ((double)yr * (1 << shift_y) + 1) < 16777216.0;
}

// Does an AREA down-scale with these tables want the divisor table of the float-weight kernels (get_area_div)?  Not where the integer tables exist, and
// tables above 2^18 entries are not built (the kernel then sums the weights itself).
bool wants_area_div(const Knobs &kn, const AreaTable &tx, const AreaTable &ty) {
    return !(tx.qdev && ty.qdev) && kn.area_divtab && (long)tx.rows * ty.rows <= (1L << 18);
}

// The AREA down-scale fields of the launch descriptor.  "Dyadic" means that both integer tables are there (qdev); `div` may be null whatever wants_area_div said.
void set_area_desc(const Plan &pl, const AreaTable &tx, const AreaTable &ty, const float *div, LaunchDesc &d) {
    d.patx = tx.dev;
    d.nx = tx.rows;
    d.rx = tx.taps;
    d.paty = ty.dev;
    d.ny = ty.rows;
    d.ry = ty.taps;
    d.patx4 = tx.dev4;
    d.nkx = tx.nk;
    d.paty4 = ty.dev4;
    d.nky = ty.nk;
    d.as_ones_x = tx.ones_end;
    d.area_div = div;
    if (tx.qdev && ty.qdev && dyadic_usable(pl.xr, pl.yr, tx.shift, ty.shift)) {
        d.qx = tx.qdev;
        d.qy = ty.qdev;
        d.box_rx = (tx.rows == 1 && tx.shift == 0 && tx.uniform_sum == tx.taps) ? tx.taps : 0; // one row of all ones
        d.box_ry = (ty.rows == 1 && ty.shift == 0 && ty.uniform_sum == ty.taps) ? ty.taps : 0;
        // one divisor for the whole frame -> exact integer division by a constant in the kernel
        if (tx.uniform_sum > 0 && ty.uniform_sum > 0 && (long)tx.uniform_sum * ty.uniform_sum < 4096)
            d.area_rcp = 1.0f / (float)(tx.uniform_sum * ty.uniform_sum);
    }
}

// A host vector as a fresh device allocation; on failure nothing stays allocated, `dev` is null and the runtime's last error is cleared: the failure is this
// function's result, and a launcher that ends in `return hipGetLastError()` must not find it later -- a first AREA conversion refused inside a capture made the
// thread's NEXT successful launch report the capture error.
template <class T> hipError_t upload(const std::vector<T> &v, T *&dev) {
    dev = nullptr;
    hipError_t e = hipMalloc((void **)&dev, v.size() * sizeof(T));
    if (e == hipSuccess && (e = hipMemcpy(dev, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice)) != hipSuccess) {
        (void)hipFree(dev);
        dev = nullptr;
    }
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
}

int get_area_table(tsvpp_ctx *ctx, float scale, AreaTable &out) {
    uint32_t key;
    std::memcpy(&key, &scale, 4);
    std::lock_guard<std::mutex> lk(ctx->area_mu);
    auto it = ctx->area.find(key);
    if (it != ctx->area.end()) {
        out = it->second;
        return TSVPP_OK;
    }
    std::vector<float> tab;
    std::vector<AreaQRow> q;
    AreaTable t;
    if (!area_axis(scale, t, tab, q)) return TSVPP_UNSUPPORTED;
    const hipError_t e = upload(tab, t.dev);
    if (e != hipSuccess) return (int)e;
    std::vector<float> pad((size_t)t.rows * 4 * t.nk, 0.0f);
    for (int r = 0; r < t.rows; r++)
        for (int k = 0; k < t.taps; k++) pad[(size_t)r * 4 * t.nk + k] = tab[(size_t)r * t.taps + k];
    t.host4 = std::make_shared<std::vector<float>>(pad);
    if (upload(pad, t.dev4) != hipSuccess) {
        (void)hipFree(t.dev);
        return TSVPP_ERROR;
    }
    if (t.dyadic) (void)upload(q, t.qdev); // (a failed upload leaves it null: the request then runs the float-weight kernels)
    ctx->area[key] = t;
    out = t;
    return TSVPP_OK;
}

// Divisor table of the float AREA kernels that keep one output column per lane (vpp_area_cols.hip): the reference
// accumulates `divide += weight` next to `colorSum = fma(data, weight, colorSum)` (src/Resize.cu:160-178), and the sum depends
// only on the column's and the row's weight patterns -- nx * ny distinct values per geometry.  Built here with the kernel's
// own fp32 operations in the kernel's order (product rounded to fp32, then added; rows outer, the 4 * nk zero-padded taps
// inner), so the kernel can load the divisor instead of spending one add per tap and lane on it.  Asked for only where
// wants_area_div says so.
#pragma clang fp contract(off)
// The table is an optimisation, never a requirement (the kernels sum the weights themselves when it is null): while `stream`
// is capturing, or when the allocation fails, nothing is built or cached and the call still succeeds -- a first conversion
// inside a hipGraph capture without tsvpp_prepare_batch runs the self-summing kernel instead of failing.
int get_area_div(tsvpp_ctx *ctx, float xr, float yr, const AreaTable &tx, const AreaTable &ty, const float *&out, hipStream_t stream) {
    out = nullptr;
    uint32_t kx, ky;
    std::memcpy(&kx, &xr, 4);
    std::memcpy(&ky, &yr, 4);
    const uint64_t key = ((uint64_t)kx << 32) | ky;
    std::lock_guard<std::mutex> lk(ctx->area_mu);
    auto it = ctx->area_div.find(key);
    if (it != ctx->area_div.end()) {
        out = it->second;
        return TSVPP_OK;
    }
    float *dev = nullptr;
    if (tx.host4 && ty.host4) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        // (the NULL stream is never queried: asking the legacy stream while another stream captures in global mode invalidates that capture)
        if (stream && hipStreamIsCapturing(stream, &cap) != hipSuccess) (void)hipGetLastError();
        if (cap != hipStreamCaptureStatusNone) { // no allocation, no synchronous copy during capture
            g_build_declined = true;
            return TSVPP_OK;
        }
        const int tx4 = 4 * tx.nk, ty4 = 4 * ty.nk;
        std::vector<float> tab((size_t)tx.rows * ty.rows);
        for (int jx = 0; jx < tx.rows; jx++) {
            const float *wx = tx.host4->data() + (size_t)jx * tx4;
            for (int iy = 0; iy < ty.rows; iy++) {
                const float *wy = ty.host4->data() + (size_t)iy * ty4;
                volatile float div = 0.0f; // volatile: every product and every partial sum is rounded to fp32, as on the device
                for (int a = 0; a < ty.taps; a++)
                    for (int k = 0; k < tx4; k++) {
                        volatile float wgt = wx[k] * wy[a];
                        div = div + wgt;
                    }
                tab[(size_t)jx * ty.rows + iy] = div;
            }
        }
        if (upload(tab, dev) != hipSuccess) {
            (void)hipGetLastError();
            return TSVPP_OK; // out stays null
        }
    }
    ctx->area_div[key] = dev;
    out = dev;
    return TSVPP_OK;
}

} // namespace

namespace tsvpp {

// An AREA down-scale's tables -- both axes and, where wanted, the divisor table -- into its descriptor: tsvpp_prepare_batch builds them ahead, a conversion looks them up.
int area_desc(tsvpp_ctx *ctx, const Plan &pl, hipStream_t stream, LaunchDesc &d) {
    if (pl.mode != M_AREA_DOWN) return TSVPP_OK;
    AreaTable tx, ty;
    const float *div = nullptr;
    int sts = get_area_table(ctx, pl.xr, tx);
    if (sts == TSVPP_OK) sts = get_area_table(ctx, pl.yr, ty);
    if (sts == TSVPP_OK && wants_area_div(ctx->knobs, tx, ty)) sts = get_area_div(ctx, pl.xr, pl.yr, tx, ty, div, stream);
    if (sts == TSVPP_OK) set_area_desc(pl, tx, ty, div, d);
    return sts;
}

// The dry run (tsvpp_describe): the tables' properties without touching a device, stand-ins for their device copies.
int area_desc(const Knobs &kn, const Plan &pl, LaunchDesc &d) {
    if (pl.mode != M_AREA_DOWN) return TSVPP_OK;
    static float dummy_f[4] = { 0, 0, 0, 0 };
    static AreaQRow dummy_q = {};
    AreaTable tab[2];
    for (int axis = 0; axis < 2; axis++) {
        std::vector<float> rows;
        std::vector<AreaQRow> q;
        if (!area_axis(axis ? pl.yr : pl.xr, tab[axis], rows, q)) return TSVPP_UNSUPPORTED;
        tab[axis].dev = tab[axis].dev4 = dummy_f;
        if (tab[axis].dyadic) tab[axis].qdev = &dummy_q;
    }
    set_area_desc(pl, tab[0], tab[1], wants_area_div(kn, tab[0], tab[1]) ? dummy_f : nullptr, d);
    return TSVPP_OK;
}

} // namespace tsvpp

extern "C" int tsvpp_area_pattern(float scale, float *out, int max_floats, int *taps) {
    std::vector<float> tab;
    int rows = 0, t = 0;
    if (!build_area_rows(scale, tab, rows, t)) return TSVPP_UNSUPPORTED;
    if (taps) *taps = t;
    if (out && (long)tab.size() <= (long)max_floats) std::memcpy(out, tab.data(), tab.size() * sizeof(float));
    return rows;
}

// DEBUG ONLY (tests): how many AREA tables the context has cached (weight tables per scale + divisor tables per pair of scales)
extern "C" int tsvpp_debug_area_tables(tsvpp_ctx *ctx) {
    if (!ctx) return TSVPP_ERROR;
    std::lock_guard<std::mutex> lk(ctx->area_mu);
    return (int)(ctx->area.size() + ctx->area_div.size());
}
