// vpp_letterbox_area.h -- launch descriptor and chain geometry of the AREA letterbox kernel (vpp_letterbox_area.hip), shared with the host API
// (tsvpp_letterbox_area.cpp: tsvpp_convert_letterbox_area / tsvpp_describe_letterbox_area / tsvpp_letterbox_area_rows).  The records, the canvas and the
// rectangle are the letterbox kernel's (vpp_letterbox.h), the weight rows and their generator the AREA region-of-interest kernel's (vpp_rois.h); what this file
// adds is where a tile's generator chain may START.  Product code -- never includes anything from oracle/.
#pragma once
#include "vpp_letterbox.h"

#pragma clang fp contract(off)

namespace tsvpp {

// One launch: LbLaunch, and behind its every field the bytes of the weight rows in front of the staged footprint (a multiple of 16; roi_area_lds of the largest
// tap counts among the launch's down-scale frames, 0 without one).  A struct of its own: vpp_letterbox.hip's kernels keep the argument block they have.
struct LbAreaLaunch : LbLaunch {
    int32_t area_lds;
};
static_assert(sizeof(LbAreaLaunch) + 256 <= 4096, "LbAreaLaunch no longer fits the kernarg segment");

// ---- where a chain starts ----------------------------------------------------------------------------------------------------------------------------------
// roi_area_step (vpp_rois.h) resets its state (k, carry) to (0, 0) behind the row whose successor index k passes build_area_rows' closing test: `(float)k * scale`
// has no fraction above FLT_EPSILON.  The test reads the pattern index and the scale, never the carry, so the resets are periodic: with P the first k >= 1 that
// passes, row j is row j % P, and a generator started at any multiple of P with state (0, 0) produces, bit for bit, the rows the generator started at 0 produces
// from there on.  A tile whose first index is `first` therefore starts its chain at (first / P) * P and runs first % P steps in front of its rows instead of
// `first`.  P is NOT src / gcd: the float product decides (1920 -> 608 closes at 57, not at 19), so the search evaluates the predicate itself.

// the closing test of build_area_rows (tsvpp_area.cpp) / roi_area_step for pattern index k, written as there
__host__ __device__ __forceinline__ bool lb_area_closes(float scale, int k) {
    const float pos = (float)k * scale;
    return !(pos - (float)(int)pos > FLT_EPSILON);
}

// The start of the chain of (scale, first): the largest multiple of the pattern's period that is <= first; 0 where the pattern does not close in 1 .. first (the
// chain then runs from index 0, as vpp_rois_area.hip's does).  The period is the axis's: the chroma chain of a tile, whose range [first >> 1, ...] begins below
// the luma range, rounds its own first index with the period the luma search found (a period above first >> 1 gives 0 -- what a search of its own would answer).
// The tests of k = 1 .. first are independent of one another.  Host: a serial scan.  Device: EVERY lane of a wave calls this with wave-uniform arguments; the wave
// tests 64 indices per round and a ballot names the first that passes.
__host__ __device__ __forceinline__ int lb_area_period(float scale, int first) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int lane = (int)(threadIdx.x & 63);
    for (int base = 1; base <= first; base += 64) {
        const int k = base + lane;
        const unsigned long long hit = __ballot(k <= first && lb_area_closes(scale, k));
        if (hit) return base + __builtin_ctzll(hit);
    }
    return 0;
#else
    for (int k = 1; k <= first; k++)
        if (lb_area_closes(scale, k)) return k;
    return 0;
#endif
}
// ... from the period (0: none found) to the start
__host__ __device__ __forceinline__ int lb_area_start_of(int period, int first) { return period > 0 ? (first / period) * period : 0; }
__host__ __device__ __forceinline__ int lb_area_chain_start(float scale, int first) { return lb_area_start_of(lb_area_period(scale, first), first); }

// (vpp_letterbox_area.hip) launches -- or, with `dry_run`, only names -- the kernel of (out, vec, staged); `lds_bytes` = L.area_lds + L.lds_bytes
hipError_t launch_letterbox_area(OutKind out, bool vec, bool staged, const LbAreaLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                 size_t name_len, bool dry_run);
// (vpp_letterbox_area_tensor.hip) the same for the tensor instantiations: `out` is O_F32_PLANAR or O_Y800_F32, the element is L.spec.dtype's
hipError_t launch_letterbox_area_tensor(OutKind out, bool vec, bool staged, const LbAreaLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                        size_t name_len, bool dry_run);

} // namespace tsvpp
