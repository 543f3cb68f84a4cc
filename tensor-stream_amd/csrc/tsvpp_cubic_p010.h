// tsvpp_cubic_p010.h -- what the host paths of the P010 BICUBIC calls share (tsvpp_rois_p010_bicubic.cpp, tsvpp_letterbox_p010_bicubic.cpp): the answer to a
// request whose walk does not fit a knob-shrunk LDS budget.
#pragma once
#include "tsvpp_tiles.h"
#include "vpp_cubic_p010.h"

namespace tsvpp {

// TSVPP_UNSUPPORTED where the largest tile of a launch does not fit the workgroup's LDS budget even with one-row bands; decided on the host, before the skeleton
// touches a device.  The default budget holds every request within the limits (Hbuf of 259 rows and two one-row bands of the widest row: 18.2 KiB, behind at
// most 12 KiB of the store side's static LDS), so the launch groups are only walked where a knob has shrunk it.  `outs`: the convert call's (null: describe,
// which says `aligned`).  A request the plan refuses is left to the skeleton.  PATH: a tile path whose stage_budget leaves the band height in L.band.
template <class PATH> int cubic_fit_status(const PATH &path, const Knobs &kn, void *const *outs, bool aligned) {
    const int widest = std::max(roi_chunks(2 * CUBIC_TILE_MAX_HROWS), roi_chunks(4 * (CUBIC_TILE_MAX_HROWS / 2 + 2)));
    if (!kn.force_gather && kn.lds_budget_kb * 1024 - roi_static_lds(O_F32_MERGED, true) >= cubic_lds(CUBIC_TILE_MAX_HROWS, 1, widest)) return TSVPP_OK;
    RoiPlan pl;
    if (tile_request(path, pl) != TSVPP_OK) return TSVPP_OK;
    const int n = path.items(), limit = path.limit(pl);
    for (int base = 0; base < n; base += limit) {
        const int cnt = std::min(n - base, limit);
        const bool vec = (outs ? outs_aligned16(outs + base, cnt) : aligned) && !narrow_tail(pl);
        typename PATH::Launch L;
        tile_fill(path, kn, pl, nullptr, base, cnt, vec, L);
        if (L.band < 1) return TSVPP_UNSUPPORTED;
    }
    return TSVPP_OK;
}

} // namespace tsvpp
