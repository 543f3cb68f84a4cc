// tsvpp_p010.h -- what the host paths for 10-bit P010 sources share (tsvpp_letterbox_p010.cpp, tsvpp_rois_p010.cpp): the frames of a request seen as byte planes,
// and the frame rules both calls add to their 8-bit call's.
#pragma once
#include <vector>

#include "tsvpp_host.h"

namespace tsvpp {

inline int p010_pitch(int pitch, int width) { return pitch ? pitch : 2 * width; } // an unset pitch means 2 * width bytes

// The frames as the tile skeletons and the 8-bit plans read them: the same planes, pitches in bytes, sizes in samples.  Up to LOCAL frames (one launch's) live on
// the stack; a larger request takes one host array of n records (32 bytes each) for the call -- the only host allocation of the path, and no device allocation ever.
template <int LOCAL> struct P010Frames {
    tsvpp_nv12 local[LOCAL];
    std::vector<tsvpp_nv12> heap;
    const tsvpp_nv12 *data = nullptr;
    P010Frames(int n, const tsvpp_p010 *in) {
        if (!in || n <= 0) return;
        tsvpp_nv12 *fr = local;
        if (n > LOCAL) {
            try {
                heap.resize((size_t)n);
            } catch (...) { // no exception crosses the C boundary: the request is answered as one without frames, TSVPP_ERROR
                return;
            }
            fr = heap.data();
        }
        for (int f = 0; f < n; f++)
            fr[f] = tsvpp_nv12{ (const uint8_t *)in[f].y, (const uint8_t *)in[f].uv, p010_pitch(in[f].pitch_y, in[f].width), p010_pitch(in[f].pitch_uv, in[f].width), in[f].width,
                                in[f].height };
        data = fr;
    }
};

// TSVPP_ERROR class, in front of the 8-bit plan's rules: a frame without size, a pitch below 2 * width bytes, an odd pitch
inline int p010_frames_error(int n, const tsvpp_nv12 *fr) {
    for (int f = 0; f < n; f++) {
        if (fr[f].width <= 0 || fr[f].height <= 0) return TSVPP_ERROR;
        if (fr[f].pitch_y < 2 * (long)fr[f].width || fr[f].pitch_uv < 2 * (long)fr[f].width) return TSVPP_ERROR;
        if ((fr[f].pitch_y | fr[f].pitch_uv) & 1) return TSVPP_ERROR;
    }
    return TSVPP_OK;
}
// ... and, converting (the planes are read, so their addresses must hold 16-bit words): a plane pointer that is not 2-byte aligned
inline int p010_planes_error(int n, const tsvpp_nv12 *fr) {
    for (int f = 0; f < n; f++)
        if (((uintptr_t)fr[f].y | (uintptr_t)fr[f].uv) & 1) return TSVPP_ERROR;
    return TSVPP_OK;
}

// (tsvpp_rois_p010.cpp) the status of a P010 ROI request, NEAREST / BILINEAR; `converting`: the planes are read.  tsvpp_rois_p010_bicubic.cpp asks it with a type
// it accepts, so that every rule in front of the type is this one's
int p010_rois_plan(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *fr, int n_rois, const tsvpp_roi *rois, bool converting, RoiPlan &pl);

} // namespace tsvpp
