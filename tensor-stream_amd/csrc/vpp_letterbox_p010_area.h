// vpp_letterbox_p010_area.h -- what the P010 AREA letterbox kernel (vpp_letterbox_p010_area.hip, vpp_letterbox_p010_area_tensor.hip) shares with the host API
// (tsvpp_letterbox_p010_area.cpp: tsvpp_convert_letterbox_p010_area / tsvpp_describe_letterbox_p010_area).  The launch block is the P010 letterbox call's LbLaunch
// (byte addresses and pitches, sizes in samples, pad 0..1023; xr / yr are not read) with the band walk's two numbers behind it.  Product code -- never includes
// anything from oracle/.
#pragma once
#include "vpp_box_p010.h"
#include "vpp_letterbox.h"

namespace tsvpp {

struct LbBoxLaunch : LbLaunch {
    int32_t band;     // source rows per band (vpp_box_p010.h), 1 .. BOX_BAND_MAX_ROWS
    int32_t band_cpr; // 16-byte chunks per staged row the band buffers are sized for: the widest footprint row of the launch's tiles, either plane
};
static_assert(sizeof(LbBoxLaunch) + 256 <= 4096, "LbBoxLaunch no longer fits the kernarg segment");

// chunks per staged row of inner columns [a0, a1] (a0 even, a1 odd) of a frame src_w wide into a rectangle `width` wide: luma words, chroma (U, V) word pairs
__host__ __device__ inline int box_cpr_y(int a0, int a1, int src_w, int width) {
    int lo, hi;
    box_span(a0, a1, src_w, width, lo, hi);
    return roi_chunks(2 * (hi - lo + 1));
}
__host__ __device__ inline int box_cpr_uv(int a0, int a1, int src_w, int width) {
    int lo, hi;
    box_span(a0 >> 1, a1 >> 1, src_w >> 1, width >> 1, lo, hi);
    return roi_chunks(4 * (hi - lo + 1));
}

// (vpp_letterbox_p010_area.hip) launches -- or, with `dry_run`, only names -- the kernel of (out, vec)
hipError_t launch_letterbox_p010_area(OutKind out, bool vec, const LbBoxLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name, size_t name_len,
                                      bool dry_run);
// (vpp_letterbox_p010_area_tensor.hip) the same for the tensor instantiations: `out` is O_F32_PLANAR or O_Y800_F32, the element is L.spec.dtype's
hipError_t launch_letterbox_p010_area_tensor(OutKind out, bool vec, const LbBoxLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name, size_t name_len,
                                             bool dry_run);

} // namespace tsvpp
