// vpp_letterbox_p010.h -- what the P010 letterbox kernel (vpp_letterbox_p010.hip, vpp_letterbox_p010_tensor.hip) shares with the host API
// (tsvpp_letterbox_p010.cpp: tsvpp_convert_letterbox_p010 / tsvpp_describe_letterbox_p010).  The launch block is the letterbox call's, LbLaunch (vpp_letterbox.h):
// plane addresses and pitches are in BYTES, the frame's size in samples, the pad sample 0..1023.  What this file adds is the LDS need of a tile whose footprint is
// staged as raw 16-bit words.  Product code -- never includes anything from oracle/.
#pragma once
#include "vpp_letterbox.h"

namespace tsvpp {

// Bytes of one staged row: `samples` luma words, or `pairs` interleaved (U, V) word pairs
__host__ __device__ inline int p010_span_y(int samples) { return 2 * samples; }
__host__ __device__ inline int p010_span_uv(int pairs) { return 4 * pairs; }
// The LDS-DMA loop fills 64 chunk slots per wave instruction (stage_plane_dma, vpp_device.h): a plane is allocated up to a multiple of 64 slots
__host__ __device__ inline int p010_slots(int chunks) { return (chunks + 63) & ~63; }
// LDS bytes of a staged tile of `ny` luma rows of `cpr_y` 16-byte chunks and `nuv` chroma rows of `cpr_uv`: twice the 8-bit call's roi_lds_need, plus the slot
// padding.  ONE statement for the host's staged= count and budget and for the kernel's per-tile decision.
__host__ __device__ inline int p010_lds_bytes(int ny, int cpr_y, int nuv, int cpr_uv) { return 16 * (p010_slots(ny * cpr_y) + p010_slots(nuv * cpr_uv)); }
__host__ __device__ inline int p010_lds_need(const RoiFootprint &f, bool luma_only) {
    return p010_lds_bytes(f.yhi - f.ylo + 1, roi_chunks(p010_span_y(f.xhi - f.xlo + 1)), luma_only ? 0 : f.cyhi - f.cylo + 1, roi_chunks(p010_span_uv(f.cxhi - f.cxlo + 1)));
}
// ... and whether it is staged at all: the bound on a row's chunks is the 8-bit call's (roi_stageable), which also keeps the slot -> (row, chunk) multiply-high
// of the staging loop exact (slots * chunks per row stays far below 2^32)
__host__ __device__ inline bool p010_stageable(const RoiFootprint &f) {
    return roi_chunks(p010_span_y(f.xhi - f.xlo + 1)) <= ROI_THREADS && roi_chunks(p010_span_uv(f.cxhi - f.cxlo + 1)) <= ROI_THREADS;
}

// (vpp_letterbox_p010.hip) launches -- or, with `dry_run`, only names -- the kernel of (mode, out, vec, staged); mode is M_NEAREST or M_BILINEAR
hipError_t launch_letterbox_p010(Mode mode, OutKind out, bool vec, bool staged, const LbLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                 size_t name_len, bool dry_run);
// (vpp_letterbox_p010_tensor.hip) the same for the tensor instantiations: `out` is O_F32_PLANAR or O_Y800_F32, the element is L.spec.dtype's
hipError_t launch_letterbox_p010_tensor(Mode mode, OutKind out, bool vec, bool staged, const LbLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                        size_t name_len, bool dry_run);

} // namespace tsvpp
