// vpp_rois_sized_tensor.hip -- the tensor instantiations of the per-box-size region-of-interest kernel (tsvpp_convert_rois_sized_tensor, include/tsvpp.h):
// vpp_rois_sized_core.h's kernel with the store of vpp_tensor_store.h, as vpp_rois_tensor.hip is to vpp_rois.hip.  Planar RGB / BGR and Y800 only.
//
// Arithmetic contract as everywhere: single IEEE-754 operations, contraction off.  Written for wave64 / CDNA4 only.

#include "vpp_rois_sized_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

hipError_t launch_rois_sized_tensor(Mode mode, OutKind out, bool vec, bool staged, const SizedLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream,
                                    char *name, size_t name_len, bool dry_run) {
    const int dt = L.spec.dtype;
    if (!tile_mode(mode) || !tile_tensor(out, dt)) return hipErrorNotSupported;
    if (name && name_len)
        snprintf(name, name_len, "vpp_rois_sized_tensor<%s,%s,%s,%s,%s>", kModeNames[mode], tensor_planes_name(out), tensor_el_name(dt), vec_name(vec), staged_name(staged));
    if (dry_run) return hipSuccess;
    return with_tile_mode(mode, [&](auto M) {
        return with_tile_tensor(out, dt, [&](auto O, auto E) {
            return with_vec_staged(vec, staged, [&](auto V, auto S) {
                constexpr bool STAGED = decltype(S)::value; // (the gather kernel takes no dynamic LDS)
                hipLaunchKernelGGL((vpp_rois_sized_kernel<decltype(M)::value, decltype(O)::value, decltype(V)::value, STAGED, decltype(E)::value>), dim3(grid), dim3(ROI_THREADS), STAGED ? lds_bytes : 0, stream, L);
                return hipGetLastError();
            });
        });
    });
}

} // namespace tsvpp
