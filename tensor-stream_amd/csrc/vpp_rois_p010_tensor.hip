// vpp_rois_p010_tensor.hip -- the tensor instantiations of the P010 region-of-interest kernel (tsvpp_convert_rois_p010 with a spec, include/tsvpp.h):
// vpp_rois_p010_core.h's kernel storing cvt(dtype, (k / 1023 - mean[c]) * scale[c]) as fp32 (EL_F32) or as fp16 / bf16 (EL_HALF, which branches on the launch's
// dtype).  A translation unit of its own, as vpp_rois_tensor.hip.  Planar RGB / BGR and Y800 only.
//
// Arithmetic contract as everywhere: single IEEE-754 operations, contraction off.  Written for wave64 / CDNA4 only.

#include "vpp_rois_p010_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

hipError_t launch_rois_p010_tensor(Mode mode, OutKind out, bool vec, bool staged, const RoiLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                   size_t name_len, bool dry_run) {
    const int dt = L.spec.dtype;
    if ((mode != M_NEAREST && mode != M_BILINEAR) || !tile_tensor(out, dt)) return hipErrorNotSupported;
    if (name && name_len)
        snprintf(name, name_len, "vpp_rois_p010_tensor<%s,%s,%s,%s,%s>", kModeNames[mode], tensor_planes_name(out), tensor_el_name(dt), vec_name(vec), staged_name(staged));
    if (dry_run) return hipSuccess;
    return with_tile_tensor(out, dt, [&](auto O, auto E) {
        return with_vec_staged(vec, staged, [&](auto V, auto S) {
            constexpr bool STAGED = decltype(S)::value; // (the gather kernel takes no dynamic LDS)
            if (mode == M_NEAREST) hipLaunchKernelGGL((vpp_rois_p010_kernel<M_NEAREST, decltype(O)::value, decltype(V)::value, STAGED, decltype(E)::value>), dim3(grid), dim3(ROI_THREADS), STAGED ? lds_bytes : 0, stream, L);
            else hipLaunchKernelGGL((vpp_rois_p010_kernel<M_BILINEAR, decltype(O)::value, decltype(V)::value, STAGED, decltype(E)::value>), dim3(grid), dim3(ROI_THREADS), STAGED ? lds_bytes : 0, stream, L);
            return hipGetLastError();
        });
    });
}

} // namespace tsvpp
