// vpp_letterbox_p010_bicubic_tensor.hip -- the tensor instantiations of the P010 BICUBIC letterbox kernel (tsvpp_convert_letterbox_p010_bicubic with a spec,
// include/tsvpp.h): vpp_letterbox_p010_bicubic_core.h's kernel storing cvt(dtype, (k / 1023 - mean[c]) * scale[c]) as fp32 (EL_F32) or as fp16 / bf16 (EL_HALF);
// the pad sample goes through it like every other.  A translation unit of its own, as vpp_letterbox_p010_tensor.hip.  Planar RGB / BGR and Y800 only.
// Written for wave64 / CDNA4 only.

#include "vpp_letterbox_p010_bicubic_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

hipError_t launch_letterbox_p010_bicubic_tensor(OutKind out, bool vec, const LbCubicLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                                size_t name_len, bool dry_run) {
    const int dt = L.spec.dtype;
    if (!tile_tensor(out, dt)) return hipErrorNotSupported;
    if (name && name_len) snprintf(name, name_len, "vpp_letterbox_p010_bicubic_tensor<%s,%s,%s>", tensor_planes_name(out), tensor_el_name(dt), vec_name(vec));
    if (dry_run) return hipSuccess;
    return with_tile_tensor(out, dt, [&](auto O, auto E) {
        if (vec) hipLaunchKernelGGL((vpp_letterbox_p010_bicubic_kernel<decltype(O)::value, true, decltype(E)::value>), dim3(grid), dim3(ROI_THREADS), lds_bytes, stream, L);
        else hipLaunchKernelGGL((vpp_letterbox_p010_bicubic_kernel<decltype(O)::value, false, decltype(E)::value>), dim3(grid), dim3(ROI_THREADS), lds_bytes, stream, L);
        return hipGetLastError();
    });
}

} // namespace tsvpp
