// vpp_letterbox_area_tensor.hip -- the tensor instantiations of the AREA letterbox kernel (tsvpp_convert_letterbox_area with a spec, include/tsvpp.h):
// vpp_letterbox_area_core.h's kernel with the store of vpp_tensor_store.h -- (q - mean[c]) * scale[c] as fp32 (EL_F32) or as fp16 / bf16 (EL_HALF, which branches on
// the launch's dtype); the pad sample goes through it like every other.  A translation unit of its own: the library builds in parallel and
// vpp_letterbox_area.hip's object does not grow.  Planar RGB / BGR and Y800 only.
//
// Arithmetic contract as everywhere: single IEEE-754 operations in the reference's order, contraction off.  Written for wave64 / CDNA4 only.

#include "vpp_letterbox_area_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

hipError_t launch_letterbox_area_tensor(OutKind out, bool vec, bool staged, const LbAreaLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                        size_t name_len, bool dry_run) {
    const int dt = L.spec.dtype;
    if (!tile_tensor(out, dt)) return hipErrorNotSupported;
    if (name && name_len) snprintf(name, name_len, "vpp_letterbox_area_tensor<%s,%s,%s,%s>", tensor_planes_name(out), tensor_el_name(dt), vec_name(vec), staged_name(staged));
    if (dry_run) return hipSuccess;
    return with_tile_tensor(out, dt, [&](auto O, auto E) {
        return with_vec_staged(vec, staged, [&](auto V, auto S) { // (lds_bytes either way: the weight rows need LDS in the gather kernel too)
            hipLaunchKernelGGL((vpp_letterbox_area_kernel<decltype(O)::value, decltype(V)::value, decltype(S)::value, decltype(E)::value>), dim3(grid), dim3(ROI_THREADS), lds_bytes, stream, L);
            return hipGetLastError();
        });
    });
}

} // namespace tsvpp
