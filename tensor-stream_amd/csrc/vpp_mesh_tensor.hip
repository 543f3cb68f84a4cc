// vpp_mesh_tensor.hip -- the tensor instantiations of the control-grid kernel (tsvpp_convert_mesh_tensor, include/tsvpp.h): vpp_mesh_core.h's kernel with the store
// of vpp_tensor_store.h -- (q - mean[c]) * scale[c] as fp32 (EL_F32) or as fp16 / bf16 (EL_HALF, which branches on the launch's dtype).  A translation unit of its
// own: the library builds in parallel and vpp_mesh.hip's object does not grow.  Planar RGB / BGR and Y800 only.
//
// Arithmetic contract as everywhere: single IEEE-754 operations, contraction off.  Written for wave64 / CDNA4 only.

#include "vpp_mesh_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

hipError_t launch_mesh_tensor(OutKind out, bool vec, bool staged, bool border, const MeshLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                              size_t name_len, bool dry_run) {
    const int dt = L.spec.dtype;
    if (!tile_tensor(out, dt)) return hipErrorNotSupported;
    if (name && name_len)
        snprintf(name, name_len, "vpp_mesh_tensor<%s,%s,%s,%s,%s>", tensor_planes_name(out), tensor_el_name(dt), vec_name(vec), staged_name(staged), border_name(border));
    if (dry_run) return hipSuccess;
    return with_tile_tensor(out, dt, [&](auto O, auto E) {
        return with_vec_staged(vec, staged, [&](auto V, auto S) {
            return with_border(border, [&](auto B) {
                constexpr bool STAGED = decltype(S)::value; // (the gather kernel takes no dynamic LDS)
                hipLaunchKernelGGL((vpp_mesh_kernel<decltype(O)::value, decltype(V)::value, STAGED, decltype(B)::value, decltype(E)::value>), dim3(grid), dim3(ROI_THREADS), STAGED ? lds_bytes : 0, stream, L);
                return hipGetLastError();
            });
        });
    });
}

} // namespace tsvpp
