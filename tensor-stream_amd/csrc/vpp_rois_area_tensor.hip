// vpp_rois_area_tensor.hip -- the tensor instantiations of the AREA region-of-interest kernel (tsvpp_convert_rois_tensor with TSVPP_AREA, include/tsvpp.h):
// vpp_rois_area_core.h's kernel with the store of vpp_tensor_store.h -- (q - mean[c]) * scale[c] as fp32 (EL_F32) or as fp16 / bf16 (EL_HALF, which branches on
// the launch's dtype).  A translation unit of its own: the library builds in parallel and vpp_rois_area.hip's object does not grow.  Planar RGB / BGR and Y800 only.
//
// Arithmetic contract as everywhere: single IEEE-754 operations in the reference's order, contraction off.  Written for wave64 / CDNA4 only.

#include "vpp_rois_area_core.h"

#pragma clang fp contract(off)

namespace tsvpp {

namespace {

template <int OUT, int EL, bool VEC, bool STAGED> hipError_t launch_k(const RoiLaunch &L, unsigned grid, size_t lds, hipStream_t stream) {
    hipLaunchKernelGGL((vpp_rois_area_kernel<OUT, VEC, STAGED, EL>), dim3(grid), dim3(ROI_THREADS), lds, stream, L);
    return hipGetLastError();
}
template <int OUT, int EL> hipError_t launch_oe(bool vec, bool staged, const RoiLaunch &L, unsigned grid, size_t lds, hipStream_t stream) {
    if (vec) return staged ? launch_k<OUT, EL, true, true>(L, grid, lds, stream) : launch_k<OUT, EL, true, false>(L, grid, lds, stream);
    return staged ? launch_k<OUT, EL, false, true>(L, grid, lds, stream) : launch_k<OUT, EL, false, false>(L, grid, lds, stream);
}

} // namespace

hipError_t launch_rois_area_tensor(OutKind out, bool vec, bool staged, const RoiLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                   size_t name_len, bool dry_run) {
    const int dt = L.spec.dtype;
    if ((out != O_F32_PLANAR && out != O_Y800_F32) || (dt != TSVPP_F32 && dt != TSVPP_F16 && dt != TSVPP_BF16)) return hipErrorNotSupported; // never a fallback
    if (name && name_len)
        snprintf(name, name_len, "vpp_rois_area_tensor<%s,%s,%s,%s>", out == O_Y800_F32 ? "Y800" : "PLANAR", tensor_el_name(dt), vec ? "vec" : "elem",
                 staged ? "staged" : "gather");
    if (dry_run) return hipSuccess;
    const int el = tensor_el(dt);
    if (out == O_Y800_F32)
        return el == EL_F32 ? launch_oe<O_Y800_F32, EL_F32>(vec, staged, L, grid, lds_bytes, stream) : launch_oe<O_Y800_F32, EL_HALF>(vec, staged, L, grid, lds_bytes, stream);
    return el == EL_F32 ? launch_oe<O_F32_PLANAR, EL_F32>(vec, staged, L, grid, lds_bytes, stream) : launch_oe<O_F32_PLANAR, EL_HALF>(vec, staged, L, grid, lds_bytes, stream);
}

} // namespace tsvpp
