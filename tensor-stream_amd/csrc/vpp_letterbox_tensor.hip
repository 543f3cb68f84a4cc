// vpp_letterbox_tensor.hip -- the tensor instantiations of the letterbox kernel (tsvpp_convert_letterbox_tensor, include/tsvpp.h): vpp_letterbox_core.h's kernel with
// the store of vpp_tensor_store.h -- (q - mean[c]) * scale[c] as fp32 (EL_F32) or as fp16 / bf16 (EL_HALF, which branches on the launch's dtype); the pad sample
// goes through it like every other.  A translation unit of its own: the library builds in parallel and vpp_letterbox.hip's object does not grow.  Planar RGB /
// BGR and Y800 only.
//
// Arithmetic contract as everywhere: single IEEE-754 operations, contraction off.  Written for wave64 / CDNA4 only.

#include "vpp_letterbox_core.h"

#pragma clang fp contract(off)

namespace tsvpp {

namespace {

const char *const kModeNames[M_COUNT] = { "M_NONE", "M_NEAREST", "M_BILINEAR", "M_BICUBIC", "M_AREA_DOWN", "M_AREA_UP" };

template <int MODE, int OUT, int EL, bool VEC, bool STAGED>
hipError_t launch_k(const LbLaunch &L, unsigned grid, size_t lds, hipStream_t stream) {
    hipLaunchKernelGGL((vpp_letterbox_kernel<MODE, OUT, VEC, STAGED, EL>), dim3(grid), dim3(ROI_THREADS), lds, stream, L);
    return hipGetLastError();
}
template <int MODE, int OUT, int EL>
hipError_t launch_moe(bool vec, bool staged, const LbLaunch &L, unsigned grid, size_t lds, hipStream_t stream) {
    if (vec) return staged ? launch_k<MODE, OUT, EL, true, true>(L, grid, lds, stream) : launch_k<MODE, OUT, EL, true, false>(L, grid, 0, stream);
    return staged ? launch_k<MODE, OUT, EL, false, true>(L, grid, lds, stream) : launch_k<MODE, OUT, EL, false, false>(L, grid, 0, stream);
}
template <int MODE>
hipError_t launch_m(bool luma_only, int el, bool vec, bool staged, const LbLaunch &L, unsigned grid, size_t lds, hipStream_t stream) {
    if (luma_only) return el == EL_F32 ? launch_moe<MODE, O_Y800_F32, EL_F32>(vec, staged, L, grid, lds, stream) : launch_moe<MODE, O_Y800_F32, EL_HALF>(vec, staged, L, grid, lds, stream);
    return el == EL_F32 ? launch_moe<MODE, O_F32_PLANAR, EL_F32>(vec, staged, L, grid, lds, stream) : launch_moe<MODE, O_F32_PLANAR, EL_HALF>(vec, staged, L, grid, lds, stream);
}

} // namespace

hipError_t launch_letterbox_tensor(Mode mode, OutKind out, bool vec, bool staged, const LbLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                   size_t name_len, bool dry_run) {
    const int dt = L.spec.dtype;
    const bool known = (mode == M_NEAREST || mode == M_BILINEAR || mode == M_BICUBIC) && (out == O_F32_PLANAR || out == O_Y800_F32) &&
                       (dt == TSVPP_F32 || dt == TSVPP_F16 || dt == TSVPP_BF16);
    if (!known) return hipErrorNotSupported; // a missing kernel is an error, never a fallback
    if (name && name_len)
        snprintf(name, name_len, "vpp_letterbox_tensor<%s,%s,%s,%s,%s>", kModeNames[mode], out == O_Y800_F32 ? "Y800" : "PLANAR", tensor_el_name(dt),
                 vec ? "vec" : "elem", staged ? "staged" : "gather");
    if (dry_run) return hipSuccess;
    const bool luma_only = out == O_Y800_F32;
    switch (mode) {
    case M_NEAREST: return launch_m<M_NEAREST>(luma_only, tensor_el(dt), vec, staged, L, grid, lds_bytes, stream);
    case M_BILINEAR: return launch_m<M_BILINEAR>(luma_only, tensor_el(dt), vec, staged, L, grid, lds_bytes, stream);
    default: return launch_m<M_BICUBIC>(luma_only, tensor_el(dt), vec, staged, L, grid, lds_bytes, stream);
    }
}

} // namespace tsvpp
