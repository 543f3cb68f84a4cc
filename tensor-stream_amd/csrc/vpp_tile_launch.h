// vpp_tile_launch.h -- what the launchers of the tile kernels share (vpp_rois.hip, vpp_rois_area.hip, vpp_letterbox.hip, the coordinate paths' vpp_warp.hip,
// vpp_persp.hip, vpp_remap.hip, vpp_mesh.hip, and their *_tensor.hip twins): which (mode, flavour, element) a kernel is instantiated for, the steps from those
// run-time values to template arguments, and the names describe reports.  Each step hands std::integral_constant / std::bool_constant values to a callable, in
// the manner of with_out_kind (vpp_kernels.h); a .hip file nests the steps it needs around its one hipLaunchKernelGGL line -- the eight of the coordinate paths
// nest the same ones, so their launcher is stated here, once for the colour units and once for the tensor units (launch_coord, launch_coord_tensor).  Anything
// not instantiated answers hipErrorNotSupported: a missing kernel is an error, never a fallback.
#pragma once
#include <cstdio>
#include <type_traits>

#include "vpp_kernels.h"
#include "vpp_rois.h"

namespace tsvpp {

inline constexpr const char *kModeNames[M_COUNT] = { "M_NONE", "M_NEAREST", "M_BILINEAR", "M_BICUBIC", "M_AREA_DOWN", "M_AREA_UP" };
inline constexpr const char *kOutNames[O_COUNT] = { "O_U8_PLANAR", "O_U8_MERGED", "O_F32_PLANAR", "O_F32_MERGED", "O_NV12_U8", "O_NV12_F32", "O_Y800_U8", "O_Y800_F32", "O_HSV_F32" };
inline const char *vec_name(bool vec) { return vec ? "vec" : "elem"; }
inline const char *staged_name(bool staged) { return staged ? "staged" : "gather"; }
inline const char *border_name(bool border) { return border ? "border" : "replicate"; } // (vpp_warp.hip: a constant outside the frame, or the edge pixel)

// the modes the ROI and letterbox kernels are instantiated for (the AREA kernel has no mode argument: it chooses per box)
constexpr bool tile_mode(int mode) { return mode == M_NEAREST || mode == M_BILINEAR || mode == M_BICUBIC; }
// the flavours the colour units are instantiated for: RGB / BGR planar and merged, Y800
constexpr bool tile_flavour(int out) { return out == O_U8_PLANAR || out == O_U8_MERGED || out == O_F32_PLANAR || out == O_F32_MERGED || out == O_Y800_U8 || out == O_Y800_F32; }
// ... and the tensor units: three planes or one (`out` is O_F32_PLANAR or O_Y800_F32), the element is the spec's dtype's
constexpr bool tile_tensor(int out, int dtype) { return (out == O_F32_PLANAR || out == O_Y800_F32) && (dtype == TSVPP_F32 || dtype == TSVPP_F16 || dtype == TSVPP_BF16); }
// kernel element (vpp_kernels.h) and the names of a tensor instantiation
inline int tensor_el(int dtype) { return dtype == TSVPP_F32 ? EL_F32 : EL_HALF; }
inline const char *tensor_el_name(int dtype) { return dtype == TSVPP_F32 ? "EL_F32" : "EL_HALF"; }
inline const char *tensor_planes_name(OutKind out) { return out == O_Y800_F32 ? "Y800" : "PLANAR"; }

template <class F> inline hipError_t with_tile_mode(Mode mode, F &&f) {
    switch (mode) {
    case M_NEAREST: return f(std::integral_constant<int, M_NEAREST>());
    case M_BILINEAR: return f(std::integral_constant<int, M_BILINEAR>());
    case M_BICUBIC: return f(std::integral_constant<int, M_BICUBIC>());
    default: return hipErrorNotSupported;
    }
}
template <class F> inline hipError_t with_tile_flavour(OutKind out, F &&f) {
    return with_out_kind(out, [&](auto O) {
        if constexpr (tile_flavour(decltype(O)::value)) return f(O);
        else return hipErrorNotSupported;
    });
}
// f(OUT, EL) of a tensor unit
template <class F> inline hipError_t with_tile_tensor(OutKind out, int dtype, F &&f) {
    if (!tile_tensor(out, dtype)) return hipErrorNotSupported;
    const bool f32 = tensor_el(dtype) == EL_F32;
    if (out == O_Y800_F32) return f32 ? f(std::integral_constant<int, O_Y800_F32>(), std::integral_constant<int, EL_F32>()) : f(std::integral_constant<int, O_Y800_F32>(), std::integral_constant<int, EL_HALF>());
    return f32 ? f(std::integral_constant<int, O_F32_PLANAR>(), std::integral_constant<int, EL_F32>()) : f(std::integral_constant<int, O_F32_PLANAR>(), std::integral_constant<int, EL_HALF>());
}
// f(VEC, STAGED): vector or element-wise stores x footprints staged in LDS or gathered
template <class F> inline hipError_t with_vec_staged(bool vec, bool staged, F &&f) {
    if (vec) return staged ? f(std::true_type(), std::true_type()) : f(std::true_type(), std::false_type());
    return staged ? f(std::false_type(), std::true_type()) : f(std::false_type(), std::false_type());
}
// f(BORDER) of the warp units
template <class F> inline hipError_t with_border(bool border, F &&f) { return border ? f(std::true_type()) : f(std::false_type()); }

// The launcher of a coordinate path's colour unit: launches -- or, with `dry_run`, only names -- the kernel of (out, vec, staged, border).  KERNELS is the path's
// tag (beside its kernel: WarpKernels, vpp_warp_core.h, and so on): `Launch`, its launch block; `kName`, "vpp_warp"; kernel<OUT, VEC, STAGED, BORDER, EL>(), the
// instantiation.  `name` receives what the describe call reports.
template <class KERNELS>
hipError_t launch_coord(OutKind out, bool vec, bool staged, bool border, const typename KERNELS::Launch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                        size_t name_len, bool dry_run) {
    if (!tile_flavour(out)) return hipErrorNotSupported;
    if (name && name_len) snprintf(name, name_len, "%s<%s,%s,%s,%s>", KERNELS::kName, kOutNames[out], vec_name(vec), staged_name(staged), border_name(border));
    if (dry_run) return hipSuccess;
    return with_tile_flavour(out, [&](auto O) {
        return with_vec_staged(vec, staged, [&](auto V, auto S) {
            return with_border(border, [&](auto B) {
                constexpr bool STAGED = decltype(S)::value; // (the gather kernel takes no dynamic LDS)
                hipLaunchKernelGGL((KERNELS::template kernel<decltype(O)::value, decltype(V)::value, STAGED, decltype(B)::value, EL_LIB>()), dim3(grid), dim3(ROI_THREADS), STAGED ? lds_bytes : 0, stream, L);
                return hipGetLastError();
            });
        });
    });
}
// ... and of its tensor unit: `out` is O_F32_PLANAR or O_Y800_F32, the element is L.spec.dtype's
template <class KERNELS>
hipError_t launch_coord_tensor(OutKind out, bool vec, bool staged, bool border, const typename KERNELS::Launch &L, unsigned grid, size_t lds_bytes, hipStream_t stream,
                               char *name, size_t name_len, bool dry_run) {
    const int dt = L.spec.dtype;
    if (!tile_tensor(out, dt)) return hipErrorNotSupported;
    if (name && name_len)
        snprintf(name, name_len, "%s_tensor<%s,%s,%s,%s,%s>", KERNELS::kName, tensor_planes_name(out), tensor_el_name(dt), vec_name(vec), staged_name(staged), border_name(border));
    if (dry_run) return hipSuccess;
    return with_tile_tensor(out, dt, [&](auto O, auto E) {
        return with_vec_staged(vec, staged, [&](auto V, auto S) {
            return with_border(border, [&](auto B) {
                constexpr bool STAGED = decltype(S)::value; // (the gather kernel takes no dynamic LDS)
                hipLaunchKernelGGL((KERNELS::template kernel<decltype(O)::value, decltype(V)::value, STAGED, decltype(B)::value, decltype(E)::value>()), dim3(grid), dim3(ROI_THREADS), STAGED ? lds_bytes : 0, stream, L);
                return hipGetLastError();
            });
        });
    });
}

} // namespace tsvpp
