"""Shared by the tests of tsvpp_convert_rois_p010_bicubic: a numpy int64 restatement of that call's resize (include/tsvpp.h) in the place of p010_util.resize; the
colour stage and the stored forms are p010_util's.  Contains no product code; the reference has no 10-bit path, so this model IS the expected value."""
import numpy as np

import p010_util as M

BICUBIC = 2
ONE = 1 << 20


def axis(N, n):
    """taps and weights of the n outputs of an axis of N samples: (n, 4) arrays of clamped tap indices and of integer weights that sum to 2^20"""
    j = np.arange(n, dtype=np.int64)
    t = (2 * j + 1) * N - n
    p = t // (2 * n)  # (floor: -1 exactly where t < 0)
    F = 32 * (t - 2 * n * p) // n
    G = 64 - F
    w = np.stack([-3 * F * G * G, 5 * F ** 3 - 576 * F * F + ONE, 5 * G ** 3 - 576 * G * G + ONE, -3 * F * F * G], 1)
    return np.clip(p[:, None] - 1 + np.arange(4)[None, :], 0, N - 1), w


def cubic(S, w, h, exact=False):
    """plane S (H, W) of samples -> (h, w): the contract's two passes; `exact`: the same cubic at the same quantised phases in float64, no rounding, no clamp"""
    H, W = S.shape
    S = S.astype(np.float64 if exact else np.int64)
    ix, wx = axis(W, w)
    s = sum(S[:, ix[:, k]] * wx[:, k] for k in range(4))
    hv = s / ONE if exact else (s + ONE // 2) >> 20
    iy, wy = axis(H, h)
    v = sum(hv[iy[:, k]] * wy[:, k, None] for k in range(4))
    return v / ONE if exact else np.clip((v + ONE // 2) >> 20, 0, 1023)


def planes(y, uv, dst):
    """the words of one box -> its Y (h, w), U and V (h / 2, w / 2) before the colour stage"""
    Ys, UVs = M.samples(y), M.samples(uv)
    return cubic(Ys, *dst), cubic(UVs[:, 0::2], dst[0] // 2, dst[1] // 2), cubic(UVs[:, 1::2], dst[0] // 2, dst[1] // 2)


def want(box_planes, dst, flavour):
    """the raw bytes of one box's output in a flavour of p010_cases.FLAVOURS"""
    import p010_cases as C
    return C.stored(M.channels(*planes(*box_planes, dst), C.FLAVOURS[flavour][0]), flavour)
