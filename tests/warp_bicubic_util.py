"""Shared by the BICUBIC warp tests (tsvpp_convert_warp_bicubic, tsvpp_convert_perspective_bicubic): a numpy restatement of the contract of include/tsvpp.h that
makes the VIRTUAL NV12 frame of dst_w x dst_h -- the samples before the colour back end -- and the expected output, the existing oracle's conversion without a
resize of that frame.  The coordinates are tests/warp_util.py's and tests/persp_util.py's (np.float32, one rounding per operation: the BILINEAR calls'
coordinates, bit for bit); the cubic is np.float64 in the contract's order.  Contains no product code.
Its judge is tests/sampler64_cubic.py: an independent float64 evaluation of the header's prose whose bracket this model must stay inside
(tests/test_warp_bicubic_cpu.py).  The pieces a mutation test replaces are module-level names: A, coeffs, tap_indices, row_round."""
import numpy as np

import persp_util as P
import warp_util as W
from warp_util import F32

BICUBIC = 2
A = -0.75  # Keys


def axis(f, limit):
    """centre tap and weight of one axis: p = floor(f), w = f - p (exact in float32); forced to (0, 0) below the plane and to (limit - 1, 0) above it"""
    pf = np.floor(f)
    w = (f - pf).astype(F32)
    p = pf.astype(np.int64)
    off = (p < 0) | (p > limit - 1)
    return np.clip(p, 0, limit - 1), np.where(off, F32(0), w).astype(np.float64)


def tap_indices(p, limit):
    """the four taps of centre p under the reference's edge rule: p - lo, p, p + hi, p + 2 hi -- BOTH upper taps collapse onto p where either would leave the
    plane, the lower one at the low edge"""
    hi = np.where((p + 1 >= limit) | (p + 2 >= limit), 0, 1)
    lo = np.where(p - 1 < 0, 0, 1)
    return p - lo, p, p + hi, p + 2 * hi


def coeffs(w):
    """the four weights from w as float64: the exact square, the correctly rounded cube, each polynomial in the library's order"""
    a = A
    w2 = w * w
    w3 = w2 * w
    return ((a * w - (2 * a) * w2) + a * w3, (1 - (a + 3) * w2) + (a + 2) * w3, ((-a) * w + (2 * a + 3) * w2) - (a + 2) * w3, a * w2 - a * w3)


def round_half_away(s):
    t = np.trunc(s)
    return t + np.where(np.abs(s - t) >= 0.5, np.sign(s), 0.0)


def row_round(s):
    """what becomes of a horizontal sum before the vertical one: rounded half away from zero, clamped to 0..255"""
    return np.clip(round_half_away(s), 0, 255)


def cubic4(c, p0, p1, p2, p3):
    return ((c[0] * p0 + c[1] * p1) + c[2] * p2) + c[3] * p3


def sample(plane, fx, fy, w, h, step=1, comp=0):
    """the plane's samples at float32 coordinates fx, fy under limits w, h; step / comp: 2 / 0 or 1 for U and V of the interleaved chroma plane"""
    x, wx = axis(fx, w)
    y, wy = axis(fy, h)
    cx, cy = coeffs(wx), coeffs(wy)
    cols = [step * c + comp for c in tap_indices(x, w)]
    b = []
    for r in tap_indices(y, h):
        b.append(row_round(cubic4(cx, *[plane[r, c].astype(np.float64) for c in cols])))
    return np.clip(round_half_away(cubic4(cy, *b)), 0, 255).astype(np.int64)


def grid_coords(coeffs_, dst_w, dst_h):
    """(luma fx, fy, chroma fx, fy) of a 2 x 3 matrix (six numbers) or a homography (nine)"""
    if len(coeffs_) == 6:
        tx, ty, ctx, cty = W.translations(coeffs_)
        return W.coords(coeffs_, tx, ty, np.arange(dst_h), np.arange(dst_w)) + W.coords(coeffs_, ctx, cty, np.arange(dst_h // 2), np.arange(dst_w // 2))
    luma, chroma = P.terms(coeffs_)
    return P.coords(luma, np.arange(dst_h), np.arange(dst_w)) + P.coords(chroma, np.arange(dst_h // 2), np.arange(dst_w // 2))


def virtual_frame(y, uv, w, h, c, dst_w, dst_h, border=None):
    """the dst_w x dst_h NV12 frame the matrix or homography `c` samples BICUBIC out of the w x h frame (y, uv: planes with any pitch)"""
    fx, fy, cfx, cfy = grid_coords(c, dst_w, dst_h)
    Y = sample(y, fx, fy, w, h)
    if border is not None:
        Y = np.where(W.outside(fx, w) | W.outside(fy, h), border[0], Y)
    cw, ch = w // 2, h // 2
    UV = np.empty((dst_h // 2, dst_w), np.uint8)
    for comp in (0, 1):
        v = sample(uv, cfx, cfy, cw, ch, step=2, comp=comp)
        if border is not None:
            v = np.where(W.outside(cfx, cw) | W.outside(cfy, ch), border[1 + comp], v)
        UV[:, comp::2] = v
    return Y.astype(np.uint8), UV


def taps(c, w, h, dst_w, dst_h):
    """per luma pixel and per chroma pair the hull of its taps: ((x first, x last, y first, y last) luma, the same in pairs for chroma)"""
    fx, fy, cfx, cfy = grid_coords(c, dst_w, dst_h)
    out = []
    for gx, gy, lw, lh in ((fx, fy, w, h), (cfx, cfy, w // 2, h // 2)):
        hull = []
        for f, limit in ((gx, lw), (gy, lh)):
            p, _ = axis(f, limit)
            t = tap_indices(p, limit)
            hull += [t[0], t[3]]
        out.append(tuple(hull))
    return tuple(out)


def expected(oracle, y, uv, w, h, c, dst, fcc, planes, norm, border=None, virtual=None):
    """the output as raw bytes: the oracle's conversion without a resize of the virtual frame"""
    V = virtual_frame(y, uv, w, h, c, dst[0], dst[1], border) if virtual is None else virtual
    return W.expected(oracle, None, None, 0, 0, None, dst, fcc, planes, norm, border, virtual=V)
