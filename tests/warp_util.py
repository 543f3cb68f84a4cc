"""Shared by the warp tests (tsvpp_convert_warp): a numpy restatement of the contract of include/tsvpp.h that makes the VIRTUAL NV12 frame of dst_w x dst_h -- the
samples before the colour back end -- and the expected output, which is the existing oracle's conversion without a resize of that virtual frame.  All arithmetic
is np.float32, one rounding per operation; the contract's fused multiply-adds are fma32 below.  Contains no product code.
Its judge is tests/sampler64.py: an independent float64 evaluation of the header's prose, whose bracket this model must stay inside (tests/test_sampler64_cpu.py)."""
from fractions import Fraction

import numpy as np

BILINEAR = 1
Y800, RGB24, BGR24 = 0, 1, 2
PLANAR, MERGED = 0, 1

F32 = np.float32
HALF = F32(0.5)


def fma32(a, b, c):
    """a * b + c with ONE rounding to float32, elementwise.  The product of two float32 is exact in float64 (48 bits); the float64 sum with c rounds, and rounding
    that to float32 would round twice.  TwoSum gives the sum's exact error term; where it is not zero the float64 sum is moved to its odd neighbour on the side of
    the exact value (rounding to odd), after which the final rounding to float32 -- 29 bits shorter -- is the correct one."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)  # exact: p + c == s + e
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0) & even
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def round_fraction_f32(q):
    """a Fraction rounded to the nearest float32, ties to even, in integer arithmetic (normal range and subnormals; no overflow handling: not needed here)"""
    if q == 0:
        return F32(0)
    sign = -1 if q < 0 else 1
    q = abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length() - 24
    while q / Fraction(2) ** e >= 2 ** 24:
        e += 1
    while q / Fraction(2) ** e < 2 ** 23:
        e -= 1
    e = max(e, -149)
    t = q / Fraction(2) ** e
    n = t.numerator // t.denominator
    rem = t - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (n & 1)):
        n += 1
    return F32(sign * float(n) * 2.0 ** e)  # n <= 2^24 and 2^e are exact doubles, their product is a float32 value


def fma_fraction(a, b, c):
    return round_fraction_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def translations(m):
    """(tx, ty, ctx, cty): what the host computes once per warp"""
    m2, m5 = F32(m[2]), F32(m[5])
    return m2 - HALF, m5 - HALF, m2 * HALF - HALF, m5 * HALF - HALF


def coords(m, tx, ty, rows, cols):
    """fx, fy of the grid points (i, j), i in rows, j in cols (index arrays): float32 arrays of shape (len(rows), len(cols))"""
    u = (np.asarray(cols).astype(F32) + HALF)[None, :]
    v = (np.asarray(rows).astype(F32) + HALF)[:, None]
    fx = fma32(u, F32(m[0]), fma32(v, F32(m[1]), tx))
    fy = fma32(u, F32(m[3]), fma32(v, F32(m[4]), ty))
    return fx, fy


def axis(f, limit):
    """bilinear_axis's tail: first tap, second tap, weight (and whether the weight was forced to zero at the low edge, where the second tap is never needed)"""
    pf = np.floor(f)
    w = (f - pf).astype(F32)
    p = pf.astype(np.int64)
    low, high = p < 0, p > limit - 1
    p = np.clip(p, 0, limit - 1)
    w = np.where(low | high, F32(0), w).astype(F32)
    p2 = np.where(p + 1 < limit, p + 1, p)
    return p, p2, w, low


def outside(f, limit):
    return (f < F32(-0.5)) | (f >= F32(limit) - HALF)


def bilerp(A, B, C, D, wx, wy):
    """the library's blend (the fma tree the reference's goldens pin), truncated"""
    A, B, C, D = (t.astype(F32) for t in (A, B, C, D))
    omx, omy = F32(1) - wx, F32(1) - wy
    s = fma32(A * omx, omy, (B * wx) * omy)
    s = fma32(C * wy, omx, s)
    s = fma32(D, wx * wy, s)
    return s.astype(np.int64) & 0xFF


def virtual_frame(y, uv, w, h, m, dst_w, dst_h, border=None):
    """the dst_w x dst_h NV12 frame the warp samples out of the w x h frame (y, uv: planes with any pitch) -> (Y (dst_h, dst_w), UV (dst_h / 2, dst_w)) uint8"""
    tx, ty, ctx, cty = translations(m)
    fx, fy = coords(m, tx, ty, np.arange(dst_h), np.arange(dst_w))
    x, x2, wx, _ = axis(fx, w)
    yy, y2, wy, _ = axis(fy, h)
    Y = bilerp(y[yy, x], y[yy, x2], y[y2, x], y[y2, x2], wx, wy)
    if border is not None:
        Y = np.where(outside(fx, w) | outside(fy, h), border[0], Y)
    cw, ch = w // 2, h // 2
    fx, fy = coords(m, ctx, cty, np.arange(dst_h // 2), np.arange(dst_w // 2))
    x, x2, wx, _ = axis(fx, cw)
    yy, y2, wy, _ = axis(fy, ch)
    UV = np.empty((dst_h // 2, dst_w), np.uint8)
    for comp in (0, 1):
        c = bilerp(uv[yy, 2 * x + comp], uv[yy, 2 * x2 + comp], uv[y2, 2 * x + comp], uv[y2, 2 * x2 + comp], wx, wy)
        if border is not None:
            c = np.where(outside(fx, cw) | outside(fy, ch), border[1 + comp], c)
        UV[:, comp::2] = c
    return Y.astype(np.uint8), UV


def taps(m, w, h, rows, cols, chroma=False):
    """the source taps of output pixels (chroma: pairs) rows x cols, per pixel: (x first, x last, y first, y last) over every tap that can reach the result -- the
    first tap always, the second unless its weight was forced to zero at the low edge (it is multiplied by that zero)"""
    tx, ty, ctx, cty = translations(m)
    fx, fy = coords(m, ctx if chroma else tx, cty if chroma else ty, rows, cols)
    out = []
    for f, limit in ((fx, w // 2 if chroma else w), (fy, h // 2 if chroma else h)):
        p, p2, _, low = axis(f, limit)
        out += [p, np.where(low, p, p2)]
    return tuple(out)


def scale_only(w, h, dst_w, dst_h):
    """the matrix under which the warp is tsvpp_convert(BILINEAR, dst) of the whole frame"""
    return (float(F32(w) / F32(dst_w)), 0.0, 0.0, 0.0, float(F32(h) / F32(dst_h)), 0.0)


def expected(oracle, y, uv, w, h, m, dst, fcc, planes, norm, border=None, virtual=None):
    """the output as raw bytes: the oracle's conversion without a resize of the virtual frame (`virtual`: that frame, if the caller has it already)"""
    Y, UV = virtual_frame(y, uv, w, h, m, dst[0], dst[1], border) if virtual is None else virtual
    ref, _, _ = oracle.convert(Y, UV, fourcc=fcc, planes=planes, normalization=norm)
    return ref.ravel().view(np.uint8)
