"""Shared by the perspective tests (tsvpp_convert_perspective): a numpy restatement of the contract of include/tsvpp.h on top of tests/warp_util.py -- the host
terms, the coordinate with its one reciprocal, the VIRTUAL NV12 frame of dst_w x dst_h and the taps of every sample.  All arithmetic is np.float32, one rounding
per operation (numpy's float32 division and product are IEEE, correctly rounded); the fused multiply-adds are warp_util.fma32.  Contains no product code.
Its judge is tests/sampler64.py: an independent float64 evaluation of the header's prose, whose bracket this model must stay inside (tests/test_sampler64_cpu.py)."""
import numpy as np

import warp_util as W
from warp_util import F32, HALF

TWO = F32(2)
MIN_DENOMINATOR = F32(2.0 ** -64)


def terms(h):
    """(luma, chroma): the nine terms (ax, bx, cx, ay, by, cy, g, hh, k) of each grid, what the host computes once per output"""
    h = [F32(v) for v in h]
    luma = (h[0] - HALF * h[6], h[1] - HALF * h[7], h[2] - HALF * h[8], h[3] - HALF * h[6], h[4] - HALF * h[7], h[5] - HALF * h[8], h[6], h[7], h[8])
    chroma = (h[0] - h[6], h[1] - h[7], h[2] * HALF - h[8] * HALF, h[3] - h[6], h[4] - h[7], h[5] * HALF - h[8] * HALF, TWO * h[6], TWO * h[7], h[8])
    return luma, chroma


def denominators(t, rows, cols):
    u = (np.asarray(cols).astype(F32) + HALF)[None, :]
    v = (np.asarray(rows).astype(F32) + HALF)[:, None]
    return W.fma32(u, t[6], W.fma32(v, t[7], t[8]))


def coords(t, rows, cols):
    """fx, fy of the grid points (i, j), i in rows, j in cols (index arrays), under the terms `t` of their grid: float32 arrays (len(rows), len(cols))"""
    u = (np.asarray(cols).astype(F32) + HALF)[None, :]
    v = (np.asarray(rows).astype(F32) + HALF)[:, None]
    nx = W.fma32(u, t[0], W.fma32(v, t[1], t[2]))
    ny = W.fma32(u, t[3], W.fma32(v, t[4], t[5]))
    nw = W.fma32(u, t[6], W.fma32(v, t[7], t[8]))
    with np.errstate(all="ignore"):
        rw = (F32(1) / nw).astype(F32)
        return (nx * rw).astype(F32), (ny * rw).astype(F32)


def in_domain(h, dst_w, dst_h):
    """the horizon rule: the denominator at the four corner pixels of the luma grid and the four corner pairs of the chroma grid is at least 2^-64"""
    luma, chroma = terms(h)
    a = denominators(luma, [0, dst_h - 1], [0, dst_w - 1])
    b = denominators(chroma, [0, dst_h // 2 - 1], [0, dst_w // 2 - 1])
    return bool((a >= MIN_DENOMINATOR).all() and (b >= MIN_DENOMINATOR).all())


def virtual_frame(y, uv, w, h, hm, dst_w, dst_h, border=None):
    """the dst_w x dst_h NV12 frame the homography `hm` samples out of the w x h frame (y, uv: planes with any pitch) -> (Y (dst_h, dst_w), UV (dst_h / 2, dst_w))"""
    luma, chroma = terms(hm)
    fx, fy = coords(luma, np.arange(dst_h), np.arange(dst_w))
    x, x2, wx, _ = W.axis(fx, w)
    yy, y2, wy, _ = W.axis(fy, h)
    Y = W.bilerp(y[yy, x], y[yy, x2], y[y2, x], y[y2, x2], wx, wy)
    if border is not None:
        Y = np.where(W.outside(fx, w) | W.outside(fy, h), border[0], Y)
    cw, ch = w // 2, h // 2
    fx, fy = coords(chroma, np.arange(dst_h // 2), np.arange(dst_w // 2))
    x, x2, wx, _ = W.axis(fx, cw)
    yy, y2, wy, _ = W.axis(fy, ch)
    UV = np.empty((dst_h // 2, dst_w), np.uint8)
    for comp in (0, 1):
        c = W.bilerp(uv[yy, 2 * x + comp], uv[yy, 2 * x2 + comp], uv[y2, 2 * x + comp], uv[y2, 2 * x2 + comp], wx, wy)
        if border is not None:
            c = np.where(W.outside(fx, cw) | W.outside(fy, ch), border[1 + comp], c)
        UV[:, comp::2] = c
    return Y.astype(np.uint8), UV


def taps(hm, w, h, rows, cols, chroma=False):
    """warp_util.taps under the homography: per pixel (chroma: pair) of rows x cols, (x first, x last, y first, y last) over every tap that can reach the result"""
    t = terms(hm)[1 if chroma else 0]
    fx, fy = coords(t, rows, cols)
    out = []
    for f, limit in ((fx, w // 2 if chroma else w), (fy, h // 2 if chroma else h)):
        p, p2, _, low = W.axis(f, limit)
        out += [p, np.where(low, p, p2)]
    return tuple(out)


def from_quad(quad, dst_w, dst_h):
    """Heckbert's closed form in Python doubles, each entry rounded once to float32 (None where den == 0): the formula of include/tsvpp.h"""
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = [(float(a), float(b)) for a, b in quad]
    sx, sy = x0 - x1 + x2 - x3, y0 - y1 + y2 - y3
    g = hh = 0.0
    if sx != 0.0 or sy != 0.0:
        dx1, dx2, dy1, dy2 = x1 - x2, x3 - x2, y1 - y2, y3 - y2
        den = dx1 * dy2 - dx2 * dy1
        if den == 0.0:
            return None
        g = (sx * dy2 - dx2 * sy) / den
        hh = (dx1 * sy - sx * dy1) / den
    m = ((x1 - x0 + g * x1) / dst_w, (x3 - x0 + hh * x3) / dst_h, x0, (y1 - y0 + g * y1) / dst_w, (y3 - y0 + hh * y3) / dst_h, y0, g / dst_w, hh / dst_h, 1.0)
    return tuple(float(F32(v + 0.0)) for v in m)


def affine(m):
    """the homography of the 2 x 3 matrix m"""
    return tuple(m) + (0.0, 0.0, 1.0)


def expected(oracle, y, uv, w, h, hm, dst, fcc, planes, norm, border=None, virtual=None):
    """the output as raw bytes: the oracle's conversion without a resize of the virtual frame (warp_util.expected on this module's virtual frame)"""
    V = virtual_frame(y, uv, w, h, hm, dst[0], dst[1], border) if virtual is None else virtual
    return W.expected(oracle, None, None, 0, 0, None, dst, fcc, planes, norm, border, virtual=V)
