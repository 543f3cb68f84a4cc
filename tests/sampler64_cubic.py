"""The judge of tests/warp_bicubic_util.py (and, through it or directly, of the kernels of tsvpp_convert_warp_bicubic / tsvpp_convert_perspective_bicubic): a float64
evaluation of what include/tsvpp.h promises in words for the BICUBIC warps, with a derived bracket per sample.  It shares no code and no operation order with the
model: the positions and the bound e of the fp32 coordinate are tests/sampler64.py's (the judge of the BILINEAR calls -- the coordinate is theirs, bit for bit);
the cubic is Keys' kernel as a function of the DISTANCE to a tap, not the model's four polynomials in w.  Contains no product code; numpy only.

The contract, per axis, on the index coordinate f = position - 1/2 (sampler64.py says what a position is):
  cell     p = floor(f), w = f - p; below the plane p = 0, w = 0; above its last sample p = limit - 1, w = 0.
  taps     p - 1, p, p + 1, p + 2 at distances 1 + w, w, 1 - w, 2 - w -- except at the edges (the reference's rule): where p + 1 OR p + 2 would leave the plane
           BOTH upper taps are p, and at p = 0 the lower tap is p.  The weights stay those of the distances.
  weights  Keys, a = -3/4: k(d) = (a + 2) d^3 - (a + 3) d^2 + 1 for d <= 1, a d^3 - 5 a d^2 + 8 a d - 4 a for 1 < d < 2.
  sum      four horizontal sums of taps times weights, each ROUNDED half away from zero and clamped to 0..255; then the vertical sum of those four integers with
           the row weights, rounded and clamped the same way.
  border   a sample is the border component iff its position is outside [0, limit) on either axis, whole, never mixed in.

The bracket.  The fp32 coordinate f' lies within e of f (sampler64.py derives e per path; e < 1/2 is asserted), so floor(f') is floor(f - e) or floor(f + e): at
most two cells per axis, four per sample; the bracket is the hull over them.  Within one cell w' lies in an interval [w0, w1] (the part of [f - e, f + e] inside
the cell; a single point 0 where the contract forces w = 0).  Interval arithmetic from there:
  weights   each weight as a function of w is Lipschitz: with c0 = k(1 + w), c1 = k(w), c2 = k(1 - w), c3 = k(2 - w),
                c0' = a (3 w^2 - 4 w + 1)           in [a, -a / 3] on [0, 1]:  |c0'| <= 3/4
                c1' = 3 (a + 2) w^2 - 2 (a + 3) w   least at w = 3/5, -27/20:  |c1'| <= 27/20
            and c2(w) = c1(1 - w), c3(w) = c0(1 - w): LIP = (3/4, 27/20, 27/20, 3/4).  So c_k(w') lies within LIP_k (w1 - w0) / 2 of c_k at the midpoint.
  rows      taps are non-negative: a horizontal sum lies within (w1 - w0) / 2 * sum LIP_k tap_k of the sum at the midpoint, plus TINY = 1e-9 for this file's own
            float64 round-off (a sum below 1024 of five-term products: 1e-12) and the contract's (the library's fp64 sum in its own order: the same size).  Rounding
            and clamping are monotone: the row's integer lies in [R(s - r), R(s + r)].
  column    the product of a weight interval [c0, c1] and an integer interval [b0, b1], b0 >= 0, lies in [min(c0 b0, c0 b1), max(c1 b0, c1 b1)]; the sum of the
            four, widened by TINY, is rounded and clamped the same way.
Where e = 0 would hold the bracket is a single value unless a sum lies within TINY of a tie; with e > 0 a sample is two-valued where a row sum or the column sum
passes a half-integer inside its interval, or where f lies within e of an integer and the two cells disagree.  No sample is ever left out.
Border mode: a sample outside by more than e is the border value, one inside by more than e is its bracket, one within e of a frame edge may be either (the hull).
Output: sampler64.output_bracket / tensor_bracket on this file's virtual bracket (the colour back end is monotone in each of Y, U, V)."""
import numpy as np

import sampler64 as S

A = -0.75
LIP = (0.75, 1.35, 1.35, 0.75)
TINY = 1e-9

FRAMES = [(322, 182, 384), (32, 18, 48), (4, 2, 4)]  # (width, height, pitch); 4 x 2: every upper tap collapses, the chroma plane is 2 x 1 pairs
DSTS = [(70, 66), (30, 34), (112, 112)]
BORDERS = [None, (3, 250, 7)]


def keys(d):
    """Keys' kernel at distance d in [0, 2]"""
    d = np.asarray(d, np.float64)
    near = (A + 2) * d ** 3 - (A + 3) * d ** 2 + 1
    far = A * d ** 3 - 5 * A * d ** 2 + 8 * A * d - 4 * A
    return np.where(d <= 1, near, far)


def _round_clamp(s):
    """half away from zero, then 0..255: for s < 0 every rounding clamps to 0, so floor(s + 1/2) serves both signs"""
    return np.clip(np.floor(s + 0.5), 0, 255)


def _cell(f, e, q, limit):
    """axis state of the raw cell q (int array) for coordinates within e of f: (p, taps (4), weight midpoints (4), weight radii (4))"""
    w0 = np.clip(np.maximum(f - e, q) - q, 0.0, 1.0)
    w1 = np.clip(np.minimum(f + e, q + 1.0) - q, 0.0, 1.0)
    forced = (q < 0) | (q > limit - 1)
    w0, w1 = np.where(forced, 0.0, w0), np.where(forced, 0.0, w1)
    p = np.clip(q, 0, limit - 1)
    collapse = (p + 1 > limit - 1) | (p + 2 > limit - 1)
    up = np.where(collapse, 0, 1)
    taps = (np.where(p == 0, p, p - 1), p, p + up, p + 2 * up)
    mid, half = (w0 + w1) / 2, (w1 - w0) / 2
    weights = (keys(1 + mid), keys(mid), keys(1 - mid), keys(2 - mid))
    return taps, weights, tuple(L * half for L in LIP)


def _combo(P, fx, ex, qx, fy, ey, qy):
    """(lo, hi) of every sample for the cell pair (qx, qy)"""
    h, w = P.shape
    xt, xw, xr = _cell(fx, ex, qx, w)
    yt, yw, yr = _cell(fy, ey, qy, h)
    lo = hi = 0.0
    for r in range(4):
        row = [P[yt[r], xt[k]] for k in range(4)]
        s = sum(xw[k] * row[k] for k in range(4))
        rad = sum(xr[k] * row[k] for k in range(4)) + TINY
        b0, b1 = _round_clamp(s - rad), _round_clamp(s + rad)
        c0, c1 = yw[r] - yr[r], yw[r] + yr[r]
        lo = lo + np.minimum(c0 * b0, c0 * b1)
        hi = hi + np.maximum(c1 * b0, c1 * b1)
    return _round_clamp(lo - TINY), _round_clamp(hi + TINY)


def bracket(plane, grid, border=None):
    """(lo, hi): the integer bracket of every sample of `grid` (a sampler64.Grid) on `plane`; border: the component samples outside the frame take"""
    P = np.asarray(plane, np.float64)
    h, w = P.shape
    assert grid.ex.max() < 0.5 and grid.ey.max() < 0.5
    fx, fy = grid.X - 0.5, grid.Y - 0.5
    # (the library clamps f into [-1, limit] before the conversion to an integer, which changes no result: do the same so that the cells are small integers)
    cx0, cx1 = np.floor(np.clip(fx - grid.ex, -1.0, w)).astype(np.int64), np.floor(np.clip(fx + grid.ex, -1.0, w)).astype(np.int64)
    cy0, cy1 = np.floor(np.clip(fy - grid.ey, -1.0, h)).astype(np.int64), np.floor(np.clip(fy + grid.ey, -1.0, h)).astype(np.int64)
    lo = hi = None
    for qx in (cx0, cx1):
        for qy in (cy0, cy1):
            a, b = _combo(P, fx, grid.ex, qx, fy, grid.ey, qy)
            lo = a if lo is None else np.minimum(lo, a)
            hi = b if hi is None else np.maximum(hi, b)
    lo, hi = lo.astype(np.int64), hi.astype(np.int64)
    if border is not None:
        X, Y, ex, ey = grid.X, grid.Y, grid.ex, grid.ey
        outside = (X < -ex) | (X >= w + ex) | (Y < -ey) | (Y >= h + ey)
        inside = (X >= ex) & (X < w - ex) & (Y >= ey) & (Y < h - ey)
        lo = np.where(outside, border, np.where(inside, lo, np.minimum(lo, border)))
        hi = np.where(outside, border, np.where(inside, hi, np.maximum(hi, border)))
    return lo, hi


def positions(c, dst_w, dst_h):
    """(luma Grid, chroma Grid) of a 2 x 3 matrix (six numbers) or a homography (nine): sampler64.py's, with its bounds e"""
    return S.affine_positions(c, dst_w, dst_h) if len(c) == 6 else S.perspective_positions(c, dst_w, dst_h)


def virtual_bracket(y, uv, w, h, grids, border=None):
    """the sample brackets of the luma and chroma Grids on the w x h frame (y, uv: planes with any pitch), as a sampler64.Virtual: Ylo, Yhi, UVlo, UVhi uint8;
    two / size = the two-valued samples and all samples of Y, U, V"""
    luma, chroma = grids
    out = S.Virtual()
    out.two, out.size = [], []
    planes = (y[:h, :w], uv[:h // 2, 0:w:2], uv[:h // 2, 1:w:2])
    los, his = [], []
    for k, plane in enumerate(planes):
        lo, hi = bracket(plane, luma if k == 0 else chroma, None if border is None else border[k])
        los.append(lo.astype(np.uint8))
        his.append(hi.astype(np.uint8))
        out.two.append(int((lo != hi).sum()))
        out.size.append(lo.size)
    out.Ylo, out.Yhi = los[0], his[0]
    out.UVlo, out.UVhi = np.empty((los[1].shape[0], 2 * los[1].shape[1]), np.uint8), np.empty((los[1].shape[0], 2 * los[1].shape[1]), np.uint8)
    out.UVlo[:, 0::2], out.UVlo[:, 1::2], out.UVhi[:, 0::2], out.UVhi[:, 1::2] = los[1], los[2], his[1], his[2]
    return out


def cases():
    """the committed case set: (frame index, (w, h, pitch), dst, name, coefficients) over FRAMES x DSTS x sampler64's affine and perspective items"""
    for k, (w, h, pitch) in enumerate(FRAMES):
        for dst in DSTS:
            for kind in (S.AFFINE, S.PERSPECTIVE):
                for name, make in kind.items():
                    yield k, (w, h, pitch), dst, name, make(w, h, *dst)
