"""The judge of tests/warp_util.py, tests/persp_util.py and tests/remap_util.py (and, through them or directly, of the kernels): a plain float64 evaluation of the
REAL-VALUED operation that include/tsvpp.h promises in words for tsvpp_convert_warp / _perspective / _remap, with a derived bound on how far a correct fp32
evaluation of the contract may sit from it.  It shares no code and no operation order with the three models: no float32 arithmetic, no fused multiply-add
emulation, nothing of the header's "Arithmetic" paragraphs but their operation COUNT.  Contains no product code; numpy only.

Positions (continuous, pixel k covering [k, k + 1); matrix and map entries are the float32 values the call receives, widened to float64)
  affine       luma pixel (i, j): X = m0 (j + 1/2) + m1 (i + 1/2) + m2, Y likewise.  Chroma pair (ci, cj): half the luma position of the pair's centre
               (u, v) = (2 cj + 1, 2 ci + 1), on the chroma grid of w / 2 x h / 2.
  perspective  the same with X = (h0 u + h1 v + h2) / (h6 u + h7 v + h8).
  remap        luma: the map entry + 1/2 (the map is index-based).  Chroma: the mean of the block's four entries + 1/2, halved.
Sampling   bilinear at the index coordinate f = position - 1/2 clamped into [0, limit - 1]: (A (1 - wx) + B wx)(1 - wy) + (C (1 - wx) + D wx) wy.  U and V
           are the de-interleaved half-size planes.
Border     a sample is the border component iff its position is outside [0, limit) on either axis; luma and chroma decide independently.

The bound.  eps = 2^-24: one fp32 rounding to nearest moves a result r by at most eps |r| (half an ulp), and by NOTHING where the exact result is representable:
a multiple of 2^-q below 2^(24 - q) in magnitude is (rule R).  e is the bound of the fp32 index coordinate against the float64 one, per axis:
  affine       t = m2 - 1/2 (host, one rounding; chroma t = m2 / 2 - 1/2), inner = fma(v, m1, t), f = fma(u, m0, inner): two fused multiply-adds after the
               host's one.  Each error passes on with factor 1: e = eps (|t| + |inner| + |f|).
  perspective  six numerator terms a = h_k - h_j / 2 (chroma: h_k - h_j, h_k / 2 - h_j / 2) rounded once by the host, eps |a| each; the denominator's terms
               are exact.  n = fma(u, a, fma(v, b, c)): E_n = eps (u |a| + v |b| + |c| + |v b + c| + |n|), the sum of the terms' sizes, which is what survives
               a cancellation in n.  nw likewise: E_w = eps (|v hh + k| + |nw|).  Then one reciprocal and one product, each (1 + eps):
               |n' / nw' - n / nw| <= q = (E_n + |f| E_w) / (nw - E_w), and e = q + (|f| + q)(2 eps + eps^2).  (E_n / nw is the cancellation term.)
  remap        luma: none, the entry is the coordinate.  Chroma: s = (x00 + x01) + (x10 + x11), three additions, then cf = fma(s, 1/8, -1/4):
               e = eps (|x00 + x01| + |x10 + x11| + |s|) / 8 + eps |cf|; and e = 0 where the four entries are multiples of 2^-10 below 2^11 (rule R: every sum
               is a multiple of 2^-10 below 2^13, cf a multiple of 2^-13 below 2^10).
Every e is multiplied by 1 + 2^-20, which covers the second-order terms (a rounding is bounded by the size of the ROUNDED result) and this file's own float64
round-off, eleven orders below.  A helper's own rounding (a matrix entry rounded after the conversion from OpenCV's form, a map made from a grid in fp32) is
added to e by the test that checks that helper, from the helper's operation count.
  blend        the sampled value is continuous and, inside one source cell, changes along x by at most max(|B - A|, |D - C|) per pixel (along y:
               max(|C - A|, |D - B|)).  The fp32 coordinate lies within e of f, so the clamped one lies in [clamp(f - e), clamp(f + e)], which touches at most
               two cells per axis (e < 1/2 is asserted): the value moves by at most Lx ex' + Ly ey', Lx / Ly the largest such difference over the up to four
               cells touched, ex' = max |clamp(f +- e) - clamp(f)| (zero where the clamp absorbs the error).  The library's blend then commits ten
               roundings -- 1 - wx, 1 - wy, A (1 - wx), B wx, (B wx)(1 - wy), C wy, wx wy and three fused multiply-adds -- each of a value below 256, so at most
               2^-17 each (1 - wx errs by 2^-25 and multiplies taps that sum to at most 255); an eleventh 2^-17 covers every product of two errors:
               BLEND = 11 * 2^-17.  BLEND = 0 where both weights are KNOWN multiples of 2^-8 -- e = 0 on that axis and 256 w an integer, or the coordinate
               outside [0, limit) by more than e, where the contract forces w = 0 -- since then every product and partial sum is a multiple of 2^-16 below 256
               (rule R).
  delta = Lx ex' + Ly ey' + BLEND, derived, never fitted.
Bracket    per sample {floor(v - delta) ... floor(v + delta)}: the library truncates the blend.  In border mode a sample outside by more than e is the border
           value, one inside by more than e is its blend's bracket, one within e of a frame edge may be either (the hull of both).
Output     the colour back end is monotone in each of Y, U, V per channel through every rounding and the truncation (tests/test_sampler64_cpu.py checks that
           over all 2^24 triples), so the oracle's conversion WITHOUT a resize of the four virtual frames (Ylo, Ulo, Vlo), (Yhi, Uhi, Vhi), (Ylo, Uhi, Vhi),
           (Yhi, Ulo, Vlo) holds, per element, the least and the largest value any frame inside the sample brackets can give: lo / hi are their element-wise
           minimum / maximum.  Where the brackets are single-valued lo == hi and the comparison is exact equality.  No sample is ever left out."""
import numpy as np

Y800, RGB24, BGR24 = 0, 1, 2
PLANAR, MERGED = 0, 1

EPS = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
BLEND = 11 * 2.0 ** -17

# ---- the case set --------------------------------------------------------------------------------------------------------------------------------------------
FRAMES = [(322, 182, 384), (128, 72, 192), (32, 18, 48)]  # (width, height, pitch)
DSTS = [(70, 66), (30, 34), (112, 112)]  # the shifted tile column; narrower than a tile; 4 x 4 tiles
BORDERS = [None, (3, 250, 7)]


def f32(values):
    """the values as the call receives them: rounded once to float32, as Python floats"""
    return tuple(float(np.float32(v)) for v in values)


def rotated_box(cx, cy, box_w, box_h, angle, dst_w, dst_h):
    """the 2 x 3 matrix under which the output spans the box of box_w x box_h centred at (cx, cy) and rotated by `angle` from x towards y: the output's centre
    lands on (cx, cy), one output column is box_w / dst_w along the rotated x axis, one row box_h / dst_h along the rotated y axis"""
    c, s = np.cos(angle), np.sin(angle)
    ax, ay, bx, by = box_w / dst_w * c, box_w / dst_w * s, -box_h / dst_h * s, box_h / dst_h * c
    return (ax, bx, cx - ax * dst_w / 2 - bx * dst_h / 2, ay, by, cy - ay * dst_w / 2 - by * dst_h / 2)


def quad_homography(quad, dst_w, dst_h):
    """the homography that takes the output's corners (0, 0), (dst_w, 0), (dst_w, dst_h), (0, dst_h) to the four points of `quad`, h8 = 1: the eight linear
    equations, solved in float64"""
    src = [(0.0, 0.0), (float(dst_w), 0.0), (float(dst_w), float(dst_h)), (0.0, float(dst_h))]
    a, b = [], []
    for (u, v), (x, y) in zip(src, quad):
        a += [[u, v, 1, 0, 0, 0, -u * x, -v * x], [0, 0, 0, u, v, 1, -u * y, -v * y]]
        b += [x, y]
    return tuple(np.linalg.solve(np.array(a, np.float64), np.array(b, np.float64))) + (1.0,)


def _rel(quad, w, h):
    return [(x * w, y * h) for x, y in quad]


MILD = [(0.10, 0.15), (0.90, 0.05), (0.95, 0.90), (0.05, 0.80)]
TRAPEZOID = [(0.40, 0.10), (0.60, 0.10), (0.90, 0.90), (0.10, 0.90)]  # the top side a quarter of the bottom
HALF_OUT = [(-0.40, 0.10), (0.50, 0.00), (0.60, 0.95), (-0.50, 0.80)]

# name -> (w, h, dst_w, dst_h) -> the float32 matrix.  (down4.6 carries a fractional translation: without one its weights are multiples of 0.2, moved by the
# rounding of 4.6 to float32, and a fifth of all blends of two taps is an integer -+ 1e-6 -- samples that truly are two-valued)
AFFINE = {
    "rot30": lambda w, h, dw, dh: f32(rotated_box(w / 2, h / 2, 1.7 * dw, 1.7 * dh, np.radians(30), dw, dh)),
    "up_shear": lambda w, h, dw, dh: f32((0.37, 0.1, 0.3 * w, 0.05, 0.37, 0.3 * h)),
    "down4.6": lambda w, h, dw, dh: f32((4.6, 0, w / 2 - 2.3 * dw + 0.137, 0, 4.6, h / 2 - 2.3 * dh + 0.291)),
    "half_out": lambda w, h, dw, dh: f32(rotated_box(0, h / 2, w, h, 0.2, dw, dh)),
    "fraction": lambda w, h, dw, dh: f32((1, 0, 0.37, 0, 1, 0.61)),
}
PERSPECTIVE = {
    "mild": lambda w, h, dw, dh: f32(quad_homography(_rel(MILD, w, h), dw, dh)),
    "trapezoid": lambda w, h, dw, dh: f32(quad_homography(_rel(TRAPEZOID, w, h), dw, dh)),
    "half_out": lambda w, h, dw, dh: f32(quad_homography(_rel(HALF_OUT, w, h), dw, dh)),
    "affine_part": lambda w, h, dw, dh: f32(quad_homography(_rel(MILD, w, h), dw, dh)[:6] + (0.0, 0.0, 1.0)),
}


def leaving_map(w, h, dw, dh):
    """a smooth map that leaves the frame on the left and at the bottom"""
    j, i = np.meshgrid(np.arange(dw, dtype=np.float64), np.arange(dh, dtype=np.float64))
    x = -0.15 * w + 1.05 * w * (j + 0.5) / dw + 1.5 * np.sin(i / 9.0)
    y = 0.10 * h + 1.05 * h * (i + 0.5) / dh + 1.5 * np.cos(j / 7.0)
    return np.ascontiguousarray(np.stack((x, y), axis=-1).astype(np.float32))


# name -> (gen, w, h, dst_w, dst_h) -> the float32 map (dst_h, dst_w, 2); gen: the module with the tests' map generators (tests/remap_util.py -- its
# generators make INPUTS; nothing of its model is used here)
REMAP = {
    "barrel": lambda gen, w, h, dw, dh: gen.barrel(dw, dh, w, h),
    "affine": lambda gen, w, h, dw, dh: gen.affine(dw, dh, w, h),
    "fraction": lambda gen, w, h, dw, dh: gen.translation(dw, dh, 2 * max((w - dw) // 4, 0) + 0.37, 2 * max((h - dh) // 4, 0) + 0.61),
    "exact2": lambda gen, w, h, dw, dh: gen.exact_ratio(dw, dh, 2),
    "leaving": lambda gen, w, h, dw, dh: leaving_map(w, h, dw, dh),
}


def smooth_nv12(w, h, seed, pitch=None):
    """a band-limited NV12 frame: a random field blurred three times by a box of 5 (luma) / 3 (chroma) samples per axis, stretched to 8 .. 247"""
    pitch = w if pitch is None else pitch
    rng = np.random.default_rng(seed)

    def field(rows, cols, k):
        f = rng.random((rows + 6 * k, cols + 6 * k))
        box = np.ones(2 * k + 1) / (2 * k + 1)
        for _ in range(3):
            f = np.apply_along_axis(np.convolve, 0, f, box, "same")
            f = np.apply_along_axis(np.convolve, 1, f, box, "same")
        f = f[3 * k:3 * k + rows, 3 * k:3 * k + cols]
        return np.rint(8 + 239 * (f - f.min()) / (f.max() - f.min())).astype(np.uint8)

    y = np.zeros((h, pitch), np.uint8)
    uv = np.zeros((h // 2, pitch), np.uint8)
    y[:, :w] = field(h, w, 2)
    uv[:, 0:w:2] = field(h // 2, w // 2, 1)
    uv[:, 1:w:2] = field(h // 2, w // 2, 1)
    return y, uv


# ---- positions -----------------------------------------------------------------------------------------------------------------------------------------------
class Grid:
    """the continuous positions X, Y of one sample grid and the bounds ex, ey of the fp32 index coordinate against X - 1/2, Y - 1/2"""

    def __init__(self, X, Y, ex, ey):
        self.X, self.Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
        self.ex, self.ey = np.broadcast_to(np.asarray(ex, np.float64), self.X.shape), np.broadcast_to(np.asarray(ey, np.float64), self.X.shape)

    def widened(self, dx, dy):
        return Grid(self.X, self.Y, self.ex + dx, self.ey + dy)


def _centres(n_rows, n_cols):
    u = (np.arange(n_cols, dtype=np.float64) + 0.5)[None, :]
    v = (np.arange(n_rows, dtype=np.float64) + 0.5)[:, None]
    return u, v


def affine_positions(m, dst_w, dst_h):
    """(luma Grid (dst_h, dst_w), chroma Grid (dst_h / 2, dst_w / 2)) of the matrix m"""
    m = [float(np.float32(v)) for v in m]
    u, v = _centres(dst_h, dst_w)
    luma = []
    for a, b, c in (m[0:3], m[3:6]):
        pos = a * u + b * v + c
        luma += [pos, EPS * SLACK * (abs(c - 0.5) + np.abs(b * v + (c - 0.5)) + np.abs(pos - 0.5))]
    u, v = _centres(dst_h // 2, dst_w // 2)
    chroma = []
    for a, b, c in (m[0:3], m[3:6]):
        pos = (a * (2 * u) + b * (2 * v) + c) / 2  # the pair's centre, in luma pixels 2 cj + 1 = 2 u, halved
        chroma += [pos, EPS * SLACK * (abs(c / 2 - 0.5) + np.abs(b * v + (c / 2 - 0.5)) + np.abs(pos - 0.5))]
    return Grid(luma[0], luma[2], luma[1], luma[3]), Grid(chroma[0], chroma[2], chroma[1], chroma[3])


def perspective_positions(hm, dst_w, dst_h, entry_ulps=0):
    """(luma Grid, chroma Grid) of the homography hm.  entry_ulps = 1: every entry additionally carries one rounding of its own (a helper's, see the docstring)"""
    hm = [float(np.float32(v)) for v in hm]
    out = []
    for chroma in (False, True):
        u, v = _centres(dst_h // 2, dst_w // 2) if chroma else _centres(dst_h, dst_w)
        U, V = (2 * u, 2 * v) if chroma else (u, v)  # the luma position of the sample
        nw = hm[6] * U + hm[7] * V + hm[8]
        assert (nw > 0).all(), "the horizon crosses the output"
        g, hh, k = (2 * hm[6], 2 * hm[7], hm[8]) if chroma else (hm[6], hm[7], hm[8])
        E_w = EPS * (np.abs(hh * v + k) + np.abs(nw)) + entry_ulps * EPS * (u * abs(g) + v * abs(hh) + abs(k))
        grid = []
        for r in (0, 3):
            pos = (hm[r] * U + hm[r + 1] * V + hm[r + 2]) / nw
            pos = pos / 2 if chroma else pos
            f = pos - 0.5
            # the folded terms: luma h_k - h_j / 2; chroma h_k - h_j for u and v, h_k / 2 - h_j / 2 for the constant
            sc, sk = (1.0, 0.5) if chroma else (0.5, 1.0)
            a, b, c = hm[r] - sc * hm[6], hm[r + 1] - sc * hm[7], sk * hm[r + 2] - 0.5 * hm[8]
            n = a * u + b * v + c
            E_n = EPS * (u * abs(a) + v * abs(b) + abs(c) + np.abs(b * v + c) + np.abs(n))
            E_n = E_n + entry_ulps * EPS * (u * (abs(hm[r]) + sc * abs(hm[6])) + v * (abs(hm[r + 1]) + sc * abs(hm[7])) + sk * abs(hm[r + 2]) + 0.5 * abs(hm[8]))
            assert (nw > 2 * E_w).all()
            q = (E_n + np.abs(f) * E_w) / (nw - E_w)
            grid += [pos, SLACK * (q + (np.abs(f) + q) * (2 * EPS + EPS * EPS))]
        out.append(Grid(grid[0], grid[2], grid[1], grid[3]))
    return out[0], out[1]


def remap_positions(xy):
    """(luma Grid, chroma Grid) of the map xy (dst_h, dst_w, 2) float32, finite entries"""
    xy = np.asarray(xy)
    assert xy.dtype == np.float32 and np.isfinite(xy).all()
    m = xy.astype(np.float64)
    luma = Grid(m[..., 0] + 0.5, m[..., 1] + 0.5, 0.0, 0.0)
    chroma = []
    for c in (m[..., 0], m[..., 1]):
        x00, x01, x10, x11 = c[0::2, 0::2], c[0::2, 1::2], c[1::2, 0::2], c[1::2, 1::2]
        s = (x00 + x01) + (x10 + x11)  # exact in float64 for every finite float32 whose exponents are not 29 binades apart; else within the SLACK
        cf = s / 8 - 0.25
        e = EPS * SLACK * ((np.abs(x00 + x01) + np.abs(x10 + x11) + np.abs(s)) / 8 + np.abs(cf))
        dyadic = np.ones(s.shape, bool)
        for t in (x00, x01, x10, x11):
            dyadic &= (np.abs(t) < 2048) & (t * 1024 == np.rint(t * 1024))
        chroma += [(cf + 0.5), np.where(dyadic, 0.0, e)]
    return luma, Grid(chroma[0], chroma[2], chroma[1], chroma[3])


# ---- sampling ------------------------------------------------------------------------------------------------------------------------------------------------
def _index(pos, limit):
    """the clamped index coordinate, its cell (0 .. limit - 2) and the weight inside it (0 .. 1)"""
    f = np.clip(pos - 0.5, 0.0, limit - 1.0)
    p = np.minimum(np.floor(f), limit - 2.0).astype(np.int64)
    return f, p, f - p


def sample(plane, X, Y):
    """the plane (rows x columns, any integer or float type) sampled bilinearly at the continuous positions X, Y, in float64"""
    P = np.asarray(plane, np.float64)
    h, w = P.shape
    _, x, wx = _index(X, w)
    _, y, wy = _index(Y, h)
    A, B, C, D = P[y, x], P[y, x + 1], P[y + 1, x], P[y + 1, x + 1]
    return (A * (1 - wx) + B * wx) * (1 - wy) + (C * (1 - wx) + D * wx) * wy


def _known_weight(pos, e, limit):
    """is the fp32 weight of this axis a KNOWN multiple of 2^-8?  (forced to zero outside [0, limit) by more than e; or e = 0 and 256 w an integer)"""
    f = pos - 0.5
    forced = (f + e < 0) | (f - e >= limit)
    w256 = (f - np.floor(f)) * 256
    return forced | ((e == 0) & (w256 == np.rint(w256)))


def delta(plane, grid):
    """the bound of the docstring, per sample"""
    P = np.asarray(plane, np.float64)
    h, w = P.shape
    assert h >= 2 and w >= 2 and grid.ex.max() < 0.5 and grid.ey.max() < 0.5
    dx, dy = np.abs(np.diff(P, axis=1)), np.abs(np.diff(P, axis=0))
    gx, gy = np.maximum(dx[:-1], dx[1:]), np.maximum(dy[:, :-1], dy[:, 1:])  # per cell (h - 1, w - 1)
    fx, _, _ = _index(grid.X, w)
    fy, _, _ = _index(grid.Y, h)
    (fx0, x0, _), (fx1, x1, _) = _index(grid.X - grid.ex, w), _index(grid.X + grid.ex, w)
    (fy0, y0, _), (fy1, y1, _) = _index(grid.Y - grid.ey, h), _index(grid.Y + grid.ey, h)
    Lx = np.maximum(np.maximum(gx[y0, x0], gx[y0, x1]), np.maximum(gx[y1, x0], gx[y1, x1]))
    Ly = np.maximum(np.maximum(gy[y0, x0], gy[y0, x1]), np.maximum(gy[y1, x0], gy[y1, x1]))
    ex, ey = np.maximum(fx1 - fx, fx - fx0), np.maximum(fy1 - fy, fy - fy0)
    exact = _known_weight(grid.X, grid.ex, w) & _known_weight(grid.Y, grid.ey, h)
    return Lx * ex + Ly * ey + np.where(exact, 0.0, BLEND)


def bracket(plane, grid, border=None, values=None):
    """(lo, hi, v, delta): the integer bracket of every sample of `grid` on `plane`; border: the component that samples outside the frame take, None replicates;
    values: v from a third party (grid_sample) instead of sample()"""
    h, w = np.asarray(plane).shape
    v = sample(plane, grid.X, grid.Y) if values is None else np.asarray(values, np.float64)
    d = delta(plane, grid)
    lo = np.clip(np.floor(v - d), 0, 255).astype(np.int64)
    hi = np.clip(np.floor(v + d), 0, 255).astype(np.int64)
    if border is not None:
        X, Y, ex, ey = grid.X, grid.Y, grid.ex, grid.ey
        outside = (X < -ex) | (X >= w + ex) | (Y < -ey) | (Y >= h + ey)
        inside = (X >= ex) & (X < w - ex) & (Y >= ey) & (Y < h - ey)
        lo = np.where(outside, border, np.where(inside, lo, np.minimum(lo, border)))
        hi = np.where(outside, border, np.where(inside, hi, np.maximum(hi, border)))
    return lo, hi, v, d


class Virtual:
    """the bracket of a virtual NV12 frame: Ylo, Yhi (dst_h, dst_w), UVlo, UVhi (dst_h / 2, dst_w) uint8; share = the two-valued share of the Y, U and V
    samples (two of size samples each); delta = the largest delta of each"""


def virtual_bracket(y, uv, w, h, grids, border=None, values=None):
    """the sample brackets of the luma and chroma Grids `grids` on the w x h frame (y, uv: planes with any pitch); values: (Y, U, V) from a third party"""
    luma, chroma = grids
    out = Virtual()
    out.share, out.delta, out.two, out.size = [], [], [], []
    planes = (y[:h, :w], uv[:h // 2, 0:w:2], uv[:h // 2, 1:w:2])
    los, his = [], []
    for k, plane in enumerate(planes):
        lo, hi, _, d = bracket(plane, luma if k == 0 else chroma, None if border is None else border[k], None if values is None else values[k])
        los.append(lo.astype(np.uint8))
        his.append(hi.astype(np.uint8))
        out.share.append(float((lo != hi).mean()))
        out.two.append(int((lo != hi).sum()))
        out.size.append(lo.size)
        out.delta.append(float(d.max()))
    out.Ylo, out.Yhi = los[0], his[0]
    out.UVlo, out.UVhi = np.empty((los[1].shape[0], 2 * los[1].shape[1]), np.uint8), np.empty((los[1].shape[0], 2 * los[1].shape[1]), np.uint8)
    out.UVlo[:, 0::2], out.UVlo[:, 1::2], out.UVhi[:, 0::2], out.UVhi[:, 1::2] = los[1], los[2], his[1], his[2]
    return out


def holds(vb, Y, UV):
    """is the virtual frame (Y, UV) inside the sample brackets?  -> the number of samples outside"""
    return int(((Y < vb.Ylo) | (Y > vb.Yhi)).sum() + ((UV < vb.UVlo) | (UV > vb.UVhi)).sum())


def output_bracket(oracle, vb, fcc, planes, norm):
    """(lo, hi) per output element, flat, uint8 or float32: see "Output" in the docstring"""
    outs = [oracle.convert(Y, UV, fourcc=fcc, planes=planes, normalization=norm)[0].ravel()
            for Y, UV in ((vb.Ylo, vb.UVlo), (vb.Yhi, vb.UVhi), (vb.Ylo, vb.UVhi), (vb.Yhi, vb.UVlo))]
    return np.minimum.reduce(outs), np.maximum.reduce(outs)


def outside(got, lo, hi):
    """the indices of the elements of `got` (flat, the type of lo / hi, compared as values) outside lo <= got <= hi"""
    got = np.asarray(got).ravel()
    assert got.dtype == lo.dtype and got.size == lo.size, (got.dtype, lo.dtype, got.size, lo.size)
    return np.flatnonzero(~((lo <= got) & (got <= hi)))


def tensor_values(raw, dtype):
    """the raw bytes of an fp32 / fp16 / bf16 tensor (tests/tensor_util.py's dtype names) as float32 values"""
    raw = np.ascontiguousarray(raw).view(np.uint8)
    if dtype == "f32":
        return raw.view(np.float32)
    if dtype == "f16":
        return raw.view(np.float16).astype(np.float32)
    import torch
    return torch.from_numpy(raw.view(np.int16).copy()).view(torch.bfloat16).to(torch.float32).numpy()


def tensor_bracket(oracle, vb, fcc, spec, dtype):
    """(lo, hi) as float32 values per element of the tensor form: the fp32 planar bracket sent through tests/tensor_util.py's expression.  The subtraction, the
    product by a constant and the conversion are monotone, rounding included: a positive scale keeps the order, a negative one swaps it -- so the two ends are
    sent through and sorted per element"""
    import tensor_util as T
    lo, hi = output_bracket(oracle, vb, fcc, PLANAR, True)
    channels = 1 if fcc == Y800 else 3
    a, b = (tensor_values(T.expected(q, channels, spec, dtype), dtype) for q in (lo, hi))
    return np.minimum(a, b), np.maximum(a, b)
