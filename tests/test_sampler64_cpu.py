"""CPU: the three sampling models (tests/warp_util.py, persp_util.py, remap_util.py) against tests/sampler64.py, the independent float64 evaluation of what
include/tsvpp.h promises in words -- and, first, sampler64 against a third party, torch's grid_sample in float64.

Measured (this file's own print-out; every frame of sampler64.FRAMES x every size of sampler64.DSTS x replicate and a constant border).  The share of
two-valued samples of a case is pooled over those 18 outputs per frame kind -- the cap is on that; the largest share of one single output is given behind it
(small outputs whose samples mostly lie outside a small frame under replicate: where two equal taps are blended the fp32 blend may truly fall below them).
No sample of any model was outside its bracket.  sampler64 against grid_sample: largest difference 7.1e-12 (budget 2.6e-7).
  call         case         noise Y / U / V         (one output)             band-limited Y / U / V  (one output)             largest delta Y / U / V
  warp         rot30        0.007 / 0.008 / 0.008   (0.020 / 0.033 / 0.035)  0.009 / 0.008 / 0.007   (0.043 / 0.035 / 0.039)  0.010  / 0.0050 / 0.0051
  warp         up_shear     0.010 / 0.014 / 0.013   (0.037 / 0.074 / 0.069)  0.007 / 0.012 / 0.012   (0.035 / 0.076 / 0.078)  0.0080 / 0.0039 / 0.0038
  warp         down4.6      0.004 / 0.006 / 0.006   (0.029 / 0.047 / 0.047)  0.011 / 0.006 / 0.005   (0.036 / 0.078 / 0.047)  0.013  / 0.0062 / 0.0066
  warp         half_out     0.004 / 0.004 / 0.003   (0.013 / 0.016 / 0.012)  0.012 / 0.006 / 0.006   (0.039 / 0.027 / 0.020)  0.011  / 0.0053 / 0.0049
  warp         fraction     0.005 / 0.005 / 0.007   (0.019 / 0.038 / 0.038)  0.006 / 0.006 / 0.005   (0.020 / 0.038 / 0.038)  0.0044 / 0.0022 / 0.0022
  perspective  mild         0.012 / 0.006 / 0.005   (0.026 / 0.012 / 0.012)  0.001 / 0.001 / 0.001   (0.003 / 0.001 / 0.002)  0.043  / 0.020  / 0.022
  perspective  trapezoid    0.012 / 0.006 / 0.006   (0.026 / 0.009 / 0.012)  0.001 / 0.001 / 0.001   (0.005 / 0.003 / 0.004)  0.052  / 0.022  / 0.023
  perspective  half_out     0.008 / 0.003 / 0.004   (0.020 / 0.020 / 0.012)  0.013 / 0.005 / 0.004   (0.052 / 0.031 / 0.020)  0.041  / 0.022  / 0.019
  perspective  affine_part  0.009 / 0.006 / 0.005   (0.025 / 0.016 / 0.011)  0.001 / 0.000 / 0.001   (0.004 / 0.003 / 0.002)  0.029  / 0.014  / 0.014
  remap        barrel       0.000 / 0.003 / 0.004   (0.000 / 0.012 / 0.027)  0.000 / 0.001 / 0.002   (0.001 / 0.004 / 0.008)  8.4e-5 / 0.0093 / 0.0098
  remap        affine       0.003 / 0.008 / 0.009   (0.020 / 0.033 / 0.035)  0.008 / 0.008 / 0.007   (0.042 / 0.035 / 0.039)  8.4e-5 / 0.0083 / 0.0080
  remap        fraction     0.004 / 0.007 / 0.007   (0.019 / 0.038 / 0.038)  0.005 / 0.006 / 0.006   (0.019 / 0.038 / 0.038)  8.4e-5 / 0.0073 / 0.0075
  remap        exact2       0 / 0 / 0               (0 / 0 / 0)              0 / 0 / 0               (0 / 0 / 0)              0 / 0 / 0 (every rounding exact)
  remap        leaving      0.003 / 0.006 / 0.007   (0.010 / 0.021 / 0.022)  0.007 / 0.007 / 0.006   (0.018 / 0.021 / 0.021)  8.4e-5 / 0.0090 / 0.0095
Power: the three wrong variants (a translation by 1/32 pixel; the chroma position as half the luma position of the pair's first pixel; the map read as
centre-based) leave the bracket in more than a tenth of the elements of every flavour.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import persp_util as P
import remap_util as R
import sampler64 as S
import tensor_util as T
import warp_util as W
from letterbox_util import FLAVOURS, PLANAR, RGB24, BGR24, Y800, MERGED
from util import coverage_frame, synth_nv12

ROUND_OFF = 1e-9 * 255  # the float64 budget of the agreement with grid_sample
CAP = {"noise": 0.25, "smooth": 0.05}  # two-valued samples per plane per case: keeps the bracket from going slack


def make_frames(kind):
    make = synth_nv12 if kind == "noise" else S.smooth_nv12
    return [make(w, h, seed=6400 + k, pitch=p) for k, (w, h, p) in enumerate(S.FRAMES)]


@pytest.fixture(scope="module")
def frames():
    return {kind: make_frames(kind) for kind in CAP}


# the three calls: name -> (case table, case -> input, input -> sampler64's grids, the model's virtual frame)
CALLS = {
    "warp": (S.AFFINE, lambda fn, w, h, dw, dh: fn(w, h, dw, dh), lambda m, dw, dh: S.affine_positions(m, dw, dh),
             lambda y, uv, w, h, m, dw, dh, border: W.virtual_frame(y, uv, w, h, m, dw, dh, border)),
    "perspective": (S.PERSPECTIVE, lambda fn, w, h, dw, dh: fn(w, h, dw, dh), lambda hm, dw, dh: S.perspective_positions(hm, dw, dh),
                    lambda y, uv, w, h, hm, dw, dh, border: P.virtual_frame(y, uv, w, h, hm, dw, dh, border)),
    "remap": (S.REMAP, lambda fn, w, h, dw, dh: fn(R, w, h, dw, dh), lambda xy, dw, dh: S.remap_positions(xy),
              lambda y, uv, w, h, xy, dw, dh, border: R.virtual_frame_from_map(y, uv, w, h, xy, border)),
}
CASES = [(call, name) for call, entry in CALLS.items() for name in entry[0]]


# ---- the judge is judged first -------------------------------------------------------------------------------------------------------------------------------
def grid_sample64(plane, X, Y):
    """torch's sampler in float64 at the continuous positions X, Y of `plane`: bilinear, border padding, align_corners=False"""
    h, w = plane.shape
    g = torch.from_numpy(np.stack((2 * X / w - 1, 2 * Y / h - 1), axis=-1))[None]
    t = torch.from_numpy(np.ascontiguousarray(plane, np.float64))[None, None]
    return F.grid_sample(t, g, mode="bilinear", padding_mode="border", align_corners=False)[0, 0].numpy()


def planes_of(frame, w, h):
    y, uv = frame
    return y[:h, :w], uv[:h // 2, 0:w:2], uv[:h // 2, 1:w:2]


def theta_of(m, w, h, dw, dh):
    """the affine_grid theta (float64) of the centre-based matrix m on a w x h frame and a dw x dh output: with xb = 2 u / dw - 1 the normalised output
    position and X = (gx + 1) w / 2 the source's, gx = (2 / w)(m0 dw / 2 (xb + 1) + m1 dh / 2 (yb + 1) + m2) - 1"""
    rows = []
    for (a, b, c), size in ((m[0:3], w), (m[3:6], h)):
        rows.append([a * dw / size, b * dh / size, (a * dw + b * dh + 2 * c) / size - 1])
    return torch.tensor([rows], dtype=torch.float64)


def matrix_of(theta, w, h, dw, dh):
    """theta_of the other way round: the matrix equivalent of an affine_grid theta, as float32 values"""
    out = []
    for (a, b, c), size in ((theta[0], w), (theta[1], h)):
        out += [a * size / dw, b * size / dh, size / 2 * (c + 1 - a - b)]
    return S.f32(out)


def third_party_grids(w, h, dw, dh):
    """name -> (luma Grid, chroma Grid, the luma X, Y the third party builds): an affine grid from F.affine_grid, a projective grid, a barrel grid"""
    c, s = math.cos(0.4), math.sin(0.4)
    m = matrix_of([[0.8 * c, -0.7 * s, 0.05], [0.8 * s, 0.7 * c, -0.1]], w, h, dw, dh)
    out = {}
    th = theta_of(m, w, h, dw, dh)
    pair = []
    for rows, cols, ww, hh in ((dh, dw, w, h), (dh // 2, dw // 2, w // 2, h // 2)):
        g = F.affine_grid(th, (1, 1, rows, cols), align_corners=False)[0].numpy()
        pair.append(((g[..., 0] + 1) * ww / 2, (g[..., 1] + 1) * hh / 2))
    out["affine_grid"] = (S.affine_positions(m, dw, dh), pair, m)
    hm = S.PERSPECTIVE["trapezoid"](w, h, dw, dh)
    out["projective"] = (S.perspective_positions(hm, dw, dh), None, hm)
    xy = R.barrel(dw, dh, w, h)
    out["barrel"] = (S.remap_positions(xy), None, xy)
    return out


def test_sampler64_is_grid_sample(frames):
    """on luma and on both chroma planes, for an affine grid from F.affine_grid, a projective grid and a barrel grid, sampler64's value is grid_sample's
    (float64, bilinear, border padding, align_corners=False) within 1e-9 * 255 -- and affine_grid's own positions are sampler64's: the pair's centre, the
    half-pixel shift and the chroma siting mean to torch what they mean here"""
    worst = 0.0
    for k, (w, h, _) in enumerate(S.FRAMES):
        for dw, dh in S.DSTS:
            for name, (grids, theirs, _) in third_party_grids(w, h, dw, dh).items():
                for kind in CAP:
                    for p, plane in enumerate(planes_of(frames[kind][k], w, h)):
                        g = grids[0 if p == 0 else 1]
                        ours = S.sample(plane, g.X, g.Y)
                        ref = grid_sample64(plane, g.X, g.Y)
                        worst = max(worst, float(np.abs(ours - ref).max()))
                        assert np.abs(ours - ref).max() <= ROUND_OFF, (name, kind, p, (w, h), (dw, dh))
                        if theirs is not None:
                            X, Y = theirs[0 if p == 0 else 1]
                            assert np.abs(X - g.X).max() <= 1e-9 and np.abs(Y - g.Y).max() <= 1e-9, (name, (w, h), (dw, dh))
                            assert np.abs(grid_sample64(plane, X, Y) - ours).max() <= 255 * 2e-9 * 2  # (positions 1e-9 apart, taps at most 255 apart, two axes)
    print(f"sampler64 against grid_sample: largest difference {worst:.3g}")


def block_mean(a):
    return (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]) / 4


def test_helpers_mean_what_grid_sample_and_opencv_mean(frames):
    """ts.remap_from_grid's map and the matrix equivalent of an affine_grid theta put the model's output inside the bracket built around grid_sample's OWN
    values; ts.warp_from_opencv and ts.perspective_from_opencv put it inside the bracket around a float64 evaluation of OpenCV's index-based M (j, i, 1)"""
    import tensor_stream as ts
    k = 1
    w, h, _ = S.FRAMES[k]
    dw, dh = 70, 66
    y, uv = frames["noise"][k]
    planes = planes_of(frames["noise"][k], w, h)
    # affine_grid theta -> matrix
    grids, theirs, m = third_party_grids(w, h, dw, dh)["affine_grid"]
    values = [grid_sample64(planes[p], *theirs[0 if p == 0 else 1]) for p in range(3)]
    vb = S.virtual_bracket(y, uv, w, h, grids, None, values)
    assert S.holds(vb, *W.virtual_frame(y, uv, w, h, m, dw, dh)) == 0
    # a grid_sample grid (float32, as the helper takes it) -> map.  The helper rounds three times: g + 1, its product by w, the difference to 1 (the halving is
    # exact) -- eps (|g + 1| w + |(g + 1) w| + |(g + 1) w - 1|) / 2 on the entry; the chroma coordinate is the mean of four entries, halved
    barrel = R.barrel(dw, dh, w, h).astype(np.float64)
    grid32 = np.stack(((2 * barrel[..., 0] + 1) / w - 1, (2 * barrel[..., 1] + 1) / h - 1), axis=-1).astype(np.float32)
    xy = ts.remap_from_grid(grid32, w, h)
    assert xy.dtype == np.float32 and xy.shape == (dh, dw, 2)
    g64 = grid32.astype(np.float64)
    X, Y = (g64[..., 0] + 1) * w / 2, (g64[..., 1] + 1) * h / 2
    ex, ey = (S.EPS * S.SLACK * (2 * np.abs(g64[..., c] + 1) * size + np.abs((g64[..., c] + 1) * size - 1)) / 2 for c, size in ((0, w), (1, h)))
    mine = S.remap_positions(xy)[1]
    grids = (S.Grid(X, Y, ex, ey), S.Grid(block_mean(X) / 2, block_mean(Y) / 2, mine.ex + block_mean(ex) / 2, mine.ey + block_mean(ey) / 2))
    values = [grid_sample64(planes[p], grids[0 if p == 0 else 1].X, grids[0 if p == 0 else 1].Y) for p in range(3)]
    for border in S.BORDERS:
        vb = S.virtual_bracket(y, uv, w, h, grids, border, values)
        assert max(vb.share) <= CAP["noise"]
        assert S.holds(vb, *R.virtual_frame_from_map(y, uv, w, h, xy, border)) == 0, border
    # OpenCV's index-based inverse matrices (entries that float32 holds): source index = M (j, i, 1), continuous = index + 1/2
    j, i = np.meshgrid(np.arange(dw, dtype=np.float64), np.arange(dh, dtype=np.float64))
    cj, ci = np.meshgrid(2 * np.arange(dw // 2, dtype=np.float64) + 0.5, 2 * np.arange(dh // 2, dtype=np.float64) + 0.5)  # the pair's centre, as an index
    M = [[1.25, -0.5, 20.75], [0.375, 1.5, -3.125]]
    m = S.f32(ts.warp_from_opencv(M))
    assert m[0] == 1.25 and m[1] == -0.5 and m[3] == 0.375 and m[4] == 1.5  # (only the translations can round: eps |m2|, halved on the chroma grid)
    luma, chroma = S.affine_positions(m, dw, dh)
    grids = (S.Grid(*[r[0] * j + r[1] * i + r[2] + 0.5 for r in M], luma.ex + S.EPS * abs(m[2]), luma.ey + S.EPS * abs(m[5])),
             S.Grid(*[(r[0] * cj + r[1] * ci + r[2] + 0.5) / 2 for r in M], chroma.ex + S.EPS * abs(m[2]) / 2, chroma.ey + S.EPS * abs(m[5]) / 2))
    for border in S.BORDERS:
        assert S.holds(S.virtual_bracket(y, uv, w, h, grids, border), *W.virtual_frame(y, uv, w, h, m, dw, dh, border)) == 0, border
    M = [[1.25, -0.5, 20.75], [0.375, 1.5, -3.125], [0.001953125, 0.00390625, 1.5]]
    hm = S.f32(ts.perspective_from_opencv(M))
    luma, chroma = S.perspective_positions(hm, dw, dh, entry_ulps=1)  # (every entry of the helper's result may round once)
    den, cden = M[2][0] * j + M[2][1] * i + M[2][2], M[2][0] * cj + M[2][1] * ci + M[2][2]
    grids = (S.Grid(*[(r[0] * j + r[1] * i + r[2]) / den + 0.5 for r in M[:2]], luma.ex, luma.ey),
             S.Grid(*[((r[0] * cj + r[1] * ci + r[2]) / cden + 0.5) / 2 for r in M[:2]], chroma.ex, chroma.ey))
    for border in S.BORDERS:
        assert S.holds(S.virtual_bracket(y, uv, w, h, grids, border), *P.virtual_frame(y, uv, w, h, hm, dw, dh, border)) == 0, border


def test_box_and_quad_helpers_geometrically():
    """ts.warp_rotated_box and ts.perspective_from_quad in float64: the output's corners land on the box's / the quad's corners within 1e-4 pixel"""
    import tensor_stream as ts
    for w, h, _ in S.FRAMES:
        for dw, dh in S.DSTS:
            corners = [(0, 0), (dw, 0), (dw, dh), (0, dh)]
            for cx, cy, bw, bh, ang in ((w / 2, h / 2, 1.7 * dw, 1.7 * dh, math.radians(30)), (0, h / 2, w, h, 0.2), (w / 3, h / 5, 40.5, 17.25, -2.0)):
                m = ts.warp_rotated_box(cx, cy, bw, bh, ang, dw, dh)
                c, s = math.cos(ang), math.sin(ang)
                for (u, v), (sx, sy) in zip(corners, ((-1, -1), (1, -1), (1, 1), (-1, 1))):
                    want = (cx + sx * bw / 2 * c - sy * bh / 2 * s, cy + sx * bw / 2 * s + sy * bh / 2 * c)
                    got = (m[0] * u + m[1] * v + m[2], m[3] * u + m[4] * v + m[5])
                    assert math.hypot(got[0] - want[0], got[1] - want[1]) <= 1e-4, (m, (u, v))
            for quad in (S.MILD, S.TRAPEZOID, S.HALF_OUT):
                q = [(x * w, y * h) for x, y in quad]
                hm = ts.perspective_from_quad(q, dw, dh)
                for (u, v), want in zip(corners, q):
                    d = hm[6] * u + hm[7] * v + hm[8]
                    got = ((hm[0] * u + hm[1] * v + hm[2]) / d, (hm[3] * u + hm[4] * v + hm[5]) / d)
                    assert math.hypot(got[0] - want[0], got[1] - want[1]) <= 1e-4, (hm, (u, v))


def test_the_colour_back_end_is_monotone(oracle):
    """what the output bracket rests on, over all 2^24 (Y, U, V): R rises with Y and V, B with Y and U, G rises with Y and falls with U and V; no channel moves
    the other way in any component -- uint8 and fp32, through every rounding and the truncation"""
    y, uv = coverage_frame()
    for norm in (False, True):
        out = oracle.convert(y, uv, fourcc=RGB24, planes=PLANAR, normalization=norm, nthreads=4)[0].reshape(3, 2048, 2, 2048, 2)
        cube = out.transpose(0, 1, 3, 2, 4).reshape(3, 256, 256, 256).astype(np.float32)  # [channel, V, U, Y]
        for c, (dv, du) in enumerate(((1, 1), (-1, -1), (1, 1))):  # the sign each channel may move with V and with U (R: U is free to be constant; B: V)
            assert (np.diff(cube[c], axis=2) >= 0).all(), ("Y", c, norm)
            assert (dv * np.diff(cube[c], axis=0) >= 0).all(), ("V", c, norm)
            assert (du * np.diff(cube[c], axis=1) >= 0).all(), ("U", c, norm)
    grey = oracle.convert(y, uv, fourcc=Y800, planes=MERGED, normalization=False, nthreads=4)[0].reshape(2048, 2, 2048, 2)
    assert (np.diff(grey.transpose(0, 2, 1, 3).reshape(256, 256, 256).astype(np.int16), axis=2) >= 0).all()


# ---- the three models inside the bracket ---------------------------------------------------------------------------------------------------------------------
def check_flavours(oracle, vb, Y, UV, what):
    """the model's virtual frame through the oracle, every flavour and two tensor forms, against the output bracket: no element outside"""
    for fcc, planes, norm in FLAVOURS:
        lo, hi = S.output_bracket(oracle, vb, fcc, planes, norm)
        got = oracle.convert(Y, UV, fourcc=fcc, planes=planes, normalization=norm)[0].ravel()
        bad = S.outside(got, lo, hi)
        assert bad.size == 0, (what, fcc, planes, norm, bad.size, bad[:4])
    for spec, dtype in (("imagenet", T.F16), ("corner", T.BF16)):
        lo, hi = S.tensor_bracket(oracle, vb, BGR24, T.SPECS[spec], dtype)
        q = oracle.convert(Y, UV, fourcc=BGR24, planes=PLANAR, normalization=True)[0]
        bad = S.outside(S.tensor_values(T.expected(q, 3, T.SPECS[spec], dtype), dtype), lo, hi)
        assert bad.size == 0, (what, spec, dtype, bad.size)


@pytest.mark.parametrize("call,name", CASES)
def test_model_inside_the_bracket(oracle, frames, call, name):
    """every frame x every output size x replicate and a constant border x noise and the band-limited frame: the model's virtual frame lies inside the sample
    brackets, its conversion inside the output bracket in every flavour, and the share of two-valued samples stays under its cap"""
    table, make, positions, model = CALLS[call]
    worst = {kind: [0.0, 0.0, 0.0] for kind in CAP}
    two, size = {kind: np.zeros(3) for kind in CAP}, {kind: np.zeros(3) for kind in CAP}
    delta = [0.0, 0.0, 0.0]
    for k, (w, h, _) in enumerate(S.FRAMES):
        for dw, dh in S.DSTS:
            arg = make(table[name], w, h, dw, dh)
            grids = positions(arg, dw, dh)
            for kind in CAP:
                y, uv = frames[kind][k]
                for border in S.BORDERS:
                    vb = S.virtual_bracket(y, uv, w, h, grids, border)
                    Y, UV = model(y, uv, w, h, arg, dw, dh, border)
                    what = (call, name, kind, (w, h), (dw, dh), border)
                    assert S.holds(vb, Y, UV) == 0, what
                    worst[kind] = [max(a, b) for a, b in zip(worst[kind], vb.share)]
                    two[kind] += vb.two
                    size[kind] += vb.size
                    delta = [max(a, b) for a, b in zip(delta, vb.delta)]
                    check_flavours(oracle, vb, Y, UV, what)
    share = {kind: two[kind] / size[kind] for kind in CAP}
    print(f"{call:12s} {name:12s} two-valued Y/U/V: " + " ".join(f"{kind} " + "/".join(f"{v:.3f}" for v in share[kind]) + " (largest single output "
          + "/".join(f"{v:.3f}" for v in worst[kind]) + ")" for kind in CAP) + " largest delta " + "/".join(f"{v:.2g}" for v in delta))
    for kind in CAP:
        assert share[kind].max() <= CAP[kind], (call, name, kind, share[kind])


# ---- power: a check that cannot fail proves nothing ----------------------------------------------------------------------------------------------------------
POWER_GEO = (1, (70, 66))  # frame 128 x 72, noise


def fails_everywhere(oracle, vb, Y, UV, what):
    """the wrong virtual frame leaves the sample brackets, and its conversion leaves the output bracket in EVERY flavour -- by more than a tenth of the elements:
    on noise a slip of 1/32 pixel moves a sample by (mean tap difference 85) / 32, several levels"""
    assert S.holds(vb, Y, UV) > 0.1 * (Y.size + UV.size), what
    for fcc, planes, norm in FLAVOURS:
        lo, hi = S.output_bracket(oracle, vb, fcc, planes, norm)
        got = oracle.convert(Y, UV, fourcc=fcc, planes=planes, normalization=norm)[0].ravel()
        assert S.outside(got, lo, hi).size > 0.1 * got.size, (what, fcc, planes, norm)


def test_power_warp(oracle, frames):
    k, (dw, dh) = POWER_GEO
    w, h, _ = S.FRAMES[k]
    y, uv = frames["noise"][k]
    m = S.AFFINE["rot30"](w, h, dw, dh)
    vb = S.virtual_bracket(y, uv, w, h, S.affine_positions(m, dw, dh))
    right = W.virtual_frame(y, uv, w, h, m, dw, dh)
    assert S.holds(vb, *right) == 0
    shifted = S.f32(m[:2] + (m[2] + 1 / 32,) + m[3:])
    fails_everywhere(oracle, vb, *W.virtual_frame(y, uv, w, h, shifted, dw, dh), "translated by 1/32")
    # the chroma position as half of the luma position of the pair's first pixel (u, v) = (2 cj + 1/2, 2 ci + 1/2): the matrix that gives the model's chroma
    # grid that position is m with m2 - (m0 + m1) / 2, m5 - (m3 + m4) / 2
    sited = S.f32(m[:2] + (m[2] - (m[0] + m[1]) / 2,) + m[3:5] + (m[5] - (m[3] + m[4]) / 2,))
    wrong = W.virtual_frame(y, uv, w, h, sited, dw, dh)[1]
    assert ((wrong < vb.UVlo) | (wrong > vb.UVhi)).sum() > 0.1 * wrong.size
    for fcc, planes, norm in FLAVOURS:
        if fcc != Y800:
            lo, hi = S.output_bracket(oracle, vb, fcc, planes, norm)
            got = oracle.convert(right[0], wrong, fourcc=fcc, planes=planes, normalization=norm)[0].ravel()
            assert S.outside(got, lo, hi).size > 0.1 * got.size, ("chroma siting", fcc, planes, norm)


def test_power_perspective(oracle, frames):
    k, (dw, dh) = POWER_GEO
    w, h, _ = S.FRAMES[k]
    y, uv = frames["noise"][k]
    hm = S.PERSPECTIVE["mild"](w, h, dw, dh)
    vb = S.virtual_bracket(y, uv, w, h, S.perspective_positions(hm, dw, dh))
    right = P.virtual_frame(y, uv, w, h, hm, dw, dh)
    assert S.holds(vb, *right) == 0
    # X + 1/32 = (n + nw / 32) / nw
    shifted = S.f32(tuple(hm[c] + hm[6 + c] / 32 for c in range(3)) + hm[3:])
    fails_everywhere(oracle, vb, *P.virtual_frame(y, uv, w, h, shifted, dw, dh), "translated by 1/32")
    # the chroma position from (u, v) = (2 cj + 1/2, 2 ci + 1/2): the homography evaluated a quarter pair earlier, H(u - 1/2, v - 1/2)
    sited = S.f32(tuple(v for r in (0, 3, 6) for v in (hm[r], hm[r + 1], hm[r + 2] - (hm[r] + hm[r + 1]) / 2)))
    wrong = P.virtual_frame(y, uv, w, h, sited, dw, dh)[1]
    assert ((wrong < vb.UVlo) | (wrong > vb.UVhi)).sum() > 0.1 * wrong.size
    for fcc, planes, norm in FLAVOURS:
        if fcc != Y800:
            lo, hi = S.output_bracket(oracle, vb, fcc, planes, norm)
            got = oracle.convert(right[0], wrong, fourcc=fcc, planes=planes, normalization=norm)[0].ravel()
            assert S.outside(got, lo, hi).size > 0.1 * got.size, ("chroma siting", fcc, planes, norm)


def test_power_remap(oracle, frames):
    k, (dw, dh) = POWER_GEO
    w, h, _ = S.FRAMES[k]
    y, uv = frames["noise"][k]
    xy = S.REMAP["affine"](R, w, h, dw, dh)
    vb = S.virtual_bracket(y, uv, w, h, S.remap_positions(xy))
    assert S.holds(vb, *R.virtual_frame_from_map(y, uv, w, h, xy)) == 0
    shifted = xy.copy()
    shifted[..., 0] += np.float32(1 / 32)
    fails_everywhere(oracle, vb, *R.virtual_frame_from_map(y, uv, w, h, shifted), "translated by 1/32")
    centre_based = (xy - np.float32(0.5)).astype(np.float32)  # the entries read as continuous positions
    fails_everywhere(oracle, vb, *R.virtual_frame_from_map(y, uv, w, h, centre_based), "centre-based")
