"""CPU: tsvpp_convert_perspective's host side and its reference model (tests/persp_util.py) -- the model's identities (an affine homography is the affine model,
h and 4 h agree), the ABI (symbols, struct size, every status from tsvpp_describe_perspective without a context, the horizon rule among them), the homography
helpers, the describe line and the footprint property: every tap of a tile lies inside the interval box the host (and, from the same function, the kernel)
computes for it.  Every comparison is on raw bits."""
import ctypes

import numpy as np
import pytest

import persp_util as P
import warp_util as W
from warp_util import BGR24, BILINEAR, MERGED, PLANAR, RGB24, Y800, F32

OK, UNSUPPORTED, ERROR = 0, -2, -3
H0 = (2, 0, 0, 0, 1.125, 0, 0, 0, 1)


@pytest.fixture(scope="module")
def native():
    from tensor_stream import _native
    _native.lib()
    return _native


def u32(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---- 1. the model's identities ----------------------------------------------------------------------------------------------------------------------------

def _seeded_affine(rng):
    return tuple(float(F32(v)) for v in (rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-400, 400), rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-400, 400)))


def test_last_row_001_is_the_affine_model_on_both_grids():
    """h = (m, 0, 0, 1): cx = m2 - 0.5f is tx, cx' = m2 0.5f - 0.5f is ctx, nw = rw = 1 and nx * 1 is exact -- warp_util.coords bit for bit"""
    rng = np.random.default_rng(501)
    rows, cols = np.arange(66), np.arange(70)
    for _ in range(50):
        m = _seeded_affine(rng)
        tx, ty, ctx, cty = W.translations(m)
        luma, chroma = P.terms(P.affine(m))
        for t, (a, b), (r, c) in ((luma, (tx, ty), (rows, cols)), (chroma, (ctx, cty), (rows[:33], cols[:35]))):
            fx, fy = P.coords(t, r, c)
            wx, wy = W.coords(m, a, b, r, c)
            assert np.array_equal(u32(fx), u32(wx)) and np.array_equal(u32(fy), u32(wy)), m


def _seeded_quads(rng, w, h, jitter):
    base = np.array([(20, 20), (w - 20, 20), (w - 20, h - 20), (20, h - 20)], np.float64)
    return base + rng.uniform(-jitter, jitter, (4, 2))


def test_model_is_invariant_under_4h():
    """every operation scales exactly by a power of two: h and 4 h give the same coordinates on both grids"""
    rng = np.random.default_rng(502)
    rows, cols = np.arange(66), np.arange(70)
    n = 0
    for _ in range(50):
        h = P.from_quad(_seeded_quads(rng, 322, 182, 40), 70, 66)
        if not P.in_domain(h, 70, 66):
            continue
        n += 1
        h4 = tuple(4.0 * v for v in h)
        assert P.in_domain(h4, 70, 66)
        for grid, (r, c) in ((0, (rows, cols)), (1, (rows[:33], cols[:35]))):
            a, b = P.coords(P.terms(h)[grid], r, c), P.coords(P.terms(h4)[grid], r, c)
            assert np.array_equal(u32(a[0]), u32(b[0])) and np.array_equal(u32(a[1]), u32(b[1])), h
    assert n >= 40


# ---- 2. ABI and statuses -----------------------------------------------------------------------------------------------------------------------------------

def _params(native, dst=(64, 64), rt=BILINEAR, fcc=RGB24, planes=MERGED, norm=0, crop=(0, 0, 0, 0)):
    return native.Params(crop[0], crop[1], crop[2], crop[3], dst[0], dst[1], rt, fcc, planes, norm)


def _persp(native, h=H0, frame=0):
    return native.Persp(frame, (ctypes.c_float * 9)(*h))


def _describe(native, p, frames, persps, border=(-1, -1, -1), spec=None, n_frames=None, n=None, aligned=1):
    L = native.lib()
    buf = ctypes.create_string_buffer(512)
    fr = (native.NV12 * max(len(frames), 1))(*frames) if frames is not None else None
    qs = (native.Persp * max(len(persps), 1))(*persps) if persps is not None else None
    nf = len(frames) if n_frames is None else n_frames
    nq = len(persps) if n is None else n
    pp = ctypes.byref(p) if p is not None else None
    if spec is None:
        sts = L.tsvpp_describe_perspective(pp, nf, fr, nq, qs, border[0], border[1], border[2], aligned, buf, len(buf))
    else:
        sp = ctypes.byref(spec) if spec != "null" else None
        sts = L.tsvpp_describe_perspective_tensor(pp, sp, nf, fr, nq, qs, border[0], border[1], border[2], aligned, buf, len(buf))
    return sts, buf.value.decode()


def test_symbols_and_struct_size(native):
    assert ctypes.sizeof(native.Persp) == 40
    assert native.TSVPP_MAX_PERSP == 32
    L = native.lib()
    for s in ("tsvpp_convert_perspective", "tsvpp_describe_perspective", "tsvpp_convert_perspective_tensor", "tsvpp_describe_perspective_tensor", "tsvpp_persp_from_quad",
              "tsvpp_persp_footprint"):
        assert s in native.SYMBOLS
        getattr(L, s)


def _with(k, v, base=H0):
    h = list(base)
    h[k] = v
    return h


def test_statuses_in_their_order_without_a_context(native):
    N = native
    fr = [N.NV12(None, None, 192, 192, 128, 72)]
    qs = [_persp(N)]
    p = _params(N)
    assert _describe(N, p, fr, qs)[0] == OK
    # TSVPP_ERROR: every case of warp_plan
    assert _describe(N, None, fr, qs)[0] == ERROR
    assert _describe(N, p, None, qs, n_frames=1)[0] == ERROR
    assert _describe(N, p, fr, None, n=1)[0] == ERROR
    assert N.lib().tsvpp_describe_perspective(ctypes.byref(p), 1, (N.NV12 * 1)(*fr), 1, (N.Persp * 1)(*qs), -1, -1, -1, 1, None, 0) == ERROR
    assert _describe(N, p, fr, qs, n_frames=0)[0] == ERROR
    assert _describe(N, p, fr, qs, n=0)[0] == ERROR
    assert _describe(N, p, [N.NV12(None, None, 192, 192, 0, 72)], qs)[0] == ERROR
    assert _describe(N, p, [N.NV12(None, None, 100, 192, 128, 72)], qs)[0] == ERROR
    assert _describe(N, p, [N.NV12(None, None, 192, 100, 128, 72)], qs)[0] == ERROR
    assert _describe(N, p, fr, [_persp(N, frame=1)])[0] == ERROR
    assert _describe(N, p, fr, [_persp(N, frame=-1)])[0] == ERROR
    assert _describe(N, _params(N, dst=(0, 64)), fr, qs)[0] == ERROR
    assert _describe(N, _params(N, dst=(64, -2)), fr, qs)[0] == ERROR
    assert _describe(N, _params(N, crop=(0, 0, 32, 32)), fr, qs)[0] == ERROR
    for border in ((256, 128, 128), (-2, -2, -2), (-1, 128, 128), (114, -1, 128), (114, 128, -1), (0, 0, 300)):
        assert _describe(N, p, fr, qs, border=border)[0] == ERROR, border
    for bad in (float("nan"), float("inf"), -float("inf")):
        for k in range(9):
            assert _describe(N, p, fr, [_persp(N, _with(k, bad))])[0] == ERROR, (k, bad)
    # TSVPP_UNSUPPORTED: every case of warp_plan
    assert _describe(N, _params(N, dst=(63, 64)), fr, qs)[0] == UNSUPPORTED
    assert _describe(N, _params(N, dst=(64, 33)), fr, qs)[0] == UNSUPPORTED
    assert _describe(N, p, [N.NV12(None, None, 192, 192, 127, 72)], qs)[0] == UNSUPPORTED
    assert _describe(N, p, [N.NV12(None, None, 192, 192, 128, 71)], qs)[0] == UNSUPPORTED
    for rt in (0, 2, 3, 7):  # NEAREST, BICUBIC, AREA, unknown
        assert _describe(N, _params(N, rt=rt), fr, qs)[0] == UNSUPPORTED, rt
    for fcc in (3, 4, 5, 6):
        if fcc not in (Y800, RGB24, BGR24):
            assert _describe(N, _params(N, fcc=fcc), fr, qs)[0] == UNSUPPORTED, fcc
    for k in range(9):
        assert _describe(N, p, fr, [_persp(N, _with(k, -(2.0 ** 24) - 2))])[0] == UNSUPPORTED, k
    for k in range(6):  # (a numerator entry at the bound is inside it; a denominator entry of 2^24 moves the horizon)
        assert _describe(N, p, fr, [_persp(N, _with(k, 2.0 ** 24))])[0] == OK, k
    assert _describe(N, p, fr, [_persp(N, _with(8, 2.0 ** 24))])[0] == OK
    assert _describe(N, _params(N, dst=(32768, 32768), norm=1), fr, qs)[0] == UNSUPPORTED  # 12 GiB
    # an ERROR condition wins over an UNSUPPORTED one, the horizon included
    assert _describe(N, _params(N, dst=(63, 64), rt=3), fr, qs, border=(256, 0, 0))[0] == ERROR
    assert _describe(N, _params(N, rt=2), fr, [_persp(N, _with(0, float("nan")))])[0] == ERROR
    assert _describe(N, p, fr, [_persp(N, _with(6, -1.0))], border=(256, 0, 0))[0] == ERROR


def test_the_horizon_rule(native):
    """nw >= 2^-64 at the corner pixels of the luma grid and the corner pairs of the chroma grid, by the contract's own expression: the status is the model's"""
    N = native
    fr = [N.NV12(None, None, 192, 192, 128, 72)]
    p = _params(N)  # 64 x 64: the last luma centre is 63.5
    cases = [(_with(6, -1 / 32), False), (_with(6, -1 / 128), True), (_with(7, -1 / 32), False), (_with(7, -1 / 128), True), (_with(8, -1.0), False), (_with(8, 0.0), False),
             (_with(6, 1.0, _with(8, -0.25)), True),    # the horizon at u = 0.25, left of the first centre: nw = u - 0.25 is positive at every centre
             (_with(6, 1.0, _with(8, -0.5)), False),    # ... through the first centre: nw = 0 there
             (_with(8, 2.0 ** -64), True), (_with(8, 2.0 ** -65), False),
             # 2^-64 exactly at the far corner: g = -2^-70, hh = 0, k = 127.5 * 2^-70 -> nw(63.5) = 64 * 2^-70; one ulp less fails
             (_with(6, -(2.0 ** -70), _with(8, 127.5 * 2.0 ** -70)), True), (_with(6, -(2.0 ** -70), _with(8, float(np.nextafter(F32(127.5 * 2.0 ** -70), F32(0))))), False)]
    for h, ok in cases:
        h = tuple(float(F32(v)) for v in h)
        assert P.in_domain(h, 64, 64) == ok, h
        assert _describe(N, p, fr, [_persp(N, h)])[0] == (OK if ok else UNSUPPORTED), h
    # the second of two outputs decides as well
    assert _describe(N, p, fr, [_persp(N), _persp(N, _with(6, -1 / 32))])[0] == UNSUPPORTED


def test_no_horizon_is_caught_by_the_chroma_corner_rule_alone(native):
    """A case that only the chroma corners refuse cannot be constructed: the rule is implied by the luma one, in fp32 as in exact arithmetic.  The corner where
    the denominator is least is the same on both grids (the signs of g and hh choose it).  There 2 u' <= u at the far end -- (float)(w / 2 - 1) + 0.5f, doubled,
    never exceeds (float)(w - 1) + 0.5f, whatever the two round to -- and 2 u' = 1 >= 0.5 = u at the near end, likewise for v; g' u' = g (2 u') exactly; and fmaf
    is monotone in each operand.  So the least chroma denominator is at least the least luma one.  The rule stays in the contract (it costs four fmafs per output
    and states the kernel's precondition on its own grid); this test pins the implication on the model for horizons that graze the far corner, at output sizes up
    to where the centres stop being exact, and the status for each."""
    N = native
    fr = [N.NV12(None, None, 192, 192, 128, 72)]
    rng = np.random.default_rng(505)
    refused = 0
    for k in range(300):
        dw, dh = [(64, 64), (70, 66), (30, 34), (2 ** 24 + 2, 2), (2 ** 25 + 6, 2)][k % 5]
        g, hh = rng.uniform(-1, 1, 2) * 2.0 ** rng.integers(-30, 1, 2)
        far = max(g * 0.5, g * (dw - 0.5)) * 0 + min(g * 0.5, g * (dw - 0.5)) + min(hh * 0.5, hh * (dh - 0.5))
        kk = float(F32(-far * (1 + rng.uniform(-3, 3) * 2.0 ** -23)))  # the least denominator is within a few ulps of zero, on either side
        h = tuple(float(F32(v)) for v in (1, 0, 0, 0, 1, 0, g, hh, kk))
        if not np.isfinite(h).all() or max(abs(v) for v in h) > 2.0 ** 24:
            continue
        luma, chroma = P.terms(h)
        lmin = P.denominators(luma, [0, dh - 1], [0, dw - 1]).min()
        cmin = P.denominators(chroma, [0, dh // 2 - 1], [0, dw // 2 - 1]).min()
        assert cmin >= lmin, (h, dw, dh, lmin, cmin)
        ok = bool(lmin >= P.MIN_DENOMINATOR)
        refused += not ok
        assert P.in_domain(h, dw, dh) == ok
        assert _describe(N, _params(N, dst=(dw, dh), fcc=Y800), fr, [_persp(N, h)])[0] == (OK if ok else UNSUPPORTED), (h, dw, dh)
    assert 50 <= refused <= 250, refused


def test_tensor_describe_adds_the_spec_rules_behind_the_request(native):
    N = native
    fr = [N.NV12(None, None, 192, 192, 128, 72)]
    qs = [_persp(N)]
    spec = N.TensorSpec(N.TSVPP_F16, (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1))
    ok = _params(N, fcc=BGR24, planes=PLANAR, norm=1)
    sts, line = _describe(N, ok, fr, qs, spec=spec, border=(114, 128, 128))
    assert sts == OK and "kernel=vpp_persp_tensor<PLANAR,EL_HALF,vec," in line and "out=f16_planar" in line and line.endswith("border=114,128,128")
    # rule 1 first: the request's own status, the horizon included
    assert _describe(N, _params(N, fcc=BGR24, planes=PLANAR, norm=1, rt=2), fr, qs, spec="null")[0] == UNSUPPORTED
    assert _describe(N, ok, fr, [_persp(N, frame=3)], spec=N.TensorSpec(9, (ctypes.c_float * 3)(), (ctypes.c_float * 3)(1, 1, 1)))[0] == ERROR
    assert _describe(N, ok, fr, [_persp(N, _with(6, -1.0))], spec="null")[0] == UNSUPPORTED
    # rule 2
    assert _describe(N, ok, fr, qs, spec="null")[0] == ERROR
    assert _describe(N, ok, fr, qs, spec=N.TensorSpec(N.TSVPP_F16, (ctypes.c_float * 3)(0, float("nan"), 0), (ctypes.c_float * 3)(1, 1, 1)))[0] == ERROR
    assert _describe(N, ok, fr, qs, spec=N.TensorSpec(N.TSVPP_F16, (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 0, 1)))[0] == ERROR
    # rule 3
    assert _describe(N, ok, fr, qs, spec=N.TensorSpec(9, (ctypes.c_float * 3)(), (ctypes.c_float * 3)(1, 1, 1)))[0] == UNSUPPORTED
    assert _describe(N, _params(N, fcc=BGR24, planes=PLANAR, norm=0), fr, qs, spec=spec)[0] == UNSUPPORTED
    assert _describe(N, _params(N, fcc=BGR24, planes=MERGED, norm=1), fr, qs, spec=spec)[0] == UNSUPPORTED
    assert _describe(N, _params(N, fcc=Y800, planes=MERGED, norm=1), fr, qs, spec=spec)[0] == OK


# ---- 3. the homography helpers -----------------------------------------------------------------------------------------------------------------------------

def _apply(h, u, v):
    d = h[6] * u + h[7] * v + h[8]
    return (h[0] * u + h[1] * v + h[2]) / d, (h[3] * u + h[4] * v + h[5]) / d


def test_from_quad(native):
    import tensor_stream as ts
    rng = np.random.default_rng(503)
    # against the formula of the header evaluated in Python doubles, bit-equal as float32
    for k in range(40):
        dw, dh = [(70, 66), (112, 112), (64, 30)][k % 3]
        quad = _seeded_quads(rng, 322, 182, (10, 40, 120)[k % 3])
        want = P.from_quad(quad, dw, dh)
        got = ts.perspective_from_quad([tuple(q) for q in quad], dw, dh)
        assert np.array_equal(u32(got), u32(want)), (quad, got, want)
        # the four output corners land on the quad (in double, on the float32 entries; keystones only: where a quad folds over, the map amplifies the
        # entries' rounding past any fixed bound)
        if k % 3 == 2:
            continue
        for (u, v), (x, y) in zip(((0, 0), (dw, 0), (dw, dh), (0, dh)), quad):
            X, Y = _apply(got, u, v)
            assert abs(X - x) < 1e-3 and abs(Y - y) < 1e-3, (quad, (u, v), X, Y)
    # an integer axis-aligned rectangle: warp_rotated_box at angle 0, last row (0, 0, 1)
    for (x0, y0, bw, bh), (dw, dh) in (((30, 12, 200, 150), (112, 112)), ((0, 0, 322, 182), (70, 66)), ((-40, 7, 96, 33), (64, 64))):
        got = ts.perspective_from_quad([(x0, y0), (x0 + bw, y0), (x0 + bw, y0 + bh), (x0, y0 + bh)], dw, dh)
        want = ts.warp_rotated_box(x0 + bw / 2, y0 + bh / 2, bw, bh, 0.0, dw, dh) + (0.0, 0.0, 1.0)
        assert np.array_equal(u32(got), u32(want)), (got, want)
    # a parallelogram: h6 == h7 == +0 exactly
    got = ts.perspective_from_quad([(10, 20), (110, 45), (140, 145), (40, 120)], 64, 64)
    assert np.array_equal(u32(got[6:]), u32((0.0, 0.0, 1.0)))
    # eight plain numbers are accepted as well
    assert ts.perspective_from_quad([10, 20, 110, 45, 140, 145, 40, 120], 64, 64) == got
    # the error cases
    L = native.lib()
    out = native.Persp()
    q = (ctypes.c_double * 8)(10, 20, 110, 45, 140, 145, 40, 120)
    assert L.tsvpp_persp_from_quad(q, 64, 64, ctypes.byref(out)) == OK
    assert L.tsvpp_persp_from_quad(None, 64, 64, ctypes.byref(out)) == ERROR
    assert L.tsvpp_persp_from_quad(q, 64, 64, None) == ERROR
    assert L.tsvpp_persp_from_quad(q, 0, 64, ctypes.byref(out)) == ERROR
    assert L.tsvpp_persp_from_quad(q, 64, -1, ctypes.byref(out)) == ERROR
    for bad in (float("nan"), float("inf")):
        for k in range(8):
            qq = (ctypes.c_double * 8)(*q)
            qq[k] = bad
            assert L.tsvpp_persp_from_quad(qq, 64, 64, ctypes.byref(out)) == ERROR, (k, bad)
    # den == 0: corners 1, 2, 3 on one line, and no parallelogram
    assert L.tsvpp_persp_from_quad((ctypes.c_double * 8)(0, 0, 10, 0, 20, 10, 30, 20), 64, 64, ctypes.byref(out)) == ERROR
    assert P.from_quad([(0, 0), (10, 0), (20, 10), (30, 20)], 64, 64) is None


def test_from_opencv():
    import tensor_stream as ts
    M = [[0.8, -0.3, 12.25], [0.3, 0.8, -4.5], [0.0011, -0.0007, 1.25]]
    h = ts.perspective_from_opencv(M)
    (a, b, c), (d, e, f), (g, hh, k) = M
    for j, i in ((0, 0), (5, 9), (63, 17), (111, 111)):
        den = g * j + hh * i + k
        X, Y = _apply(h, j + 0.5, i + 0.5)
        assert abs(X - ((a * j + b * i + c) / den + 0.5)) < 1e-9 and abs(Y - ((d * j + e * i + f) / den + 0.5)) < 1e-9
    # last row (0, 0, 1): warp_from_opencv
    assert ts.perspective_from_opencv(M[:2] + [[0, 0, 1]]) == ts.warp_from_opencv(M[:2]) + (0.0, 0.0, 1.0)


# ---- 4. describe -----------------------------------------------------------------------------------------------------------------------------------------

def _footprint(native, h, w, hh, j0, j1, i0, i1, status=OK):
    out = (ctypes.c_int32 * 8)()
    assert native.lib().tsvpp_persp_footprint(ctypes.byref(_persp(native, h)), w, hh, j0, j1, i0, i1, out) == status
    return list(out)


def _chunks(span):
    return ((span + 14) >> 4) + 1


def _lds_need(f, luma_only=False):
    ny, nuv = f[3] - f[2] + 1, 0 if luma_only else f[7] - f[6] + 1
    return 16 * (ny * _chunks(f[1] - f[0] + 1) + nuv * _chunks(2 * (f[5] - f[4] + 1)))


def test_describe_line(native, monkeypatch):
    import torch
    import tensor_stream as ts
    from util import knob_run
    if knob_run():  # (replayed under A/B knobs: the selections are the knobs')
        return
    fp = ts.FrameParameters(width=112, height=112, resize_type=ts.ResizeType.BILINEAR, pixel_format=ts.FourCC.BGR24, planes_pos=ts.Planes.PLANAR, normalization=True)
    h = ts.perspective_from_quad([(800, 420), (1120, 450), (1100, 660), (820, 640)], 112, 112)
    for n, launches in ((32, 1), (33, 2)):
        d = ts.describe_perspective(fp, (1920, 1080, 2048), [h] * n)
        assert d["mode"] == "persp_bilinear" and d["out"] == "f32_planar" and d["dst"] == "112x112" and d["warps"] == n and d["frames"] == 1
        assert d["launches"] == launches and d["staged"] == n and d["limit"] == 32 and d["tiles"] == "4x4" and d["shape"] == "8x16"
        assert d["grid"] == 16 * min(n, 32) and d["kernel"] == "vpp_persp<O_F32_PLANAR,vec,staged,replicate>" and d["border"] == "replicate" and d["lds"] > 0
    d = ts.describe_perspective(fp, (1920, 1080, 2048), [h], border=(114, 128, 128), aligned_outputs=False)
    assert d["kernel"] == "vpp_persp<O_F32_PLANAR,elem,staged,border>" and d["border"] == "114,128,128"
    # one staged and one gathering output in a launch: a quad whose tiles tap more than the budget holds
    big = ts.perspective_from_quad([(100, 40), (1800, 60), (1820, 1040), (160, 1000)], 112, 112)
    d = ts.describe_perspective(fp, (1920, 1080, 2048), [h, big])
    assert d["staged"] == 1 and d["kernel"].endswith("staged,replicate>")
    # a scale-down by 10 (322 x 182 -> 30 x 34), as tsvpp_describe_warp: the first tile gathers, the tile of rows 32, 33 stages.  With no budget everything gathers
    small = ts.FrameParameters(width=30, height=34, resize_type=ts.ResizeType.BILINEAR, pixel_format=ts.FourCC.RGB24, planes_pos=ts.Planes.MERGED, normalization=False)
    so = P.affine(W.scale_only(322, 182, 30, 34))
    d = ts.describe_perspective(small, (322, 182, 384), [so])
    rest = _lds_need(_footprint(native, so, 322, 182, 0, 29, 32, 33))
    assert _lds_need(_footprint(native, so, 322, 182, 0, 29, 0, 31)) > 40 * 1024 > rest
    assert d["staged"] == 0 and d["lds"] == rest and d["kernel"] == "vpp_persp<O_U8_MERGED,elem,staged,replicate>"
    monkeypatch.setenv("TSVPP_LDS_KB", "0")
    for geo in ((322, 182, 384), (128, 72, 192)):
        d = ts.describe_perspective(small, geo, [P.affine(W.scale_only(geo[0], geo[1], 30, 34))])
        assert d["staged"] == 0 and d["lds"] == 0 and d["kernel"] == "vpp_persp<O_U8_MERGED,elem,gather,replicate>"
    monkeypatch.delenv("TSVPP_LDS_KB")
    # one tile of a keystone: lds= is the footprint function's box
    one = ts.FrameParameters(width=32, height=32, resize_type=ts.ResizeType.BILINEAR, pixel_format=ts.FourCC.BGR24, planes_pos=ts.Planes.PLANAR, normalization=True)
    key = ts.perspective_from_quad([(120, 40), (200, 44), (206, 120), (116, 116)], 32, 32)
    f = _footprint(native, key, 322, 182, 0, 31, 0, 31)
    d = ts.describe_perspective(one, (322, 182, 384), [key])
    assert d["lds"] == _lds_need(f) and d["staged"] == 1
    assert f[0] <= 117 and f[1] >= 205 and f[2] <= 41 and f[3] >= 119  # the box holds the quad's own bounding box
    y8 = ts.FrameParameters(width=32, height=32, resize_type=ts.ResizeType.BILINEAR, pixel_format=ts.FourCC.Y800, planes_pos=ts.Planes.MERGED, normalization=False)
    assert ts.describe_perspective(y8, (322, 182, 384), [key])["lds"] == _lds_need(f, luma_only=True)
    # the tensor form names its kernel and element
    d = ts.describe_perspective(fp, (1920, 1080, 2048), [h], border=(114, 128, 128), dtype=torch.float16, mean=0.0, std=1.0)
    assert d["kernel"] == "vpp_persp_tensor<PLANAR,EL_HALF,vec,staged,border>" and d["out"] == "f16_planar"


def test_affine_footprint_is_the_affine_calls(native):
    """for an affine h the interval box is exactly tsvpp_warp_footprint's (nw is the same everywhere: the four products are the numerators' extremes)"""
    rng = np.random.default_rng(504)
    w, h = 322, 182
    for _ in range(50):
        m = _seeded_affine(rng)
        for j0, j1, i0, i1 in ((0, 31, 0, 31), (38, 69, 32, 63), (64, 69, 64, 65)):
            out = (ctypes.c_int32 * 8)()
            assert native.lib().tsvpp_warp_footprint(ctypes.byref(native.Warp(0, (ctypes.c_float * 6)(*m))), w, h, j0, j1, i0, i1, out) == OK
            assert _footprint(native, P.affine(m), w, h, j0, j1, i0, i1) == list(out), m
            assert _footprint(native, tuple(4.0 * v for v in P.affine(m)), w, h, j0, j1, i0, i1) == list(out), m


# ---- 5. the footprint property ----------------------------------------------------------------------------------------------------------------------------

def test_every_tap_of_a_tile_lies_inside_the_host_footprint(native):
    """200 seeded quads -- the frame's inset corners, each moved by a jitter that grows by kind: mild keystone (10 px), strong keystone (40), partly outside
    (120), and the whole quad pushed outside the frame or thousands of pixels away (with 60) -- and every tile of a 70 x 66 output, the shifted last tile column
    of the vector-store kernels included: first and second tap of every pixel and of every chroma pair lie inside the box of tsvpp_persp_footprint (the second
    tap where its weight was not forced to zero at the low edge), and the box lies inside the frame.  Quads the request rules refuse (horizon through the output:
    non-convex or nearly so) are skipped and counted; the jitters are chosen so that at most 20 % are, by the model alone."""
    N = native
    rng = np.random.default_rng(78)
    w, h, dw, dh = 322, 182, 70, 66
    cols = [(0, 31), (32, 63), (64, 69), (38, 69)]
    rows = [(0, 31), (32, 63), (64, 65)]
    p = _params(N, dst=(dw, dh))
    fr = [N.NV12(None, None, 384, 384, w, h)]
    skipped = 0
    for k in range(200):
        kind = k % 4
        quad = _seeded_quads(rng, w, h, (10, 40, 120, 60)[kind])
        if kind == 3:
            quad = quad + (rng.choice([-1, 1]) * (w + 400), rng.choice([-1, 1]) * (h + 400)) if k % 8 == 3 else quad + (rng.choice([-1, 1]) * 5000, rng.choice([-1, 1]) * 7000)
        hm = P.from_quad(quad, dw, dh)
        ok = P.in_domain(hm, dw, dh)
        assert _describe(N, p, fr, [_persp(N, hm)])[0] == (OK if ok else UNSUPPORTED), (k, hm)
        if not ok:
            skipped += 1
            continue
        luma = P.taps(hm, w, h, np.arange(dh), np.arange(dw))
        chroma = P.taps(hm, w, h, np.arange(dh // 2), np.arange(dw // 2), chroma=True)
        for j0, j1 in cols:
            for i0, i1 in rows:
                f = _footprint(N, hm, w, h, j0, j1, i0, i1)
                assert 0 <= f[0] <= f[1] < w and 0 <= f[2] <= f[3] < h and 0 <= f[4] <= f[5] < w // 2 and 0 <= f[6] <= f[7] < h // 2, (k, hm, f)
                for grid, (a0, a1, b0, b1), box in ((luma, (j0, j1, i0, i1), f[:4]), (chroma, (j0 >> 1, j1 >> 1, i0 >> 1, i1 >> 1), f[4:])):
                    xa, xb, ya, yb = (t[b0:b1 + 1, a0:a1 + 1] for t in grid)
                    assert box[0] <= xa.min() and xb.max() <= box[1] and box[2] <= ya.min() and yb.max() <= box[3], (k, hm, (j0, j1, i0, i1), box)
    assert skipped <= 40, skipped
    # the debug export refuses a range the horizon crosses instead of computing a box from a reciprocal that means nothing
    _footprint(N, _with(6, -1 / 32), w, h, 0, 63, 0, 31, status=UNSUPPORTED)
    _footprint(N, _with(6, -1 / 32), w, h, 0, 15, 0, 31)
    assert N.lib().tsvpp_persp_footprint(None, w, h, 0, 31, 0, 31, (ctypes.c_int32 * 8)()) == ERROR
    assert N.lib().tsvpp_persp_footprint(ctypes.byref(_persp(N)), w, h, 8, 7, 0, 31, (ctypes.c_int32 * 8)()) == ERROR
