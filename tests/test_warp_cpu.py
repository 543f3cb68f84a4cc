"""CPU: tsvpp_convert_warp's host side and its reference model (tests/warp_util.py) -- the exactly rounded fma the model stands on, the model against the oracle
and against closed forms, the ABI (symbols, struct size, every status from tsvpp_describe_warp without a context), the matrix helpers, the describe line and the
footprint property: every tap of a tile lies inside the bounding box the host (and, from the same function, the kernel) computes for it."""
import ctypes
import math

import numpy as np
import pytest

import warp_util as W
from warp_util import BGR24, BILINEAR, MERGED, PLANAR, RGB24, Y800, F32
from util import synth_nv12

OK, UNSUPPORTED, ERROR = 0, -2, -3


@pytest.fixture(scope="module")
def native():
    from tensor_stream import _native
    _native.lib()
    return _native


# ---- 1. fma32 ------------------------------------------------------------------------------------------------------------------------------------------

def test_fma32_is_the_exactly_rounded_fused_multiply_add():
    rng = np.random.default_rng(11)
    n = 100000
    # magnitudes as the contract's operands have them (indices, ratios, translations, pixel values, weights), with cancellation: c near -a * b in a quarter
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(F32)
    b = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(F32)
    c = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(F32)
    near = rng.random(n) < 0.25
    c[near] = (-(a[near].astype(np.float64) * b[near].astype(np.float64)) * (1 + rng.standard_normal(near.sum()) * 1e-6)).astype(F32)
    got = W.fma32(a, b, c)
    want = np.array([W.fma_fraction(a[k], b[k], c[k]) for k in range(n)], F32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_fma32_where_the_double_sum_is_a_tie_and_the_exact_value_is_not():
    """constructed triples: a * b lies exactly midway between two float32 neighbours (it fits float64), and c is so small that the float64 sum drops it and sits
    ON the tie -- which a plain second rounding would send to the even neighbour for either sign of c, while the exact value lies to one side"""
    from fractions import Fraction
    triples = []
    for k in (12, 10, 7):
        x = F32(1 + 2.0 ** -k)                     # x * x = 1 + 2^(1-k) + 2^(-2k): for k = 12 the last term is half an ulp of float32 at 1
        y = F32(1 + 2.0 ** -(24 - k))              # x * y = 1 + 2^-k + 2^-(24-k) + 2^-24: the last term is half an ulp for every k
        for c in (2.0 ** -60, -(2.0 ** -60), 2.0 ** -80, -(2.0 ** -100), 0.0):
            triples.append((x, y, F32(c)))
    sides = set()
    for x, y, c in triples:
        prod = Fraction(float(x)) * Fraction(float(y))
        lo = np.nextafter(W.round_fraction_f32(prod), F32(0))
        assert any(prod == (Fraction(float(t)) + Fraction(float(np.nextafter(t, F32(2))))) / 2 for t in (lo, np.nextafter(lo, F32(2)))), "not a tie"
        assert float(x) * float(y) + float(c) == float(x) * float(y), "the float64 sum keeps the addend: not the case this test is about"
        got, want = W.fma32(x, y, c), W.fma_fraction(x, y, c)
        assert got.view(np.uint32) == want.view(np.uint32), (x, y, c, got, want)
        if c != 0:
            sides.add((float(x), float(y), bool(c > 0), float(got)))
    # for every product the two signs of the addend gave different results
    for x, y, _ in triples:
        assert len({r for (a, b, _, r) in sides if (a, b) == (float(x), float(y))}) == 2


# ---- 2. the model against the oracle ---------------------------------------------------------------------------------------------------------------------

SCALE_CASES = [((128, 72, 192), [(64, 64), (70, 66), (30, 34), (200, 100)]), ((322, 182, 384), [(64, 64), (112, 112), (640, 360)]), ((72, 128, 96), [(96, 64)])]


@pytest.mark.parametrize("border", [None, (114, 128, 128)])
def test_scale_only_model_is_the_oracles_bilinear_resize(oracle, border):
    """with a scale-only matrix the coordinate expressions reduce to the BILINEAR coordinate and no position lies outside the frame: the virtual frame is the
    oracle's resize stage, byte for byte, under both border modes"""
    for k, ((w, h, pitch), dsts) in enumerate(SCALE_CASES):
        y, uv = synth_nv12(w, h, seed=40 + k, pitch=pitch)
        for dw, dh in dsts:
            Y, UV = W.virtual_frame(y, uv, w, h, W.scale_only(w, h, dw, dh), dw, dh, border)
            ry, ruv = oracle.resize_stage(y, uv, dw, dh, BILINEAR, width=w)
            assert np.array_equal(Y, ry) and np.array_equal(UV, ruv), (w, h, dw, dh, border)


# ---- 3. closed forms -------------------------------------------------------------------------------------------------------------------------------------

def test_transpose_and_mirror_need_no_blend():
    w, h = 64, 48
    y, uv = synth_nv12(w, h, seed=5, pitch=80)
    # transpose: X = v, Y = u -- pixel centres map to pixel centres, every weight is zero
    Y, UV = W.virtual_frame(y, uv, w, h, (0, 1, 0, 1, 0, 0), h, w)
    assert np.array_equal(Y, y[:h, :w].T)
    pairs = uv[:h // 2, :w].reshape(h // 2, w // 2, 2)
    assert np.array_equal(UV.reshape(w // 2, h // 2, 2), pairs.transpose(1, 0, 2))
    # mirror in x: X = w - u
    for border in (None, (1, 2, 3)):
        Y, UV = W.virtual_frame(y, uv, w, h, (-1, 0, w, 0, 1, 0), w, h, border)
        assert np.array_equal(Y, y[:h, :w][:, ::-1])
        assert np.array_equal(UV.reshape(h // 2, w // 2, 2), pairs[:, ::-1, :])


# ---- 4. ABI and statuses ---------------------------------------------------------------------------------------------------------------------------------

def _params(native, dst=(64, 64), rt=BILINEAR, fcc=RGB24, planes=MERGED, norm=0, crop=(0, 0, 0, 0)):
    return native.Params(crop[0], crop[1], crop[2], crop[3], dst[0], dst[1], rt, fcc, planes, norm)


def _warp(native, m=(2, 0, 0, 0, 1.125, 0), frame=0):
    return native.Warp(frame, (ctypes.c_float * 6)(*m))


def _describe(native, p, frames, warps, border=(-1, -1, -1), spec=None, n_frames=None, n_warps=None, aligned=1):
    L = native.lib()
    buf = ctypes.create_string_buffer(512)
    fr = (native.NV12 * max(len(frames), 1))(*frames) if frames is not None else None
    ws = (native.Warp * max(len(warps), 1))(*warps) if warps is not None else None
    nf = len(frames) if n_frames is None else n_frames
    nw = len(warps) if n_warps is None else n_warps
    pp = ctypes.byref(p) if p is not None else None
    if spec is None:
        sts = L.tsvpp_describe_warp(pp, nf, fr, nw, ws, border[0], border[1], border[2], aligned, buf, len(buf))
    else:
        sp = ctypes.byref(spec) if spec != "null" else None
        sts = L.tsvpp_describe_warp_tensor(pp, sp, nf, fr, nw, ws, border[0], border[1], border[2], aligned, buf, len(buf))
    return sts, buf.value.decode()


def test_symbols_and_struct_size(native):
    assert ctypes.sizeof(native.Warp) == 28
    assert native.TSVPP_MAX_WARPS == 32
    L = native.lib()
    for s in ("tsvpp_convert_warp", "tsvpp_describe_warp", "tsvpp_convert_warp_tensor", "tsvpp_describe_warp_tensor", "tsvpp_warp_rotated_box", "tsvpp_warp_footprint"):
        assert s in native.SYMBOLS
        getattr(L, s)


def test_statuses_in_their_order_without_a_context(native):
    N = native
    fr = [N.NV12(None, None, 192, 192, 128, 72)]
    ws = [_warp(N)]
    p = _params(N)
    assert _describe(N, p, fr, ws)[0] == OK
    # TSVPP_ERROR
    assert _describe(N, None, fr, ws)[0] == ERROR
    assert _describe(N, p, None, ws, n_frames=1)[0] == ERROR
    assert _describe(N, p, fr, None, n_warps=1)[0] == ERROR
    assert N.lib().tsvpp_describe_warp(ctypes.byref(p), 1, (N.NV12 * 1)(*fr), 1, (N.Warp * 1)(*ws), -1, -1, -1, 1, None, 0) == ERROR
    assert _describe(N, p, fr, ws, n_frames=0)[0] == ERROR
    assert _describe(N, p, fr, ws, n_warps=0)[0] == ERROR
    assert _describe(N, p, [N.NV12(None, None, 192, 192, 0, 72)], ws)[0] == ERROR
    assert _describe(N, p, [N.NV12(None, None, 100, 192, 128, 72)], ws)[0] == ERROR
    assert _describe(N, p, [N.NV12(None, None, 192, 100, 128, 72)], ws)[0] == ERROR
    assert _describe(N, p, fr, [_warp(N, frame=1)])[0] == ERROR
    assert _describe(N, p, fr, [_warp(N, frame=-1)])[0] == ERROR
    assert _describe(N, _params(N, dst=(0, 64)), fr, ws)[0] == ERROR
    assert _describe(N, _params(N, dst=(64, -2)), fr, ws)[0] == ERROR
    assert _describe(N, _params(N, crop=(0, 0, 32, 32)), fr, ws)[0] == ERROR
    for border in ((256, 128, 128), (-2, -2, -2), (-1, 128, 128), (114, -1, 128), (114, 128, -1), (0, 0, 300)):
        assert _describe(N, p, fr, ws, border=border)[0] == ERROR, border
    for bad in (float("nan"), float("inf"), -float("inf")):
        for k in range(6):
            m = [2, 0, 0, 0, 1.125, 0]
            m[k] = bad
            assert _describe(N, p, fr, [_warp(N, m)])[0] == ERROR, (k, bad)
    # TSVPP_UNSUPPORTED
    assert _describe(N, _params(N, dst=(63, 64)), fr, ws)[0] == UNSUPPORTED
    assert _describe(N, _params(N, dst=(64, 33)), fr, ws)[0] == UNSUPPORTED
    assert _describe(N, p, [N.NV12(None, None, 192, 192, 127, 72)], ws)[0] == UNSUPPORTED
    assert _describe(N, p, [N.NV12(None, None, 192, 192, 128, 71)], ws)[0] == UNSUPPORTED
    for rt in (0, 2, 3, 7):  # NEAREST, BICUBIC, AREA, unknown
        assert _describe(N, _params(N, rt=rt), fr, ws)[0] == UNSUPPORTED, rt
    for fcc in (3, 4, 5, 6):  # NV12, UYVY, YUV444, HSV in the header's numbering, whichever they are: none is in the list
        if fcc not in (Y800, RGB24, BGR24):
            assert _describe(N, _params(N, fcc=fcc), fr, ws)[0] == UNSUPPORTED, fcc
    for k in range(6):
        m = [2, 0, 0, 0, 1.125, 0]
        m[k] = -(2.0 ** 24) - 2
        assert _describe(N, p, fr, [_warp(N, m)])[0] == UNSUPPORTED, k
        m[k] = 2.0 ** 24
        assert _describe(N, p, fr, [_warp(N, m)])[0] == OK, k
    assert _describe(N, _params(N, dst=(32768, 32768), norm=1), fr, ws)[0] == UNSUPPORTED  # 12 GiB
    # an ERROR condition wins over an UNSUPPORTED one
    assert _describe(N, _params(N, dst=(63, 64), rt=3), fr, ws, border=(256, 0, 0))[0] == ERROR
    assert _describe(N, _params(N, rt=2), fr, [_warp(N, (float("nan"), 0, 0, 0, 1, 0))])[0] == ERROR


def test_tensor_describe_adds_the_spec_rules_behind_the_request(native):
    N = native
    fr = [N.NV12(None, None, 192, 192, 128, 72)]
    ws = [_warp(N)]
    spec = N.TensorSpec(N.TSVPP_F16, (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1))
    ok = _params(N, fcc=BGR24, planes=PLANAR, norm=1)
    sts, line = _describe(N, ok, fr, ws, spec=spec, border=(114, 128, 128))
    assert sts == OK and "kernel=vpp_warp_tensor<PLANAR,EL_HALF,vec," in line and "out=f16_planar" in line and line.endswith("border=114,128,128")
    # rule 1 first: the request's own status
    assert _describe(N, _params(N, fcc=BGR24, planes=PLANAR, norm=1, rt=2), fr, ws, spec="null")[0] == UNSUPPORTED
    assert _describe(N, ok, fr, [_warp(N, frame=3)], spec=N.TensorSpec(9, (ctypes.c_float * 3)(), (ctypes.c_float * 3)(1, 1, 1)))[0] == ERROR
    # rule 2
    assert _describe(N, ok, fr, ws, spec="null")[0] == ERROR
    assert _describe(N, ok, fr, ws, spec=N.TensorSpec(N.TSVPP_F16, (ctypes.c_float * 3)(0, float("nan"), 0), (ctypes.c_float * 3)(1, 1, 1)))[0] == ERROR
    assert _describe(N, ok, fr, ws, spec=N.TensorSpec(N.TSVPP_F16, (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 0, 1)))[0] == ERROR
    # rule 3
    assert _describe(N, ok, fr, ws, spec=N.TensorSpec(9, (ctypes.c_float * 3)(), (ctypes.c_float * 3)(1, 1, 1)))[0] == UNSUPPORTED
    assert _describe(N, _params(N, fcc=BGR24, planes=PLANAR, norm=0), fr, ws, spec=spec)[0] == UNSUPPORTED
    assert _describe(N, _params(N, fcc=BGR24, planes=MERGED, norm=1), fr, ws, spec=spec)[0] == UNSUPPORTED
    assert _describe(N, _params(N, fcc=Y800, planes=MERGED, norm=1), fr, ws, spec=spec)[0] == OK


# ---- 5. the matrix helpers --------------------------------------------------------------------------------------------------------------------------------

def test_rotated_box_and_opencv_conversion(native):
    import tensor_stream as ts
    for (w, h), (dw, dh) in (((1920, 1080), (112, 112)), ((322, 182), (70, 66)), ((128, 72), (200, 100))):
        m = ts.warp_rotated_box(w / 2, h / 2, w, h, 0.0, dw, dh)
        want = W.scale_only(w, h, dw, dh)
        assert np.array_equal(np.array(m, F32).view(np.uint32), np.array(want, F32).view(np.uint32)), (m, want)
    # a quarter turn: the box's corners land on the output's corners.  Box 300 x 200 centred at (500, 400): local corner (-150, -100) rotated by +pi / 2
    # (x towards y) is (100, -150)
    cx, cy, bw, bh, dw, dh = 500.0, 400.0, 300.0, 200.0, 96, 64
    m = ts.warp_rotated_box(cx, cy, bw, bh, math.pi / 2, dw, dh)
    for (u, v), (lx, ly) in (((0, 0), (-150, -100)), ((dw, 0), (150, -100)), ((0, dh), (-150, 100)), ((dw, dh), (150, 100))):
        X, Y = m[0] * u + m[1] * v + m[2], m[3] * u + m[4] * v + m[5]
        assert abs(X - (cx - ly)) < 1e-4 and abs(Y - (cy + lx)) < 1e-4, ((u, v), X, Y)
    # ... and at 30 degrees against the formula of the header, evaluated here in double
    a = math.radians(30)
    m = ts.warp_rotated_box(cx, cy, bw, bh, a, dw, dh)
    c, s = math.cos(a), math.sin(a)
    want = (bw * c / dw, -bh * s / dh, cx - 0.5 * bw * c + 0.5 * bh * s, bw * s / dw, bh * c / dh, cy - 0.5 * bw * s - 0.5 * bh * c)
    assert np.array_equal(np.array(m, F32), np.array(want, F32))
    out = native.Warp()
    L = native.lib()
    assert L.tsvpp_warp_rotated_box(0.0, 0.0, 10.0, 10.0, 0.0, 8, 8, None) == ERROR
    assert L.tsvpp_warp_rotated_box(0.0, 0.0, 0.0, 10.0, 0.0, 8, 8, ctypes.byref(out)) == ERROR
    assert L.tsvpp_warp_rotated_box(0.0, 0.0, 10.0, 10.0, float("nan"), 8, 8, ctypes.byref(out)) == ERROR
    assert L.tsvpp_warp_rotated_box(0.0, 0.0, 10.0, 10.0, 0.0, 0, 8, ctypes.byref(out)) == ERROR
    # OpenCV's index-based inverse matrix: source index = M (output index); this library: source position = m (output centre), position = index + 0.5
    M = [[0.8, -0.3, 12.25], [0.3, 0.8, -4.5]]
    m = ts.warp_from_opencv(M)
    (a_, b_, c_), (d_, e_, f_) = M
    assert m == (a_, b_, c_ + 0.5 - 0.5 * (a_ + b_), d_, e_, f_ + 0.5 - 0.5 * (d_ + e_))
    for j, i in ((0, 0), (5, 9), (63, 17)):
        assert abs((m[0] * (j + 0.5) + m[1] * (i + 0.5) + m[2]) - (a_ * j + b_ * i + c_ + 0.5)) < 1e-9
        assert abs((m[3] * (j + 0.5) + m[4] * (i + 0.5) + m[5]) - (d_ * j + e_ * i + f_ + 0.5)) < 1e-9


# ---- 6. describe -----------------------------------------------------------------------------------------------------------------------------------------

def _footprint(native, m, w, h, j0, j1, i0, i1):
    out = (ctypes.c_int32 * 8)()
    assert native.lib().tsvpp_warp_footprint(ctypes.byref(_warp(native, m)), w, h, j0, j1, i0, i1, out) == OK
    return list(out)


def _chunks(span):
    return ((span + 14) >> 4) + 1


def _lds_need(f, luma_only=False):
    ny, nuv = f[3] - f[2] + 1, 0 if luma_only else f[7] - f[6] + 1
    return 16 * (ny * _chunks(f[1] - f[0] + 1) + nuv * _chunks(2 * (f[5] - f[4] + 1)))


def test_describe_line(native, monkeypatch):
    import tensor_stream as ts
    from util import knob_run
    if knob_run():  # (replayed under A/B knobs: the selections are the knobs')
        return
    fp = ts.FrameParameters(width=112, height=112, resize_type=ts.ResizeType.BILINEAR, pixel_format=ts.FourCC.BGR24, planes_pos=ts.Planes.PLANAR, normalization=True)
    m = ts.warp_rotated_box(960, 540, 300, 240, 0.5, 112, 112)
    for n, launches in ((32, 1), (33, 2)):
        d = ts.describe_warp(fp, (1920, 1080, 2048), [m] * n)
        assert d["mode"] == "warp_bilinear" and d["out"] == "f32_planar" and d["dst"] == "112x112" and d["warps"] == n and d["frames"] == 1
        assert d["launches"] == launches and d["staged"] == n and d["limit"] == 32 and d["tiles"] == "4x4" and d["shape"] == "8x16"
        assert d["grid"] == 16 * min(n, 32) and d["kernel"] == "vpp_warp<O_F32_PLANAR,vec,staged,replicate>" and d["border"] == "replicate" and d["lds"] > 0
    d = ts.describe_warp(fp, (1920, 1080, 2048), [m], border=(114, 128, 128), aligned_outputs=False)
    assert d["kernel"] == "vpp_warp<O_F32_PLANAR,elem,staged,border>" and d["border"] == "114,128,128"
    # one staged and one gathering warp in a launch: a box whose tiles tap more than the budget holds (1600 x 1000 -> 112 x 112: a tile's box is ~460 x 290)
    big = ts.warp_rotated_box(960, 540, 1600, 1000, 0.0, 112, 112)
    d = ts.describe_warp(fp, (1920, 1080, 2048), [m, big])
    assert d["staged"] == 1 and d["kernel"].endswith("staged,replicate>")
    # a scale-down by 10 (322 x 182 -> 30 x 34): the tile of rows 0 .. 31 taps nearly the whole frame, ~80 KB, and gathers under the default budget; the tile of
    # rows 32, 33 stages its few rows -- a launch mixes the two, the warp does not count as staged.  A scale-down by 4 stages both tiles.  With no LDS budget
    # everything gathers
    small = ts.FrameParameters(width=30, height=34, resize_type=ts.ResizeType.BILINEAR, pixel_format=ts.FourCC.RGB24, planes_pos=ts.Planes.MERGED, normalization=False)
    d = ts.describe_warp(small, (322, 182, 384), [W.scale_only(322, 182, 30, 34)])
    rest = _lds_need(_footprint(native, W.scale_only(322, 182, 30, 34), 322, 182, 0, 29, 32, 33))
    assert _lds_need(_footprint(native, W.scale_only(322, 182, 30, 34), 322, 182, 0, 29, 0, 31)) > 40 * 1024 > rest
    assert d["staged"] == 0 and d["lds"] == rest and d["kernel"] == "vpp_warp<O_U8_MERGED,elem,staged,replicate>"  # (4 k + 2 columns, narrower than a tile: element-wise)
    d = ts.describe_warp(small, (128, 72, 192), [W.scale_only(128, 72, 30, 34)])
    assert d["staged"] == 1 and d["lds"] == _lds_need(_footprint(native, W.scale_only(128, 72, 30, 34), 128, 72, 0, 29, 0, 31)) and d["kernel"] == "vpp_warp<O_U8_MERGED,elem,staged,replicate>"
    monkeypatch.setenv("TSVPP_LDS_KB", "0")
    for geo in ((322, 182, 384), (128, 72, 192)):
        d = ts.describe_warp(small, geo, [W.scale_only(geo[0], geo[1], 30, 34)])
        assert d["staged"] == 0 and d["lds"] == 0 and d["kernel"] == "vpp_warp<O_U8_MERGED,elem,gather,replicate>"
    monkeypatch.delenv("TSVPP_LDS_KB")
    # one tile of a 45 degree warp: lds= is the footprint function's box
    one = ts.FrameParameters(width=32, height=32, resize_type=ts.ResizeType.BILINEAR, pixel_format=ts.FourCC.BGR24, planes_pos=ts.Planes.PLANAR, normalization=True)
    m45 = ts.warp_rotated_box(160, 90, 80, 80, math.pi / 4, 32, 32)
    f = _footprint(native, m45, 322, 182, 0, 31, 0, 31)
    d = ts.describe_warp(one, (322, 182, 384), [m45])
    assert d["lds"] == _lds_need(f) and d["staged"] == 1
    # the box is the rotated square's bounding box: 80 sqrt(2) = 113 pixels and the taps' +1, not the 80 of the unrotated square
    assert 112 <= f[1] - f[0] + 1 <= 116 and 112 <= f[3] - f[2] + 1 <= 116
    y8 = ts.FrameParameters(width=32, height=32, resize_type=ts.ResizeType.BILINEAR, pixel_format=ts.FourCC.Y800, planes_pos=ts.Planes.MERGED, normalization=False)
    assert ts.describe_warp(y8, (322, 182, 384), [m45])["lds"] == _lds_need(f, luma_only=True)


# ---- 7. the footprint property -----------------------------------------------------------------------------------------------------------------------------

def test_every_tap_of_a_tile_lies_inside_the_host_footprint(native):
    """200 seeded matrices -- scales 0.3 .. 5, any angle, shear, translations that push the box partly or wholly outside -- and every tile of a 70 x 66 output,
    the shifted last tile column of the vector-store kernels included: first and second tap of every pixel and of every chroma pair lie inside the box of
    tsvpp_warp_footprint (the second tap where its weight was not forced to zero at the low edge: there it is multiplied by that zero and never fetched), and
    the box lies inside the frame"""
    rng = np.random.default_rng(77)
    w, h, dw, dh = 322, 182, 70, 66
    cols = [(0, 31), (32, 63), (64, 69), (38, 69)]
    rows = [(0, 31), (32, 63), (64, 65)]
    for k in range(200):
        sx, sy = rng.uniform(0.3, 5.0, 2)
        ang, shear = rng.uniform(0, 2 * math.pi), rng.uniform(-0.5, 0.5)
        c, s = math.cos(ang), math.sin(ang)
        a, b, d, e = sx * c, -sy * s + shear * sx * c, sx * s, sy * c + shear * sx * s
        kind = k % 4  # centred; partly outside; wholly outside, near; thousands of pixels away
        cx = w / 2 + (0, rng.uniform(-w, w), rng.choice([-1, 1]) * (w + 400), rng.choice([-1, 1]) * 5000)[kind]
        cy = h / 2 + (0, rng.uniform(-h, h), rng.choice([-1, 1]) * (h + 400), rng.choice([-1, 1]) * 7000)[kind]
        m = tuple(float(F32(v)) for v in (a, b, cx - a * dw / 2 - b * dh / 2, d, e, cy - d * dw / 2 - e * dh / 2))
        luma = W.taps(m, w, h, np.arange(dh), np.arange(dw))
        chroma = W.taps(m, w, h, np.arange(dh // 2), np.arange(dw // 2), chroma=True)
        for j0, j1 in cols:
            for i0, i1 in rows:
                f = _footprint(native, m, w, h, j0, j1, i0, i1)
                assert 0 <= f[0] <= f[1] < w and 0 <= f[2] <= f[3] < h and 0 <= f[4] <= f[5] < w // 2 and 0 <= f[6] <= f[7] < h // 2, (k, m, f)
                for grid, (a0, a1, b0, b1), box in ((luma, (j0, j1, i0, i1), f[:4]), (chroma, (j0 >> 1, j1 >> 1, i0 >> 1, i1 >> 1), f[4:])):
                    xa, xb, ya, yb = (t[b0:b1 + 1, a0:a1 + 1] for t in grid)
                    assert box[0] <= xa.min() and xb.max() <= box[1] and box[2] <= ya.min() and yb.max() <= box[3], (k, m, (j0, j1, i0, i1), box)
