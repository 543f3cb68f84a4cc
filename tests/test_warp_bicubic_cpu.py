"""CPU: tsvpp_convert_warp_bicubic / tsvpp_convert_perspective_bicubic -- the host side and the reference model (tests/warp_bicubic_util.py): the contract's
identities against the existing oracle, the model inside the bracket of its independent float64 judge (tests/sampler64_cubic.py) with the mutations that judge
must reject, the footprint property on the DEBUG exports, the describe lines and every status in its order -- the existing calls still refusing BICUBIC."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import persp_util as P
import sampler64 as S
import sampler64_cubic as C
import warp_bicubic_util as B
import warp_util as W
from warp_util import BGR24, MERGED, PLANAR, RGB24, Y800
from util import knob_run, synth_nv12

OK, UNSUPPORTED, ERROR = 0, -2, -3
NEAREST, BILINEAR, BICUBIC, AREA = 0, 1, 2, 3
FRAMES, DSTS = C.FRAMES, C.DSTS  # 322 x 182 (pitch 384), 32 x 18 (pitch 48), 4 x 2; 70 x 66, 30 x 34, 112 x 112


@pytest.fixture(scope="module")
def native():
    from tensor_stream import _native
    _native.lib()
    return _native


# ---- 1. the identities against the existing oracle ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("border", [None, (114, 128, 128)])
def test_scale_only_model_is_the_oracles_bicubic_resize(oracle, border):
    """with the scale-only matrix the coordinate reduces to fmaf(j + 0.5f, ratio, -0.5f) and no position lies outside the frame: the virtual frame is the oracle's
    BICUBIC resize stage byte for byte, as a matrix and as a homography with last row (0, 0, 1), under both border modes.  At 4 x 2 every upper tap collapses"""
    for k, (w, h, pitch) in enumerate(FRAMES):
        y, uv = synth_nv12(w, h, seed=60 + k, pitch=pitch)
        for dw, dh in DSTS:
            m = W.scale_only(w, h, dw, dh)
            ry, ruv = oracle.resize_stage(y, uv, dw, dh, BICUBIC, width=w)
            for c in (m, P.affine(m)):
                Y, UV = B.virtual_frame(y, uv, w, h, c, dw, dh, border)
                assert np.array_equal(Y, ry) and np.array_equal(UV, ruv), (w, h, dw, dh, border, len(c))


def test_even_translation_is_the_colour_conversion_of_the_crop(oracle):
    """(1, 0, tx, 0, 1, ty) with even tx, ty inside the frame: every weight is zero, the coefficients are 0, 1, 0, 0 and the output is the oracle's plain colour
    conversion of that crop, whatever the edge rule does to the other taps.  Every output size that fits the frame, and the whole frame itself"""
    for k, (w, h, pitch) in enumerate(FRAMES):
        y, uv = synth_nv12(w, h, seed=70 + k, pitch=pitch)
        for dw, dh in DSTS + [(w, h)]:
            if dw > w or dh > h:
                continue
            for tx, ty in {(0, 0), (w - dw, h - dh), (2 * ((w - dw) // 4), 2 * ((h - dh) // 4))}:
                crop_y = np.ascontiguousarray(y[ty:ty + dh, tx:tx + dw])
                crop_uv = np.ascontiguousarray(uv[ty // 2:(ty + dh) // 2, tx:tx + dw])
                for fcc, planes, norm in ((BGR24, PLANAR, True), (RGB24, MERGED, False), (Y800, MERGED, False)):
                    ref = oracle.convert(crop_y, crop_uv, fourcc=fcc, planes=planes, normalization=norm)[0].ravel().view(np.uint8)
                    for c in ((1, 0, tx, 0, 1, ty), P.affine((1, 0, tx, 0, 1, ty))):
                        for border in (None, (3, 250, 7)):
                            got = B.expected(oracle, y, uv, w, h, c, (dw, dh), fcc, planes, norm, border)
                            assert np.array_equal(got, ref), (w, h, dw, dh, tx, ty, fcc, border, len(c))


def test_a_homography_and_four_times_it_give_the_same_model_bits():
    import coord_paths as cp
    w, h, pitch = FRAMES[0]
    y, uv = synth_nv12(w, h, seed=81, pitch=pitch)
    hs = cp.homographies(w, h, 70, 66)
    for name in ("mild", "strong", "left"):
        a = B.virtual_frame(y, uv, w, h, hs[name], 70, 66, (3, 250, 7))
        b = B.virtual_frame(y, uv, w, h, tuple(4.0 * v for v in hs[name]), 70, 66, (3, 250, 7))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), name


# ---- 2. the judge ------------------------------------------------------------------------------------------------------------------------------------------

def _mutant(**replace):
    """a copy of the model with some of its pieces replaced"""
    spec = importlib.util.spec_from_file_location("warp_bicubic_util_mutant", os.path.join(os.path.dirname(os.path.abspath(__file__)), "warp_bicubic_util.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    for k, v in replace.items():
        setattr(m, k, v(getattr(m, k)) if callable(v) and k != "A" else v)
    return m


MUTANTS = {
    "c0 and c3 swapped": dict(coeffs=lambda f: (lambda w: (lambda c: (c[3], c[1], c[2], c[0]))(f(w)))),
    "a = -0.5": dict(A=-0.5),
    "the edge collapse dropped (every tap clamped on its own)": dict(
        tap_indices=lambda f: (lambda p, limit: (np.maximum(p - 1, 0), p, np.minimum(p + 1, limit - 1), np.minimum(p + 2, limit - 1)))),
    "the row rounding dropped": dict(row_round=lambda f: (lambda s: s)),
}


def test_model_lies_inside_the_float64_bracket_and_every_mutant_leaves_it():
    """the committed case set (FRAMES x DSTS x sampler64's affine and perspective items x replicate and a border): no sample of the model outside its bracket, none
    left out; the bracket is not vacuous -- most samples are single-valued and each mutation of the model puts samples outside"""
    mutants = {name: _mutant(**r) for name, r in MUTANTS.items()}
    outside = {name: 0 for name in mutants}
    two = size = n_cases = 0
    for k, (w, h, pitch), dst, name, c in C.cases():
        y, uv = S.smooth_nv12(w, h, 900 + k, pitch)
        grids = C.positions(c, *dst)
        for border in C.BORDERS:
            vb = C.virtual_bracket(y, uv, w, h, grids, border)
            two, size, n_cases = two + sum(vb.two), size + sum(vb.size), n_cases + 1
            Y, UV = B.virtual_frame(y, uv, w, h, c, dst[0], dst[1], border)
            assert S.holds(vb, Y, UV) == 0, ((w, h), dst, name, border)
            for mname, m in mutants.items():
                outside[mname] += S.holds(vb, *m.virtual_frame(y, uv, w, h, c, dst[0], dst[1], border))
    print(f"cases={n_cases} samples={size} two-valued={two} ({100.0 * two / size:.2f} %) mutants outside: {outside}")
    assert n_cases == 3 * 3 * 9 * 2 and two < 0.05 * size
    for mname, n in outside.items():
        assert n > 0, f"the judge accepts the model with {mname}"


# ---- 3. ABI, describe and statuses ---------------------------------------------------------------------------------------------------------------------------

def _params(native, dst=(64, 64), rt=BICUBIC, fcc=RGB24, planes=MERGED, norm=0, crop=(0, 0, 0, 0)):
    return native.Params(crop[0], crop[1], crop[2], crop[3], dst[0], dst[1], rt, fcc, planes, norm)


M0 = (2, 0, 0, 0, 1.125, 0)
H0 = M0 + (0, 0, 1)


def _rec(native, c, frame=0):
    return native.Warp(frame, (ctypes.c_float * 6)(*c)) if len(c) == 6 else native.Persp(frame, (ctypes.c_float * 9)(*c))


def _describe(native, kind, p, frames, recs, border=(-1, -1, -1), spec=None, n_frames=None, n=None, aligned=1, buf_len=512):
    """tsvpp_describe_warp_bicubic (kind "warp") / tsvpp_describe_perspective_bicubic ("perspective"); recs: records, or None for a null array"""
    L = native.lib()
    T = native.Warp if kind == "warp" else native.Persp
    buf = ctypes.create_string_buffer(512)
    fr = (native.NV12 * max(len(frames), 1))(*frames) if frames is not None else None
    rs = (T * max(len(recs), 1))(*recs) if recs is not None else None
    nf = len(frames) if n_frames is None else n_frames
    nr = len(recs) if n is None else n
    sts = getattr(L, f"tsvpp_describe_{kind}_bicubic")(ctypes.byref(p) if p is not None else None, ctypes.byref(spec) if spec is not None else None, nf, fr, nr, rs,
                                                      border[0], border[1], border[2], aligned, buf if buf_len else None, buf_len)
    return sts, buf.value.decode()


def test_symbols(native):
    L = native.lib()
    for s in ("tsvpp_convert_warp_bicubic", "tsvpp_describe_warp_bicubic", "tsvpp_warp_bicubic_footprint", "tsvpp_convert_perspective_bicubic",
              "tsvpp_describe_perspective_bicubic", "tsvpp_persp_bicubic_footprint"):
        assert s in native.SYMBOLS
        getattr(L, s)
    assert ctypes.sizeof(native.Warp) == 28 and ctypes.sizeof(native.Persp) == 40 and native.TSVPP_MAX_WARPS == 32 and native.TSVPP_MAX_PERSP == 32


@pytest.mark.parametrize("kind,c0", [("warp", M0), ("perspective", H0)])
def test_statuses_in_their_order_without_a_context(native, kind, c0):
    """every refusal of the BILINEAR call, in its order, with `a resize type other than BICUBIC`"""
    N = native
    fr = [N.NV12(None, None, 192, 192, 128, 72)]
    rs = [_rec(N, c0)]
    p = _params(N)

    def d(p=p, fr=fr, rs=rs, **kw):
        return _describe(N, kind, p, fr, rs, **kw)[0]
    assert d() == OK
    # TSVPP_ERROR
    assert d(p=None) == ERROR and d(fr=None, n_frames=1) == ERROR and d(rs=None, n=1) == ERROR and d(buf_len=0) == ERROR
    assert d(n_frames=0) == ERROR and d(n=0) == ERROR
    for bad in (N.NV12(None, None, 192, 192, 0, 72), N.NV12(None, None, 100, 192, 128, 72), N.NV12(None, None, 192, 100, 128, 72)):
        assert d(fr=[bad]) == ERROR
    assert d(rs=[_rec(N, c0, frame=1)]) == ERROR and d(rs=[_rec(N, c0, frame=-1)]) == ERROR
    assert d(p=_params(N, dst=(0, 64))) == ERROR and d(p=_params(N, dst=(64, -2))) == ERROR and d(p=_params(N, crop=(0, 0, 32, 32))) == ERROR
    for border in ((256, 128, 128), (-2, -2, -2), (-1, 128, 128), (114, -1, 128), (114, 128, -1), (0, 0, 300)):
        assert d(border=border) == ERROR, border
    for bad in (float("nan"), float("inf"), -float("inf")):
        for k in range(len(c0)):
            c = list(c0)
            c[k] = bad
            assert d(rs=[_rec(N, c)]) == ERROR, (k, bad)
    # TSVPP_UNSUPPORTED
    assert d(p=_params(N, dst=(63, 64))) == UNSUPPORTED and d(p=_params(N, dst=(64, 33))) == UNSUPPORTED
    assert d(fr=[N.NV12(None, None, 192, 192, 127, 72)]) == UNSUPPORTED and d(fr=[N.NV12(None, None, 192, 192, 128, 71)]) == UNSUPPORTED
    for rt in (BILINEAR, NEAREST, AREA, 7):  # ... and an unknown type
        assert d(p=_params(N, rt=rt)) == UNSUPPORTED, rt
    for fcc in (3, 4, 5, 6):
        if fcc not in (Y800, RGB24, BGR24):
            assert d(p=_params(N, fcc=fcc)) == UNSUPPORTED, fcc
    for k in range(6):
        c = list(c0)
        c[k] = -(2.0 ** 24) - 2
        assert d(rs=[_rec(N, c)]) == UNSUPPORTED, k
        c[k] = 2.0 ** 24
        assert d(rs=[_rec(N, c)]) == OK, k
    assert d(p=_params(N, dst=(32768, 32768), norm=1)) == UNSUPPORTED  # 12 GiB
    if kind == "perspective":  # the horizon rule, last
        assert d(rs=[_rec(N, c0[:6] + (-1 / 32, 0.0, 1.0))]) == UNSUPPORTED
        assert d(rs=[_rec(N, c0[:6] + (-1 / 32, 0.0, 1.0))], p=_params(N, dst=(63, 64))) == UNSUPPORTED
        assert d(rs=[_rec(N, c0[:6] + (-1 / 32, 0.0, 1.0))], border=(256, 0, 0)) == ERROR
    # an ERROR condition wins over an UNSUPPORTED one
    assert d(p=_params(N, dst=(63, 64), rt=AREA), border=(256, 0, 0)) == ERROR
    assert d(p=_params(N, rt=BILINEAR), rs=[_rec(N, (float("nan"),) + tuple(c0[1:]))]) == ERROR


@pytest.mark.parametrize("kind,c0,kernel", [("warp", M0, "vpp_warp_bicubic"), ("perspective", H0, "vpp_persp_bicubic")])
def test_a_spec_adds_the_tensor_rules_behind_the_request(native, kind, c0, kernel):
    N = native
    fr = [N.NV12(None, None, 192, 192, 128, 72)]
    rs = [_rec(N, c0)]

    def spec(dtype=N.TSVPP_F16, mean=(0, 0, 0), scale=(1, 1, 1)):
        return N.TensorSpec(dtype, (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*scale))
    ok = _params(N, fcc=BGR24, planes=PLANAR, norm=1)
    sts, line = _describe(N, kind, ok, fr, rs, spec=spec(), border=(114, 128, 128))
    assert sts == OK and f"kernel={kernel}_tensor<PLANAR,EL_HALF,vec," in line and "out=f16_planar" in line and line.endswith("border=114,128,128")
    # rule 1 first: the request's own status
    assert _describe(N, kind, _params(N, fcc=BGR24, planes=PLANAR, norm=1, rt=BILINEAR), fr, rs, spec=spec(dtype=9))[0] == UNSUPPORTED
    assert _describe(N, kind, ok, fr, [_rec(N, c0, frame=3)], spec=spec(dtype=9))[0] == ERROR
    # rule 2
    assert _describe(N, kind, ok, fr, rs, spec=spec(mean=(0, float("nan"), 0)))[0] == ERROR
    assert _describe(N, kind, ok, fr, rs, spec=spec(scale=(1, 0, 1)))[0] == ERROR
    # rule 3
    assert _describe(N, kind, ok, fr, rs, spec=spec(dtype=9))[0] == UNSUPPORTED
    assert _describe(N, kind, _params(N, fcc=BGR24, planes=PLANAR, norm=0), fr, rs, spec=spec())[0] == UNSUPPORTED
    assert _describe(N, kind, _params(N, fcc=BGR24, planes=MERGED, norm=1), fr, rs, spec=spec())[0] == UNSUPPORTED
    assert _describe(N, kind, _params(N, fcc=Y800, planes=MERGED, norm=1), fr, rs, spec=spec())[0] == OK
    # without a spec the merged and the uint8 flavours are the plain call's
    assert _describe(N, kind, _params(N, fcc=BGR24, planes=MERGED, norm=0), fr, rs)[0] == OK


def test_the_existing_calls_still_refuse_bicubic(native):
    N = native
    L = N.lib()
    fr = (N.NV12 * 1)(N.NV12(None, None, 192, 192, 128, 72))
    buf = ctypes.create_string_buffer(512)
    p = _params(N, rt=BICUBIC)
    spec = N.TensorSpec(N.TSVPP_F32, (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1))
    pt = _params(N, rt=BICUBIC, fcc=BGR24, planes=PLANAR, norm=1)
    ws, qs = (N.Warp * 1)(_rec(N, M0)), (N.Persp * 1)(_rec(N, H0))
    assert L.tsvpp_describe_warp(ctypes.byref(p), 1, fr, 1, ws, -1, -1, -1, 1, buf, len(buf)) == UNSUPPORTED
    assert L.tsvpp_describe_warp_tensor(ctypes.byref(pt), ctypes.byref(spec), 1, fr, 1, ws, -1, -1, -1, 1, buf, len(buf)) == UNSUPPORTED
    assert L.tsvpp_describe_perspective(ctypes.byref(p), 1, fr, 1, qs, -1, -1, -1, 1, buf, len(buf)) == UNSUPPORTED
    assert L.tsvpp_describe_perspective_tensor(ctypes.byref(pt), ctypes.byref(spec), 1, fr, 1, qs, -1, -1, -1, 1, buf, len(buf)) == UNSUPPORTED
    p.resize_type = BILINEAR
    assert L.tsvpp_describe_warp(ctypes.byref(p), 1, fr, 1, ws, -1, -1, -1, 1, buf, len(buf)) == OK and b"mode=warp_bilinear" in buf.value


def _chunks(span):
    return ((span + 14) >> 4) + 1


def _lds_need(f, luma_only=False):
    ny, nuv = f[3] - f[2] + 1, 0 if luma_only else f[7] - f[6] + 1
    return 16 * (ny * _chunks(f[1] - f[0] + 1) + nuv * _chunks(2 * (f[5] - f[4] + 1)))


def _footprint(native, c, w, h, j0, j1, i0, i1):
    out = (ctypes.c_int32 * 8)()
    entry = native.lib().tsvpp_warp_bicubic_footprint if len(c) == 6 else native.lib().tsvpp_persp_bicubic_footprint
    assert entry(ctypes.byref(_rec(native, c)), w, h, j0, j1, i0, i1, out) == OK
    return list(out)


def test_describe_lines(native, monkeypatch):
    """mode= and kernel= are the new calls'; every other key is the BILINEAR call's for the same request, except what the halo changes: lds= (and, under a small
    budget, staged=)"""
    import tensor_stream as ts
    import torch
    if knob_run():
        return

    def fp(dst, rt, fcc=ts.FourCC.BGR24, planes=ts.Planes.PLANAR, norm=True):
        return ts.FrameParameters(width=dst[0], height=dst[1], resize_type=rt, pixel_format=fcc, planes_pos=planes, normalization=norm)
    geo = (1920, 1080, 2048)
    m = ts.warp_rotated_box(960, 540, 300, 240, 0.5, 112, 112)
    q = ts.perspective_from_quad([(800, 400), (1100, 430), (1080, 700), (780, 650)], 112, 112)
    for cubic, plain, item, mode, kernel in ((ts.describe_warp_bicubic, ts.describe_warp, m, "warp_bicubic", "vpp_warp_bicubic"),
                                             (ts.describe_perspective_bicubic, ts.describe_perspective, q, "persp_bicubic", "vpp_persp_bicubic")):
        for n, launches in ((32, 1), (33, 2)):
            d = cubic(fp((112, 112), ts.ResizeType.BICUBIC), geo, [item] * n)
            b = plain(fp((112, 112), ts.ResizeType.BILINEAR), geo, [item] * n)
            assert d["mode"] == mode and d["kernel"] == kernel + "<O_F32_PLANAR,vec,staged,replicate>" and d["launches"] == launches and d["staged"] == n
            assert d["lds"] > b["lds"] > 0
            assert {k: v for k, v in d.items() if k not in ("mode", "kernel", "lds")} == {k: v for k, v in b.items() if k not in ("mode", "kernel", "lds")}
        d = cubic(fp((112, 112), ts.ResizeType.BICUBIC), geo, [item], border=(114, 128, 128), aligned_outputs=False)
        assert d["kernel"] == kernel + "<O_F32_PLANAR,elem,staged,border>" and d["border"] == "114,128,128"
        d = cubic(fp((112, 112), ts.ResizeType.BICUBIC), geo, [item], dtype=torch.float16, mean=0.5, std=0.25)
        assert d["kernel"] == kernel + "_tensor<PLANAR,EL_HALF,vec,staged,replicate>" and d["out"] == "f16_planar" and d["mode"] == mode
    # one tile: lds= is the footprint function's box, with the halo
    one = fp((32, 32), ts.ResizeType.BICUBIC)
    m45 = ts.warp_rotated_box(160, 90, 80, 80, 0.785398, 32, 32)
    f = _footprint(native, m45, 322, 182, 0, 31, 0, 31)
    assert ts.describe_warp_bicubic(one, (322, 182, 384), [m45])["lds"] == _lds_need(f)
    assert ts.describe_warp_bicubic(fp((32, 32), ts.ResizeType.BICUBIC, ts.FourCC.Y800, ts.Planes.MERGED, False), (322, 182, 384), [m45])["lds"] == _lds_need(f, luma_only=True)
    h45 = P.affine(m45)
    assert _footprint(native, h45, 322, 182, 0, 31, 0, 31) == f  # (an affine map's interval box is its corner box)
    assert ts.describe_perspective_bicubic(one, (322, 182, 384), [h45])["lds"] == _lds_need(f)
    # no budget: everything gathers
    monkeypatch.setenv("TSVPP_LDS_KB", "0")
    d = ts.describe_warp_bicubic(one, (322, 182, 384), [m45])
    assert d["staged"] == 0 and d["lds"] == 0 and d["kernel"] == "vpp_warp_bicubic<O_F32_PLANAR,vec,gather,replicate>"


# ---- 4. the footprint property -------------------------------------------------------------------------------------------------------------------------------

def _tiles(dw, dh):
    """(j0, j1, i0, i1) of every tile of a dw x dh output, the shifted last tile column of the vector-store kernels included"""
    cols = [(j, min(j + 31, dw - 1)) for j in range(0, dw, 32)]
    if dw % 4 and dw >= 32:
        cols.append((dw - 32, dw - 1))
    return [(j0, j1, i, min(i + 31, dh - 1)) for j0, j1 in cols for i in range(0, dh, 32)]


@pytest.mark.parametrize("frame", FRAMES)
def test_every_tap_of_a_tile_lies_inside_the_exported_footprint(native, frame):
    """every tile of the three outputs under every item of coord_paths.matrices / homographies ("far", "singular", "left", "bottom" leave the frame or
    degenerate): the box lies inside the frame, every one of the 16 taps of every pixel and of every chroma pair lies inside it -- the zero-weight taps of samples
    beyond the frame included, they are fetched --, and for an affine tile, whose corner coordinates ARE attained, it is at most one pixel wider per side than the
    hull of the taps (one: where the edge rule collapses the upper taps)"""
    import coord_paths as cp
    w, h, _ = frame
    for dw, dh in DSTS:
        items = [(n, m) for n, m in cp.matrices(w, h, dw, dh).items()] + [(n, q) for n, q in cp.homographies(w, h, dw, dh).items()]
        for name, c in items:
            luma, chroma = B.taps(c, w, h, dw, dh)
            for j0, j1, i0, i1 in _tiles(dw, dh):
                f = _footprint(native, c, w, h, j0, j1, i0, i1)
                assert 0 <= f[0] <= f[1] < w and 0 <= f[2] <= f[3] < h and 0 <= f[4] <= f[5] < w // 2 and 0 <= f[6] <= f[7] < h // 2, (name, c, f)
                for grid, (a0, a1, b0, b1), box in ((luma, (j0, j1, i0, i1), f[:4]), (chroma, (j0 >> 1, j1 >> 1, i0 >> 1, i1 >> 1), f[4:])):
                    xa, xb, ya, yb = (t[b0:b1 + 1, a0:a1 + 1] for t in grid)
                    hull = (xa.min(), xb.max(), ya.min(), yb.max())
                    assert box[0] <= hull[0] and hull[1] <= box[1] and box[2] <= hull[2] and hull[3] <= box[3], (name, c, (j0, j1, i0, i1), box, hull)
                    if len(c) == 6:
                        assert hull[0] - box[0] <= 1 and box[1] - hull[1] <= 1 and hull[2] - box[2] <= 1 and box[3] - hull[3] <= 1, (name, c, (j0, j1, i0, i1), box, hull)


def test_footprint_exports_refuse_what_the_bilinear_ones_refuse(native):
    L = native.lib()
    out = (ctypes.c_int32 * 8)()
    w, q = _rec(native, M0), _rec(native, H0)
    for entry, rec in ((L.tsvpp_warp_bicubic_footprint, w), (L.tsvpp_persp_bicubic_footprint, q)):
        assert entry(None, 128, 72, 0, 31, 0, 31, out) == ERROR and entry(ctypes.byref(rec), 128, 72, 0, 31, 0, 31, None) == ERROR
        assert entry(ctypes.byref(rec), 0, 72, 0, 31, 0, 31, out) == ERROR and entry(ctypes.byref(rec), 128, 72, 8, 7, 0, 31, out) == ERROR
        assert entry(ctypes.byref(rec), 128, 72, -2, 31, 0, 31, out) == ERROR and entry(ctypes.byref(rec), 128, 72, 0, 31, 4, 3, out) == ERROR
    horizon = _rec(native, M0 + (-1 / 32, 0.0, 1.0))
    assert L.tsvpp_persp_bicubic_footprint(ctypes.byref(horizon), 128, 72, 0, 63, 0, 63, out) == UNSUPPORTED
