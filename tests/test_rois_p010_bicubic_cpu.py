"""No GPU: tsvpp_convert_rois_p010_bicubic's contract (include/tsvpp.h) -- the integer model (tests/p010_cubic_util.py) against the real-valued cubic at the same
phases, tsvpp_cubic_p010_plane (the kernel's own functions, compiled for the host) against the model bit for bit, every refusal of its own through the describe
call (and the convert call with a null context), and the describe line."""
import ctypes

import numpy as np
import pytest

import p010_cubic_util as Q
import p010_util as M
from tensor_stream import _native as N

OK, UNSUPPORTED, ERROR = 0, -2, -3
# (W, H) -> (w, h), and whether a 0 / 1023 checkerboard overshoots there (F = 0 on both axes does not: the identity, and the centred odd ratio 9)
SHAPES = [((24, 20), (24, 20), False), ((16, 12), (32, 24), True), ((4, 4), (40, 36), True), ((64, 48), (32, 24), True), ((48, 36), (32, 24), True),
          ((256, 256), (32, 32), True), ((288, 32), (32, 32), False), ((96, 20), (32, 40), True)]


def random_plane(W, H, seed=5):
    return np.random.default_rng(seed).integers(0, 1024, (H, W)).astype(np.uint16)


def checkerboard(W, H):
    """0 / 1023 in blocks of 3 samples: h reaches both ends of its range, k both clamps"""
    y, x = np.mgrid[0:H, 0:W]
    return (((x // 3 + y // 3) & 1) * 1023).astype(np.uint16)


def test_weights_sum_to_one_for_all_64_phases():
    _, w = Q.axis(64, 4096)  # 32 rem / n = j + 1/2 (mod 64): every phase 0..63 occurs
    assert len({tuple(r) for r in w}) == 64 and (w.sum(1) == Q.ONE).all() and np.abs(w).sum(1).max() == 1.375 * Q.ONE


@pytest.mark.parametrize("src,dst", [s[:2] for s in SHAPES])
def test_model_against_the_real_valued_cubic(src, dst):
    S = random_plane(*src)
    err = np.abs(Q.cubic(S, *dst) - np.clip(Q.cubic(S, *dst, exact=True), 0, 1023)).max()
    assert err <= 1.1875, err


def test_flat_and_identity_come_back_unchanged():
    assert (Q.cubic(np.full((12, 16), 777), 40, 18) == 777).all()
    S = random_plane(24, 20)
    assert np.array_equal(Q.cubic(S, 24, 20), S)


@pytest.mark.parametrize("content", ["random", "checkerboard"])
@pytest.mark.parametrize("src,dst,overshoots", SHAPES)
def test_plane_function_against_the_model(src, dst, overshoots, content):
    S = random_plane(*src) if content == "random" else checkerboard(*src)
    if content == "checkerboard" and overshoots:  # the unclamped k leaves 0..1023 on both sides, even by the model's whole error bound: both clamps act
        e = Q.cubic(S, *dst, exact=True)
        assert e.min() < -1.1875 and e.max() > 1023 + 1.1875, (e.min(), e.max())
    out = np.zeros(dst[::-1], np.uint16)
    assert N.lib().tsvpp_cubic_p010_plane(S.ctypes.data, src[0], src[1], out.ctypes.data, dst[0], dst[1]) == OK
    assert np.array_equal(out, Q.cubic(S, *dst))


def both(entry="rois_p010_bicubic", frames=((1920, 1080, 4096),), rois=((0, 100, 60, 164, 108),), dst=(112, 112), rt=Q.BICUBIC, fcc=M.RGB24, planes=M.PLANAR, norm=1, spec=None):
    # -> (status of the describe call, of the convert call with a null context, the describe line)
    p = N.Params(0, 0, 0, 0, dst[0], dst[1], rt, fcc, planes, norm)
    fr = (N.P010 * len(frames))(*[N.P010(None, None, f[2], f[2], f[0], f[1]) for f in frames])
    bx = (N.Roi * len(rois))(*[N.Roi(*b) for b in rois])
    sp = None if spec is None else ctypes.byref(N.TensorSpec(spec, (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1)))
    buf = ctypes.create_string_buffer(512)
    d = getattr(N.lib(), "tsvpp_describe_" + entry)(ctypes.byref(p), sp, len(frames), fr, len(rois), bx, 1, buf, len(buf))
    c = getattr(N.lib(), "tsvpp_convert_" + entry)(None, len(frames), fr, len(rois), bx, ctypes.byref(p), sp, (ctypes.c_void_p * len(rois))(), None)
    return d, c, buf.value.decode()


@pytest.mark.parametrize("req", [dict(rt=M.BILINEAR), dict(rt=M.NEAREST), dict(rt=3), dict(rois=((0, 101, 60, 165, 108),)), dict(rois=((0, 100, 61, 164, 109),)),
                                 dict(frames=((16386, 1080, 32772),), rois=((0, 0, 0, 16386, 64),), dst=(2050, 64)),  # a box side above the limit
                                 dict(rois=((0, 0, 0, 64, 64),), dst=(16386, 64)),                                  # an output side above the limit
                                 dict(rois=((0, 0, 0, 258, 64),), dst=(32, 32)), dict(rois=((0, 0, 0, 64, 258),), dst=(32, 32)),  # N = 8 n + 2 on one luma axis
                                 dict(entry="rois_p010")])  # the NEAREST / BILINEAR call keeps refusing BICUBIC
def test_refusals(req):
    assert both(**req)[:2] == (UNSUPPORTED, UNSUPPORTED), req


def test_the_p010_rules_come_first_and_the_limit_is_accepted():
    assert both(frames=((1920, 1080, 4097),), rt=M.BILINEAR)[:2] == (ERROR, ERROR)  # an odd pitch wins over the type
    assert both(rois=((0, 0, 0, 256, 256),), dst=(32, 32))[:2] == (OK, ERROR)       # N = 8 n; a null context is the convert call's error


@pytest.mark.parametrize("req,kernel,out", [
    (dict(planes=M.MERGED, norm=0), "vpp_rois_p010_bicubic<O_U8_MERGED,vec>", "u8_merged"),
    (dict(fcc=M.Y800), "vpp_rois_p010_bicubic<O_Y800_F32,vec>", "y800_f32"),
    (dict(spec=1), "vpp_rois_p010_bicubic_tensor<PLANAR,EL_HALF,vec>", "f16_planar")])
def test_describe_line(req, kernel, out):
    """64 x 64 to 64 x 64: a tile's footprint is its 32 rows and one or two on either side, so the band height is its cap of 32 rows"""
    d, _, text = both(rois=((0, 100, 60, 164, 124),), dst=(64, 64), **req)
    assert d == OK and text.startswith("mode=bicubic ") and f" kernel={kernel} " in text and f" out={out} " in text and " src=p010 rois=1 " in text, text
    assert " staged=1 " in text and text.endswith(" limit=64 band=32"), text
