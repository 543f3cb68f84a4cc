"""No GPU: tsvpp_convert_rois_p010_area's request rules in their order (include/tsvpp.h) through the describe call and the convert call with a null context,
the describe line, the LDS budget knob, and tsvpp_box_p010_plane -- the contract's executable form -- on the cut of a box against tests/p010_area_util.box."""
import ctypes

import numpy as np
import pytest

import p010_util as M
from p010_area_util import AREA, box
from tensor_stream import _native as N

OK, UNSUPPORTED, ERROR = 0, -2, -3
KNOBS = ("TSVPP_LDS_KB", "TSVPP_FORCE_GATHER", "TSVPP_NT_STORES")


def both(entry="rois_p010_area", frames=((1920, 1080, 4096),), rois=((0, 100, 60, 400, 760),), dst=(128, 256), rt=AREA, fcc=M.RGB24, planes=M.PLANAR, norm=1, spec=None):
    # -> (status of the describe call, of the convert call with a null context, the describe line)
    p = N.Params(0, 0, 0, 0, dst[0], dst[1], rt, fcc, planes, norm)
    fr = (N.P010 * len(frames))(*[N.P010(None, None, f[2], f[2], f[0], f[1]) for f in frames])
    bx = (N.Roi * len(rois))(*[N.Roi(*b) for b in rois])
    sp = None if spec is None else ctypes.byref(N.TensorSpec(spec, (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1)))
    buf = ctypes.create_string_buffer(512)
    d = getattr(N.lib(), "tsvpp_describe_" + entry)(ctypes.byref(p), sp, len(frames), fr, len(rois), bx, 1, buf, len(buf))
    c = getattr(N.lib(), "tsvpp_convert_" + entry)(None, len(frames), fr, len(rois), bx, ctypes.byref(p), sp, (ctypes.c_void_p * len(rois))(), None)
    return d, c, buf.value.decode()


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("req", [dict(rt=M.BILINEAR), dict(rt=M.NEAREST), dict(rt=2),
                                 dict(rois=((0, 101, 60, 401, 760),)),                                              # an odd left
                                 dict(frames=((16386, 1080, 32772),), rois=((0, 0, 0, 16386, 64),), dst=(2050, 64)),  # a box side above the limit
                                 dict(rois=((0, 0, 0, 64, 64),), dst=(16386, 64)),                                  # an output side above the limit
                                 dict(rois=((0, 0, 0, 270, 64),), dst=(16, 16)), dict(rois=((0, 0, 0, 64, 270),), dst=(16, 16)),  # 18 taps on one luma axis
                                 dict(entry="rois_p010")])  # the NEAREST / BILINEAR call keeps refusing AREA
# (no case of a chroma-only excess: with N, n even and g = gcd(N, n), luma has (n - g + N - 1) / n + 1 taps and chroma (n - g + N - 2) / n + 1, never more)
def test_refusals(req):
    assert both(**req)[:2] == (UNSUPPORTED, UNSUPPORTED), req


def test_the_p010_rules_come_first_and_the_limit_is_accepted():
    assert both(frames=((1920, 1080, 4097),), rt=M.BILINEAR)[:2] == (ERROR, ERROR)  # an odd pitch wins over the type
    assert both(rois=((0, 101, 60, 401, 760),), rt=M.BILINEAR)[:2] == (UNSUPPORTED, UNSUPPORTED)
    assert both(rois=((0, 0, 0, 254, 254),), dst=(16, 16))[:2] == (OK, ERROR)       # 17 taps; a null context is the convert call's error


@pytest.mark.parametrize("req,kernel,out", [
    (dict(planes=M.MERGED, norm=0), "vpp_rois_p010_area<O_U8_MERGED,vec>", "u8_merged"),
    (dict(fcc=M.Y800), "vpp_rois_p010_area<O_Y800_F32,vec>", "y800_f32"),
    (dict(spec=1), "vpp_rois_p010_area_tensor<PLANAR,EL_HALF,vec>", "f16_planar")])
def test_describe_line(req, kernel, out):
    """300 x 700 to 128 x 256 beside 64 x 64: 300 -> 128 has 4 taps (150 -> 64 too), 700 -> 256 has 4; the widest footprint row is 77 words, 11 chunks, which
    the budget holds in bands of the 32-row cap"""
    d, _, text = both(rois=((0, 100, 60, 400, 760), (0, 0, 0, 64, 64)), **req)
    assert d == OK and text.startswith("mode=area ") and f" kernel={kernel} " in text and f" out={out} " in text and " src=p010 rois=2 " in text, text
    assert " staged=2 " in text and text.endswith(" limit=64 taps=4x4 band=32"), text


def test_a_shrunk_budget_is_refused_not_launched_with_zero_rows(monkeypatch):
    """254 -> 16: one tile of 254 words, 33 chunks a row; one-row bands take 128 + 2 x 16 x 64 = 2176 bytes.  2 KiB refuse it, 3 KiB hold one row"""
    req = dict(rois=((0, 0, 0, 254, 254),), dst=(16, 16))
    monkeypatch.setenv("TSVPP_LDS_KB", "2")
    assert both(**req)[0] == UNSUPPORTED  # (the convert call reads the knob from its context)
    monkeypatch.setenv("TSVPP_LDS_KB", "3")
    d, _, text = both(**req)
    assert d == OK and " lds=2176 " in text and text.endswith(" taps=17x17 band=1"), text
    monkeypatch.setenv("TSVPP_FORCE_GATHER", "1")
    assert both(**req)[0] == UNSUPPORTED  # there is no gathering variant


@pytest.mark.parametrize("bx,dst", [((6, 8, 42, 32), (16, 16)), ((4, 2, 258, 256), (16, 16)), ((0, 0, 96, 20), (32, 40))])
def test_plane_function_on_the_cut_of_a_box(bx, dst):
    """the three planes of a box cut out of a 262 x 258 frame: the host's compile of the kernel's functions against the model, bit for bit"""
    rng = np.random.default_rng(9)
    y, uv = rng.integers(0, 65536, (258, 270), dtype=np.uint16), rng.integers(0, 65536, (129, 270), dtype=np.uint16)
    l, t, r, b = bx
    Ys, UVs = M.samples(y[t:b, l:r]), M.samples(uv[t // 2:b // 2, l:r])
    for S, (w, h) in ((Ys, dst), (UVs[:, 0::2], (dst[0] // 2, dst[1] // 2)), (UVs[:, 1::2], (dst[0] // 2, dst[1] // 2))):
        S, out = np.ascontiguousarray(S, dtype=np.uint16), np.zeros((h, w), np.uint16)
        assert N.lib().tsvpp_box_p010_plane(S.ctypes.data, S.shape[1], S.shape[0], out.ctypes.data, w, h) == OK
        assert np.array_equal(out, box(S, w, h))
