"""No GPU: the host side of tsvpp_convert_letterbox_p010_bicubic (include/tsvpp.h) -- the exported pair, the describe line and every refusal in its order.  The
arithmetic (tsvpp_cubic_p010_plane against tests/p010_cubic_util.py) is tests/test_rois_p010_bicubic_cpu.py's."""
import ctypes

import pytest

import p010_util as M
from p010_cubic_util import BICUBIC
from tensor_stream import _native as N

OK, UNSUPPORTED, ERROR = 0, -2, -3
NAMES = ["tsvpp_convert_letterbox_p010_bicubic", "tsvpp_describe_letterbox_p010_bicubic"]


def both(frames=((1920, 1080, 4096),), dst=(1280, 1280), rects=None, rt=BICUBIC, spec=None, null_p=False, call="_bicubic"):
    # -> (status of the describe call, of the convert call with a null context, the describe line); a frame is (width, height, pitch)
    p = None if null_p else ctypes.byref(N.Params(0, 0, 0, 0, dst[0], dst[1], rt, M.RGB24, M.PLANAR, 1))
    fr = (N.P010 * len(frames))(*[N.P010(None, None, f[2], f[2], f[0], f[1]) for f in frames])
    rc = None if rects is None else (N.Rect * len(rects))(*[N.Rect(*r) for r in rects])
    sp = None if spec is None else ctypes.byref(N.TensorSpec(spec, (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1)))
    buf = ctypes.create_string_buffer(512)
    d = getattr(N.lib(), "tsvpp_describe_letterbox_p010" + call)(p, sp, len(frames), fr, rc, 1, buf, len(buf))
    c = getattr(N.lib(), "tsvpp_convert_letterbox_p010" + call)(None, len(frames), fr, p, sp, rc, 64, 512, 512, (ctypes.c_void_p * len(frames))(), None)
    return d, c, buf.value.decode()


def test_both_symbols_are_exported_and_listed():
    for name in NAMES:
        assert name in N.SYMBOLS and getattr(N.lib(), name)


@pytest.mark.parametrize("spec,kernel", [(None, "vpp_letterbox_p010_bicubic<O_F32_PLANAR,vec>"), (1, "vpp_letterbox_p010_bicubic_tensor<PLANAR,EL_HALF,vec>")])
def test_describe_1080p_into_1280(spec, kernel):
    d, c, text = both(spec=spec)
    keys = dict(item.partition("=")[::2] for item in text.split(" "))
    assert (d, c) == (OK, ERROR) and keys["kernel"] == kernel and keys["mode"] == "bicubic" and keys["src"] == "p010", text
    assert keys["inner"] == "1280x720+0+280" and keys["grid"] == "1600" and keys["limit"] == "32" and keys["staged"] == "1", text
    assert int(keys["band"]) >= 1 and int(keys["lds"]) <= 40 * 1024, text


ONE_TILE = dict(dst=(32, 32), rects=((0, 0, 32, 32),))


@pytest.mark.parametrize("req", [dict(rt=M.BILINEAR), dict(rt=3), dict(rt=M.NEAREST), dict(rt=77),  # any type but BICUBIC
                                 dict(frames=((258, 32, 516),), **ONE_TILE),                        # a ratio just above 8
                                 dict(frames=((16386, 1080, 32772),))])                             # a side above TSVPP_CUBIC_P010_MAX_SIDE
def test_refused_as_unsupported(req):
    d, c, _ = both(**req)
    assert (d, c) == (UNSUPPORTED, UNSUPPORTED), req


@pytest.mark.parametrize("req", [dict(rects=((0, 0, 1280, 721),)), dict(rects=((1, 0, 1280, 720),)), dict(null_p=True)])
@pytest.mark.parametrize("rt", [BICUBIC, M.NEAREST])
def test_the_bilinear_calls_rules_come_first(req, rt):
    """an odd rectangle number and a null p answer what tsvpp_convert_letterbox_p010 answers for BILINEAR, whatever this call's type"""
    assert both(rt=rt, **req)[:2] == both(rt=M.BILINEAR, call="", **req)[:2] != (OK, OK)


def test_the_ratio_limit_itself_and_the_existing_call():
    """256 -> 32 is served; tsvpp_convert_letterbox_p010 keeps refusing BICUBIC"""
    assert both(frames=((256, 32, 512),), **ONE_TILE)[0] == OK
    assert both(call="")[:2] == (UNSUPPORTED, UNSUPPORTED)
