"""No GPU: the host side of tsvpp_letterbox_rect / tsvpp_convert_letterbox / tsvpp_describe_letterbox (include/tsvpp.h) -- exported symbols and struct layout,
the default rectangle against a Python restatement of its integer rule, every validation status in its stated order (through the describe call, and through the
convert call with a null context: the request is checked before the context is touched), the describe line, the staged / gather decision under the LDS knob."""
import ctypes
import os
import random
import subprocess
import sys

import pytest

from letterbox_util import default_rect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OK, UNSUPPORTED, ERROR = 0, -2, -3
NEAREST, BILINEAR, BICUBIC, AREA = 0, 1, 2, 3
Y800, RGB24, BGR24, NV12, UYVY, YUV444, HSV = range(7)
F1080 = (1920, 1080, 2048)


@pytest.fixture(scope="module")
def native():
    from tensor_stream import _native
    _native.lib()
    return _native


def P(native, dst=(640, 640), rt=BILINEAR, fcc=RGB24, planes=1, norm=0, crop=(0, 0, 0, 0)):
    return native.Params(crop[0], crop[1], crop[2], crop[3], dst[0], dst[1], rt, fcc, planes, norm)


def both(native, p, frames, rects=None, pad=(114, 128, 128), n=None, null=()):
    """the status of tsvpp_describe_letterbox and of tsvpp_convert_letterbox with a NULL context for the same request: (describe, convert, text)"""
    L = native.lib()
    fr = (native.NV12 * max(len(frames), 1))(*[native.NV12(None, None, f[2] if len(f) > 2 else 0, f[3] if len(f) > 3 else (f[2] if len(f) > 2 else 0), f[0], f[1])
                                               for f in frames])
    rc = None if rects is None else (native.Rect * max(len(rects), 1))(*[native.Rect(*r) for r in rects])
    outs = (ctypes.c_void_p * max(len(frames), 1))()
    buf = ctypes.create_string_buffer(512)
    cnt = len(frames) if n is None else n
    pp = None if "p" in null else ctypes.byref(p)
    a_fr = None if "frames" in null else fr
    d = L.tsvpp_describe_letterbox(pp, cnt, a_fr, rc, 1, buf, len(buf))
    c = L.tsvpp_convert_letterbox(None, cnt, a_fr, pp, rc, pad[0], pad[1], pad[2], outs, None)
    return d, c, buf.value.decode()


def test_symbols_signatures_and_struct_layout(native):
    L = native.lib()
    for sym in ("tsvpp_letterbox_rect", "tsvpp_convert_letterbox", "tsvpp_describe_letterbox"):
        assert sym in native.SYMBOLS and hasattr(L, sym)
    assert ctypes.sizeof(native.Rect) == 16
    assert [f[0] for f in native.Rect._fields_] == ["left", "top", "width", "height"]
    assert native.TSVPP_MAX_LETTERBOX == 32
    assert len(L.tsvpp_letterbox_rect.argtypes) == 5 and L.tsvpp_letterbox_rect.restype is ctypes.c_int
    assert len(L.tsvpp_convert_letterbox.argtypes) == 10 and L.tsvpp_convert_letterbox.restype is ctypes.c_int
    assert len(L.tsvpp_describe_letterbox.argtypes) == 7 and L.tsvpp_describe_letterbox.restype is ctypes.c_int
    hdr = open(os.path.join(ROOT, "include", "tsvpp.h")).read()
    assert "#define TSVPP_MAX_LETTERBOX 32" in hdr
    assert "int tsvpp_letterbox_rect(int in_w, int in_h, int dst_w, int dst_h, tsvpp_rect *out);" in hdr
    assert "(114, 128, 128) is gray 114" in hdr and "(16, 128, 128) is black" in hdr
    import tensor_stream as ts
    from tensor_stream import vpp
    assert ts.letterbox_rect is vpp.letterbox_rect and ts.describe_letterbox is vpp.describe_letterbox and ts.Rect is native.Rect
    assert hasattr(ts.VideoProcessor, "convert_letterbox")


def test_the_header_compiles_as_c_and_the_struct_is_16_bytes(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "tsvpp.h"\n_Static_assert(sizeof(tsvpp_rect) == 16, "tsvpp_rect");\nint main(void) { return TSVPP_MAX_LETTERBOX == 32 ? 0 : 1; }\n')
    cc = os.environ.get("CC", "cc")
    subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(src)])
    subprocess.check_call([str(tmp_path / "t")])


def c_rect(native, iw, ih, dw, dh):
    r = native.Rect()
    sts = native.lib().tsvpp_letterbox_rect(iw, ih, dw, dh, ctypes.byref(r))
    return sts, (r.left, r.top, r.width, r.height)


def test_default_rectangle_named_cases(native):
    assert c_rect(native, 1920, 1080, 640, 640) == (OK, (0, 140, 640, 360))
    assert c_rect(native, 1080, 1920, 640, 640) == (OK, (140, 0, 360, 640))
    assert c_rect(native, 1280, 720, 640, 360) == (OK, (0, 0, 640, 360))    # equal aspect: no pad
    assert c_rect(native, 640, 640, 640, 640) == (OK, (0, 0, 640, 640))
    assert c_rect(native, 2, 2, 640, 640) == (OK, (0, 0, 640, 640))         # 2 x 2: up-scaled to the whole canvas
    assert c_rect(native, 2, 2, 2, 2) == (OK, (0, 0, 2, 2))
    assert c_rect(native, 4000, 2, 640, 640) == (OK, (0, 318, 640, 2))      # a sliver: the height clamps to 2
    assert c_rect(native, 2, 4000, 640, 640) == (OK, (318, 0, 2, 640))
    assert c_rect(native, 1920, 1080, 70, 66) == (OK, (0, 12, 70, 40))      # left / top are even where the margin is odd: 13 -> 12
    # 64-bit arithmetic: products beyond 2^31
    assert c_rect(native, 2000000000, 2, 2000000000, 2000000000) == (OK, default_rect(2000000000, 2, 2000000000, 2000000000))
    assert c_rect(native, 1999999998, 2000000000, 2000000000, 1999999998) == (OK, default_rect(1999999998, 2000000000, 2000000000, 1999999998))
    L = native.lib()
    assert L.tsvpp_letterbox_rect(1920, 1080, 640, 640, None) == ERROR
    for bad in [(0, 1080, 640, 640), (1920, -2, 640, 640), (1920, 1080, 0, 640), (1920, 1080, 640, -640)]:
        assert c_rect(native, *bad)[0] == ERROR
    assert c_rect(native, 1920, 1080, 641, 640)[0] == UNSUPPORTED and c_rect(native, 1920, 1080, 640, 639)[0] == UNSUPPORTED


def test_default_rectangle_against_the_integer_rule(native):
    r = random.Random(20261018)
    for _ in range(4000):
        big = r.random() < 0.2
        iw, ih = (r.randrange(1, 1 << 30), r.randrange(1, 1 << 30)) if big else (r.randrange(1, 4097), r.randrange(1, 4097))
        dw, dh = 2 * r.randrange(1, 1025), 2 * r.randrange(1, 1025)
        sts, got = c_rect(native, iw, ih, dw, dh)
        assert (sts, got) == (OK, default_rect(iw, ih, dw, dh)), (iw, ih, dw, dh)
        left, top, w, h = got
        assert w % 2 == 0 and h % 2 == 0 and left % 2 == 0 and top % 2 == 0 and w >= 2 and h >= 2
        assert left >= 0 and top >= 0 and left + w <= dw and top + h <= dh and (w == dw or h == dh)


# in the order letterbox_plan (csrc/tsvpp_plan.cpp) states them; every case is at fault in exactly the way its name says
ERROR_CASES = [
    ("null params", dict(null=("p",))),
    ("null frames", dict(null=("frames",))),
    ("n zero", dict(n=0)),
    ("n negative", dict(n=-1)),
    ("frame without a size", dict(frames=[(0, 1080, 2048)])),
    ("frame with a negative height", dict(frames=[(1920, -1080, 2048)])),
    ("pitch below the width", dict(frames=[(1920, 1080, 1900)])),
    ("second frame bad", dict(frames=[F1080, (1280, 0, 1280)])),
    ("dst_width zero", dict(dst=(0, 640))),
    ("dst_height zero", dict(dst=(640, 0))),
    ("dst negative", dict(dst=(-640, 640))),
    ("crop in the parameters", dict(crop=(0, 0, 64, 64))),
    ("crop_left alone", dict(crop=(2, 0, 0, 0))),
    ("empty rectangle", dict(rects=[(0, 0, 0, 64)])),
    ("empty rectangle (height)", dict(rects=[(0, 0, 64, 0)])),
    ("negative width", dict(rects=[(10, 10, -4, 64)])),
    ("rectangle with a negative corner", dict(rects=[(-2, 0, 64, 64)])),
    ("rectangle past the right edge", dict(rects=[(600, 0, 42, 64)])),
    ("rectangle past the bottom edge", dict(rects=[(0, 600, 64, 42)])),
    ("rectangle larger than the canvas", dict(rects=[(0, 0, 642, 640)])),
    ("pad_y above 255", dict(pad=(256, 128, 128)), True),
    ("pad_u negative", dict(pad=(114, -1, 128)), True),
    ("pad_v above 255", dict(pad=(114, 128, 1000)), True),
]
UNSUPPORTED_CASES = [
    ("odd dst_width", dict(dst=(639, 640))),
    ("odd dst_height", dict(dst=(640, 639))),
    ("odd frame width", dict(frames=[(1919, 1080, 2048)])),
    ("odd frame height", dict(frames=[(1920, 1079, 2048)])),
    ("odd rectangle left", dict(rects=[(1, 0, 64, 64)])),
    ("odd rectangle top", dict(rects=[(0, 3, 64, 64)])),
    ("odd rectangle width", dict(rects=[(0, 0, 63, 64)])),
    ("odd rectangle height", dict(rects=[(0, 0, 64, 65)])),
    ("AREA", dict(rt=AREA)),
    ("unknown resize type", dict(rt=7)),
    ("unknown planes", dict(planes=2)),
    ("NV12 output", dict(fcc=NV12)),
    ("UYVY output", dict(fcc=UYVY)),
    ("YUV444 output", dict(fcc=YUV444)),
    ("HSV output", dict(fcc=HSV)),
    ("unknown fourcc", dict(fcc=9)),
    ("an output of 4 GiB", dict(dst=(32768, 32768), norm=1, fcc=Y800)),
]


def _status(native, case):
    case = dict(case)
    frames = case.pop("frames", [F1080])
    kw = {k: case.pop(k) for k in ("rects", "pad", "n", "null") if k in case}
    return both(native, P(native, **case), frames, **kw)


@pytest.mark.parametrize("case", ERROR_CASES, ids=[c[0] for c in ERROR_CASES])
def test_invalid_arguments_are_errors(native, case):
    d, c, text = _status(native, case[1])
    # (the describe call takes no pad: a pad at fault is the convert call's to refuse)
    assert (d, c, text[:5]) == ((OK, ERROR, "mode=") if len(case) > 2 else (ERROR, ERROR, ""))


@pytest.mark.parametrize("case", UNSUPPORTED_CASES, ids=[c[0] for c in UNSUPPORTED_CASES])
def test_unsupported_requests(native, case):
    d, c, text = _status(native, case[1])
    assert (d, c, text) == (UNSUPPORTED, UNSUPPORTED, "")


def test_errors_come_before_unsupported_and_in_the_stated_order(native):
    """a request at fault in two ways answers the status that is stated first"""
    every_unsupported = dict(dst=(640, 640), rt=AREA, fcc=HSV, planes=2, frames=[(1919, 1079, 2048)], rects=[(1, 1, 63, 63)])
    assert _status(native, every_unsupported)[:2] == (UNSUPPORTED, UNSUPPORTED)
    for _, err in [c[:2] for c in ERROR_CASES]:
        if "null" in err and "frames" in err["null"]:
            continue  # (no frames to be odd)
        d, c, _ = _status(native, {**every_unsupported, **err})
        assert c == ERROR and d == (UNSUPPORTED if "pad" in err else ERROR), err  # (describe never sees the pad: it gets as far as the odd frame)
    # inside TSVPP_ERROR: the frame before the canvas, the canvas before the crop, the crop before the rectangle, the rectangle before the pad -- each pair
    # leaves the later fault in place and repairs the earlier one: still TSVPP_ERROR; what proves the order is that no UNSUPPORTED fault shows through
    assert _status(native, dict(frames=[(1919, 1080, 100)]))[:2] == (ERROR, ERROR)       # pitch below the width, on an odd frame
    assert _status(native, dict(dst=(639, 0)))[:2] == (ERROR, ERROR)                     # a missing height, beside an odd width
    assert _status(native, dict(rects=[(1, 1, 700, 63)]))[:2] == (ERROR, ERROR)          # outside the canvas, and odd
    assert _status(native, dict(rt=AREA, pad=(0, 0, 256)))[:2] == (UNSUPPORTED, ERROR)
    # inside TSVPP_UNSUPPORTED every fault answers the same status; a legal request with every legal oddity is fine
    assert _status(native, dict(rects=[(638, 638, 2, 2)], rt=BICUBIC, fcc=Y800, planes=0, norm=1, frames=[(2, 2)]))[:2] == (OK, ERROR)


def test_a_legal_request_needs_a_context_to_convert_and_a_buffer_to_describe(native):
    d, c, text = _status(native, {})
    assert d == OK and text.startswith("mode=bilinear ")
    assert c == ERROR  # the request is fine; the context is null
    L = native.lib()
    p = P(native)
    fr = (native.NV12 * 1)(native.NV12(None, None, 2048, 2048, 1920, 1080))
    assert L.tsvpp_describe_letterbox(ctypes.byref(p), 1, fr, None, 1, None, 0) == ERROR
    # legal: up-scaling, a rectangle that does not keep the aspect, frames of different sizes, an unset pitch, pad 0 and 255
    d, c, _ = both(native, p, [(1920, 1080), (64, 36, 64), (720, 1280, 768, 1024)], rects=[(0, 0, 640, 640), (2, 2, 636, 636), (320, 0, 2, 640)], pad=(0, 255, 0))
    assert (d, c) == (OK, ERROR)


def test_describe_line(native):
    import tensor_stream as ts
    from tensor_stream import vpp
    fp = ts.FrameParameters(width=640, height=640, resize_type=BILINEAR, pixel_format=BGR24, planes_pos=0, normalization=True)
    d = ts.describe_letterbox(fp, [F1080, F1080])
    assert d["mode"] == "bilinear" and d["out"] == "f32_planar" and d["dst"] == "640x640" and d["frames"] == 2
    assert d["kernel"].startswith("vpp_letterbox<") and "_kernel<" not in d["kernel"]  # (tests/dispatch_grid.py scrapes "vpp_..._kernel<" literals)
    assert d["tiles"] == "20x20" and d["limit"] == 32 and d["launches"] == 1 and d["inner"] == "640x360+0+140"
    assert d["grid"] == 400 * 2 and d["shape"] == "8x16" and d["tail"] == 0
    for key in ("mode", "out", "dst", "frames", "launches", "kernel", "shape", "lds", "grid", "tiles", "staged", "tail", "nt", "limit", "inner"):
        assert key in d
    many = ts.describe_letterbox(fp, [F1080] * 33)
    assert many["launches"] == 2 and many["frames"] == 33 and many["grid"] == 400 * 32
    # the caller's rectangle is the one reported; a portrait frame gets its own default
    assert ts.describe_letterbox(fp, [F1080], rects=[(6, 2, 20, 10)])["inner"] == "20x10+6+2"
    assert ts.describe_letterbox(fp, [(1080, 1920, 1088)])["inner"] == "360x640+140+0"
    # the raw line parses with the parser of tsvpp_describe's lines; a buffer that is too small truncates, never overruns
    buf = ctypes.create_string_buffer(512)
    fr = (native.NV12 * 2)(*[native.NV12(None, None, 2048, 2048, 1920, 1080)] * 2)
    assert native.lib().tsvpp_describe_letterbox(ctypes.byref(fp.parameters), 2, fr, None, 1, buf, len(buf)) == OK
    assert vpp._parse_selection(buf.value.decode()) == d
    small = ctypes.create_string_buffer(16)
    assert native.lib().tsvpp_describe_letterbox(ctypes.byref(fp.parameters), 2, fr, None, 1, small, len(small)) == OK
    assert small.raw[-1:] == b"\0" and buf.value.startswith(small.value)


def test_vector_and_element_wise_variants_and_the_tail():
    import tensor_stream as ts
    fp = ts.FrameParameters(width=70, height=66, resize_type=BICUBIC, pixel_format=RGB24, planes_pos=1, normalization=False)
    a = ts.describe_letterbox(fp, F1080, aligned_outputs=True)
    b = ts.describe_letterbox(fp, F1080, aligned_outputs=False)
    assert a["kernel"].split(",")[2] == "vec" and a["tail"] == 2 and a["tiles"] == "3x3"  # 70 = 4 k + 2: the last tile column is shifted to the right edge
    assert b["kernel"].split(",")[2] == "elem" and b["tail"] == 0
    narrow = ts.FrameParameters(width=30, height=34, resize_type=BICUBIC, pixel_format=RGB24, planes_pos=1, normalization=False)
    c = ts.describe_letterbox(narrow, F1080, aligned_outputs=True)
    assert c["kernel"].split(",")[2] == "elem" and c["tail"] == 0  # narrower than a tile: no column to shift


SCRIPT = r"""
import sys
sys.path[:0] = [{root!r}, {pkg!r}]
import tensor_stream as ts
fp = ts.FrameParameters(width=640, height=640, resize_type=1, pixel_format=2, planes_pos=0, normalization=True)
d = ts.describe_letterbox(fp, [(1920, 1080, 2048), (1920, 1080, 2048)])
print(d["kernel"], d["staged"], d["lds"])
"""


def _describe_under(env_extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("TSVPP_")}
    env.update(env_extra)
    out = subprocess.check_output([sys.executable, "-c", SCRIPT.format(root=ROOT, pkg=os.path.join(ROOT, "tensor-stream_amd"))], env=env)
    k, staged, lds = out.decode().split()
    return k, int(staged), int(lds)


def test_the_lds_budget_flips_staged_to_gather():
    k, staged, lds = _describe_under({"TSVPP_DEBUG_KNOBS": "1"})
    assert k.endswith(",staged>") and staged == 2 and 0 < lds <= 40 * 1024
    k0, staged0, lds0 = _describe_under({"TSVPP_DEBUG_KNOBS": "1", "TSVPP_LDS_KB": "0"})
    assert k0.endswith(",gather>") and staged0 == 0 and lds0 == 0
    # the knob is a debug knob: ignored without the gate
    assert _describe_under({"TSVPP_LDS_KB": "0"}) == (k, staged, lds)
    assert _describe_under({"TSVPP_DEBUG_KNOBS": "1", "TSVPP_FORCE_GATHER": "1"})[1] == 0


def test_python_argument_checks():
    from tensor_stream import vpp
    assert vpp.letterbox_rect(1920, 1080, 640, 640) == (0, 140, 640, 360)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.letterbox_rect(1920, 1080, 641, 640)
    with pytest.raises(ValueError):
        vpp._rects([(0, 0, 2, 2)], 2)
    with pytest.raises(ValueError):
        vpp._rects([(0, 0, 2)], 1)
    r = vpp._rects([(2, 4, 6, 8)], 1)
    assert (r[0].left, r[0].top, r[0].width, r[0].height) == (2, 4, 6, 8)
