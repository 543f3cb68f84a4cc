"""No GPU: the host side of tsvpp_convert_rois / tsvpp_describe_rois (include/tsvpp.h) -- exported symbols and struct layout, every validation status
(through the describe call, and through the convert call with a null context: the request is checked before the context is touched), the describe line,
the staged / gather decision under the LDS knob, and the pure-Python argument normalisation of VideoProcessor.convert_rois."""
import ctypes
import math
import os
import subprocess
import sys

import pytest

from util import knob_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OK, UNSUPPORTED, ERROR = 0, -2, -3
NEAREST, BILINEAR, BICUBIC, AREA = 0, 1, 2, 3
Y800, RGB24, BGR24, NV12, UYVY, YUV444, HSV = range(7)


@pytest.fixture(scope="module")
def native():
    from tensor_stream import _native
    _native.lib()
    return _native


def P(native, dst=(224, 224), rt=BILINEAR, fcc=RGB24, planes=1, norm=0, crop=(0, 0, 0, 0)):
    return native.Params(crop[0], crop[1], crop[2], crop[3], dst[0], dst[1], rt, fcc, planes, norm)


def both(native, p, frames, rois, n_frames=None, n_rois=None, null=()):
    """the status of tsvpp_describe_rois and of tsvpp_convert_rois with a NULL context for the same request: (describe, convert, text)"""
    L = native.lib()
    fr = (native.NV12 * max(len(frames), 1))(*[native.NV12(None, None, f[2] if len(f) > 2 else 0, f[3] if len(f) > 3 else (f[2] if len(f) > 2 else 0), f[0], f[1])
                                               for f in frames])
    bx = (native.Roi * max(len(rois), 1))(*[native.Roi(*r) for r in rois])
    outs = (ctypes.c_void_p * max(len(rois), 1))()
    buf = ctypes.create_string_buffer(512)
    nf = len(frames) if n_frames is None else n_frames
    nr = len(rois) if n_rois is None else n_rois
    pp = None if "p" in null else ctypes.byref(p)
    a_fr = None if "frames" in null else fr
    a_bx = None if "rois" in null else bx
    d = L.tsvpp_describe_rois(pp, nf, a_fr, nr, a_bx, 1, buf, len(buf))
    c = L.tsvpp_convert_rois(None, nf, a_fr, nr, a_bx, pp, outs, None)
    return d, c, buf.value.decode()


F1080 = (1920, 1080, 2048)


def test_symbols_signatures_and_struct_layout(native):
    L = native.lib()
    assert "tsvpp_convert_rois" in native.SYMBOLS and "tsvpp_describe_rois" in native.SYMBOLS
    assert ctypes.sizeof(native.Roi) == 20
    assert [f[0] for f in native.Roi._fields_] == ["frame", "left", "top", "right", "bottom"]
    assert native.TSVPP_MAX_ROIS == 64
    assert len(L.tsvpp_convert_rois.argtypes) == 8 and L.tsvpp_convert_rois.restype is ctypes.c_int
    assert len(L.tsvpp_describe_rois.argtypes) == 8 and L.tsvpp_describe_rois.restype is ctypes.c_int
    hdr = open(os.path.join(ROOT, "include", "tsvpp.h")).read()
    assert "#define TSVPP_MAX_ROIS 64" in hdr
    assert "int tsvpp_convert_rois(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois, const tsvpp_params *p, void *const *outs," in hdr
    assert "int tsvpp_describe_rois(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois, int aligned_outputs, char *buf," in hdr


def test_the_header_compiles_as_c_and_the_struct_is_20_bytes(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "tsvpp.h"\n_Static_assert(sizeof(tsvpp_roi) == 20, "tsvpp_roi");\nint main(void) { return TSVPP_MAX_ROIS == 64 ? 0 : 1; }\n')
    cc = os.environ.get("CC", "cc")
    subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "t"), str(src)])
    subprocess.check_call([str(tmp_path / "t")])


ERROR_CASES = {
    "null params": dict(null=("p",)),
    "null frames": dict(null=("frames",)),
    "null rois": dict(null=("rois",)),
    "n_rois zero": dict(n_rois=0),
    "n_rois negative": dict(n_rois=-1),
    "n_frames zero": dict(n_frames=0),
    "n_frames negative": dict(n_frames=-2),
    "frame index past the end": dict(rois=[(1, 0, 0, 64, 64)]),
    "frame index negative": dict(rois=[(-1, 0, 0, 64, 64)]),
    "empty box": dict(rois=[(0, 10, 10, 10, 74)]),
    "empty box (height)": dict(rois=[(0, 10, 10, 74, 10)]),
    "inverted box": dict(rois=[(0, 100, 100, 50, 164)]),
    "box past the right edge": dict(rois=[(0, 1900, 0, 1922, 64)]),
    "box past the bottom edge": dict(rois=[(0, 0, 1060, 64, 1082)]),
    "box with a negative corner": dict(rois=[(0, -2, 0, 62, 64)]),
    "second box bad": dict(rois=[(0, 0, 0, 64, 64), (0, 0, -4, 64, 60)]),
    "dst_width zero": dict(dst=(0, 224)),
    "dst_height zero": dict(dst=(224, 0)),
    "dst negative": dict(dst=(-224, 224)),
    "crop in the parameters": dict(crop=(0, 0, 64, 64)),
    "crop_left alone": dict(crop=(2, 0, 0, 0)),
    "frame without a size": dict(frames=[(0, 1080, 2048)]),
    "pitch below the width": dict(frames=[(1920, 1080, 1900)]),
}
UNSUPPORTED_CASES = {
    "odd box width": dict(rois=[(0, 0, 0, 63, 64)]),
    "odd box height": dict(rois=[(0, 0, 0, 64, 65)]),
    "odd dst_width": dict(dst=(223, 224)),
    "odd dst_height": dict(dst=(224, 223)),
    "odd frame width": dict(frames=[(1919, 1080, 2048)]),
    "odd frame height": dict(frames=[(1920, 1079, 2048)]),
    "AREA": dict(rt=AREA),
    "unknown resize type": dict(rt=7),
    "NV12 output": dict(fcc=NV12),
    "UYVY output": dict(fcc=UYVY),
    "YUV444 output": dict(fcc=YUV444),
    "HSV output": dict(fcc=HSV),
    "unknown fourcc": dict(fcc=9),
}


def _status(native, case):
    case = dict(case)
    frames = case.pop("frames", [F1080])
    rois = case.pop("rois", [(0, 0, 0, 64, 64)])
    kw = {k: case.pop(k) for k in ("n_frames", "n_rois", "null") if k in case}
    return both(native, P(native, **case), frames, rois, **kw)


@pytest.mark.parametrize("name", sorted(ERROR_CASES))
def test_invalid_arguments_are_errors(native, name):
    d, c, text = _status(native, ERROR_CASES[name])
    assert (d, c, text) == (ERROR, ERROR, "")


@pytest.mark.parametrize("name", sorted(UNSUPPORTED_CASES))
def test_unsupported_requests(native, name):
    d, c, text = _status(native, UNSUPPORTED_CASES[name])
    assert (d, c, text) == (UNSUPPORTED, UNSUPPORTED, "")


def test_a_legal_request_needs_a_context_to_convert_and_a_buffer_to_describe(native):
    d, c, text = _status(native, {})
    assert d == OK and text.startswith("mode=bilinear ")
    assert c == ERROR  # the request is fine; the context is null
    L = native.lib()
    p = P(native)
    fr = (native.NV12 * 1)(native.NV12(None, None, 2048, 2048, 1920, 1080))
    bx = (native.Roi * 1)(native.Roi(0, 0, 0, 64, 64))
    assert L.tsvpp_describe_rois(ctypes.byref(p), 1, fr, 1, bx, 1, None, 0) == ERROR
    # legal everywhere: up-scaling, full width / height, the frame itself, a 2 x 2 box, overlapping boxes, an unset pitch (= the width)
    d, c, _ = both(native, p, [(1920, 1080)], [(0, 0, 0, 1920, 1080), (0, 0, 100, 1920, 324), (0, 800, 0, 1000, 1080), (0, 1918, 1078, 1920, 1080), (0, 0, 0, 1920, 1080)])
    assert (d, c) == (OK, ERROR)


def _boxes(n, seed=3):
    import random
    r = random.Random(seed)
    out = []
    for _ in range(n):
        w, h = r.randrange(64, 513, 2), r.randrange(64, 513, 2)
        l, t = r.randrange(0, 1920 - w), r.randrange(0, 1080 - h)
        out.append((l, t, l + w, t + h))
    return out


@pytest.mark.parametrize("rt,fcc,planes,norm,mode,out", [(BILINEAR, BGR24, 0, True, "bilinear", "f32_planar"), (BICUBIC, RGB24, 1, False, "bicubic", "u8_merged"),
                                                         (NEAREST, Y800, 1, True, "nearest", "y800_f32"), (NEAREST, RGB24, 0, False, "nearest", "u8_planar"),
                                                         (BILINEAR, RGB24, 1, True, "bilinear", "f32_merged"), (BICUBIC, Y800, 0, False, "bicubic", "y800_u8")])
def test_describe_line(native, rt, fcc, planes, norm, mode, out):
    import tensor_stream as ts
    from tensor_stream import vpp
    fp = ts.FrameParameters(width=224, height=224, resize_type=rt, pixel_format=fcc, planes_pos=planes, normalization=norm)
    boxes = _boxes(33)
    d = ts.describe_rois(fp, F1080, boxes)
    limit = d["limit"]
    assert limit == native.TSVPP_MAX_ROIS
    assert d["mode"] == mode and d["out"] == out and d["dst"] == "224x224"
    assert d["rois"] == 33 and d["frames"] == 1 and d["launches"] == math.ceil(33 / limit)
    assert d["kernel"].startswith("vpp_rois<") and "_kernel<" not in d["kernel"]  # (tests/dispatch_grid.py scrapes "vpp_..._kernel<" literals: this one is not in tsvpp_describe's grid)
    assert d["tiles"] == "7x7" and d["grid"] == 49 * min(33, limit) and d["shape"] == "8x16"
    # the raw line parses with the parser of tsvpp_describe's lines
    buf = ctypes.create_string_buffer(512)
    fr = (native.NV12 * 1)(native.NV12(None, None, 2048, 2048, 1920, 1080))
    bx = (native.Roi * 33)(*[native.Roi(0, *b) for b in boxes])
    assert native.lib().tsvpp_describe_rois(ctypes.byref(fp.parameters), 1, fr, 33, bx, 1, buf, len(buf)) == OK
    assert vpp._parse_selection(buf.value.decode()) == d
    for key in ("mode", "out", "rois", "launches", "kernel", "grid", "lds", "staged"):
        assert key in d
    # 3 x limit + 5 boxes: four launches; a buffer that is too small truncates, never overruns
    many = ts.describe_rois(fp, F1080, _boxes(3 * limit + 5))
    assert many["launches"] == 4 and many["rois"] == 3 * limit + 5 and many["grid"] == 49 * limit
    small = ctypes.create_string_buffer(16)
    assert native.lib().tsvpp_describe_rois(ctypes.byref(fp.parameters), 1, fr, 33, bx, 1, small, len(small)) == OK
    assert small.raw[-1:] == b"\0" and buf.value.startswith(small.value)


def test_vector_and_element_wise_variants_and_the_tail(native):
    import tensor_stream as ts
    fp = ts.FrameParameters(width=250, height=250, resize_type=BILINEAR, pixel_format=BGR24, planes_pos=0, normalization=True)
    boxes = _boxes(5)
    a = ts.describe_rois(fp, F1080, boxes, aligned_outputs=True)
    b = ts.describe_rois(fp, F1080, boxes, aligned_outputs=False)
    assert a["kernel"].split(",")[2] == "vec" and a["tail"] == 2  # 250 = 4 k + 2: the last tile column is shifted to the right edge
    assert b["kernel"].split(",")[2] == "elem" and b["tail"] == 0
    assert a["tiles"] == "8x8"
    narrow = ts.FrameParameters(width=30, height=30, resize_type=BILINEAR, pixel_format=BGR24, planes_pos=0, normalization=True)
    c = ts.describe_rois(narrow, F1080, boxes, aligned_outputs=True)
    assert c["kernel"].split(",")[2] == "elem" and c["tail"] == 0  # narrower than a tile: no column to shift


SCRIPT = r"""
import sys
sys.path[:0] = [{root!r}, {pkg!r}]
import tensor_stream as ts
fp = ts.FrameParameters(width=224, height=224, resize_type=1, pixel_format=2, planes_pos=0, normalization=True)
d = ts.describe_rois(fp, (1920, 1080, 2048), [(100, 50, 700, 550), (300, 200, 364, 248), (0, 100, 1920, 324)])
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
    assert k.endswith(",staged>") and staged == 3 and 0 < lds <= 40 * 1024
    k0, staged0, lds0 = _describe_under({"TSVPP_DEBUG_KNOBS": "1", "TSVPP_LDS_KB": "0"})
    assert k0.endswith(",gather>") and staged0 == 0 and lds0 == 0
    # a budget that holds the small boxes only: one launch, some boxes staged
    k1, staged1, lds1 = _describe_under({"TSVPP_DEBUG_KNOBS": "1", "TSVPP_LDS_KB": "4"})
    assert k1.endswith(",staged>") and 0 < staged1 < 3 and lds1 <= 4 * 1024
    # the knob is a debug knob: ignored without the gate
    assert _describe_under({"TSVPP_LDS_KB": "0"}) == (k, staged, lds)
    assert _describe_under({"TSVPP_DEBUG_KNOBS": "1", "TSVPP_FORCE_GATHER": "1"})[1] == 0


def test_a_box_beyond_the_budget_gathers_beside_staged_ones():
    import tensor_stream as ts
    fp = ts.FrameParameters(width=112, height=112, resize_type=BICUBIC, pixel_format=RGB24, planes_pos=0, normalization=True)
    d = ts.describe_rois(fp, F1080, [(0, 0, 1920, 1080), (100, 100, 300, 300), (0, 0, 1920, 540), (7, 9, 71, 73)])
    assert d["rois"] == 4 and d["launches"] == 1
    if not knob_run():  # (a knob run moves the budget on purpose)
        assert d["kernel"].endswith(",staged>") and d["staged"] == 2


def test_python_argument_normalisation():
    from tensor_stream import vpp
    y, uv = object(), object()
    ys, uvs, boxes = vpp._normalize_rois(y, uv, [(1, 2, 33, 44)])
    assert ys == [y] and uvs == [uv] and boxes == [(0, 1, 2, 33, 44)]
    y2, uv2 = object(), object()
    ys, uvs, boxes = vpp._normalize_rois([y, y2], (uv, uv2), [(1, 0, 0, 64, 64), [2, 4, 66, 68], (0, 8, 8, 16, 16)])
    assert ys == [y, y2] and uvs == [uv, uv2] and boxes == [(1, 0, 0, 64, 64), (0, 2, 4, 66, 68), (0, 8, 8, 16, 16)]
    import numpy as np
    assert vpp._normalize_rois(y, uv, np.array([[0, 0, 10, 10]], dtype=np.int64))[2] == [(0, 0, 0, 10, 10)]
    with pytest.raises(ValueError):
        vpp._normalize_rois(y, uv, [(1, 2, 3)])
    with pytest.raises(ValueError):
        vpp._normalize_rois([y, y2], [uv], [(0, 0, 2, 2)])
    with pytest.raises(ValueError):
        vpp._normalize_rois([y, y2], uv, [(0, 0, 2, 2)])
    assert vpp._per_frame(None, 2) == [None, None] and vpp._per_frame(1920, 2) == [1920, 1920] and vpp._per_frame([1920, 1280], 2) == [1920, 1280]
    with pytest.raises(ValueError):
        vpp._per_frame([1920], 2)
    import tensor_stream as ts
    assert ts.describe_rois is vpp.describe_rois and ts.Roi is vpp.N.Roi and hasattr(ts.VideoProcessor, "convert_rois")
