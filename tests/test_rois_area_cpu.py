"""No GPU: the host side of tsvpp_convert_rois_area / tsvpp_describe_rois_area / tsvpp_roi_area_rows (include/tsvpp.h).

The weight-row generator the AREA ROI kernel runs per tile (roi_area_step, csrc/vpp_rois.h: a __host__ __device__ function) is evaluated on the host through the
debug export and compared, on raw bits, with rows[j % rows] of the library's table (tsvpp_area_pattern) and with the oracle's restatement of the reference's
generateResizePattern; then every validation status of tests/test_rois_cpu.py through the AREA describe call, and the describe line."""
import ctypes
import math

import numpy as np
import pytest

import test_rois_cpu as base
from test_rois_cpu import AREA, BGR24, BICUBIC, BILINEAR, ERROR, F1080, NEAREST, OK, RGB24, UNSUPPORTED, Y800, P

MAX_TAPS = 40  # ROI_AREA_MAX_TAPS (csrc/vpp_rois.h)


@pytest.fixture(scope="module")
def native():
    from tensor_stream import _native
    _native.lib()
    return _native


def gen_rows(native, scale, first, n):
    taps = ctypes.c_int(0)
    t = int(math.ceil(float(scale)))
    buf = np.full(n * t + 8, np.float32(-7.0))  # (guard floats behind the rows)
    got = native.lib().tsvpp_roi_area_rows(ctypes.c_float(scale), first, n, buf.ctypes.data, n * t, ctypes.byref(taps))
    assert got == n and taps.value == t, (scale, first, n, got, taps.value)
    assert np.all(buf[n * t:] == np.float32(-7.0))
    return buf[:n * t].reshape(n, t)


def table_rows(native, scale):
    buf = np.zeros(1 << 21, np.float32)
    taps = ctypes.c_int(0)
    rows = native.lib().tsvpp_area_pattern(ctypes.c_float(scale), buf.ctypes.data, buf.size, ctypes.byref(taps))
    assert rows > 0 and rows * taps.value <= buf.size
    return buf[:rows * taps.value].reshape(rows, taps.value)


def _seeded_scales():
    rng = np.random.default_rng(20261018)
    out = []
    for k in range(60):
        w = 2 * int(rng.integers(1, 257))  # even widths 2 .. 512
        d = (112, 224, 250)[k % 3]
        if w > d:
            out.append((w, d))
    return out


SCALES = [(448, 224), (336, 224), (300, 224), (226, 224), (302, 224), (500, 112), (1920, 112), (1080, 30)] + _seeded_scales()


@pytest.mark.parametrize("w,d", SCALES)
def test_generator_rows_equal_the_table_and_the_oracle(native, oracle, w, d):
    scale = np.float32(w) / np.float32(d)
    assert int(math.ceil(float(scale))) <= MAX_TAPS
    tab = table_rows(native, scale)
    taps = tab.shape[1]
    ref = oracle.area_pattern(float(scale))[:, :taps]
    assert ref.shape == tab.shape
    for first, n in [(0, 512), (0, 32), (31, 32), (32, 32), (250 - 32, 32)]:
        rows = gen_rows(native, scale, first, n)
        idx = (np.arange(first, first + n)) % tab.shape[0]
        assert np.array_equal(rows.view(np.uint32), tab[idx].view(np.uint32)), (w, d, first, n)
        assert np.array_equal(rows.view(np.uint32), ref[idx].view(np.uint32)), (w, d, first, n)


def test_the_named_scales_have_the_periods_the_cases_are_there_for(native):
    period = lambda w, d: table_rows(native, np.float32(w) / np.float32(d)).shape[0]
    assert period(448, 224) == 1 and period(336, 224) == 2 and period(300, 224) == 56
    assert table_rows(native, np.float32(226) / np.float32(224)).shape[1] == 2
    assert period(302, 224) == 112 and period(226, 224) == 112 and period(500, 112) == 28  # wrap inside a tile column, away from every tile boundary but one
    assert table_rows(native, np.float32(1920) / np.float32(112)).shape[1] == 18
    assert table_rows(native, np.float32(1080) / np.float32(30)).shape[1] == 36
    assert len(_seeded_scales()) >= 30


def test_generator_argument_checks(native):
    L = native.lib()
    buf = np.zeros(256, np.float32)
    taps = ctypes.c_int(0)
    call = lambda scale, first, n, out=buf.ctypes.data, cap=buf.size: L.tsvpp_roi_area_rows(ctypes.c_float(scale), first, n, out, cap, ctypes.byref(taps))
    assert call(1.5, 0, 4) == 4 and taps.value == 2
    assert L.tsvpp_roi_area_rows(ctypes.c_float(1.5), 0, 4, buf.ctypes.data, buf.size, None) == 4
    assert call(1.0, 0, 4) == UNSUPPORTED and call(0.5, 0, 4) == UNSUPPORTED
    assert call(40.5, 0, 1) == UNSUPPORTED and call(40.0, 0, 1) == 1  # 41 taps / 40 taps
    assert call(1.5, 65536 - 3, 4) == UNSUPPORTED
    assert call(1.5, -1, 4) == ERROR and call(1.5, 0, 0) == ERROR and call(1.5, 0, 4, out=None) == ERROR
    assert call(1.5, 0, 4, cap=7) == ERROR


def both(native, p, frames, rois, n_frames=None, n_rois=None, null=()):
    """test_rois_cpu.both for the AREA entry points: (describe status, convert status with a NULL context, describe text)"""
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
    d = L.tsvpp_describe_rois_area(pp, nf, a_fr, nr, a_bx, 1, buf, len(buf))
    c = L.tsvpp_convert_rois_area(None, nf, a_fr, nr, a_bx, pp, outs, None)
    return d, c, buf.value.decode()


def _status(native, case):
    case = dict(case)
    frames = case.pop("frames", [F1080])
    rois = case.pop("rois", [(0, 0, 0, 64, 64)])
    kw = {k: case.pop(k) for k in ("n_frames", "n_rois", "null") if k in case}
    case.setdefault("rt", AREA)
    return both(native, P(native, **case), frames, rois, **kw)


@pytest.mark.parametrize("name", sorted(base.ERROR_CASES))
def test_invalid_arguments_are_errors(native, name):
    assert _status(native, base.ERROR_CASES[name]) == (ERROR, ERROR, "")


AREA_UNSUPPORTED = {k: v for k, v in base.UNSUPPORTED_CASES.items() if k != "AREA"}
AREA_UNSUPPORTED.update({
    "NEAREST": dict(rt=NEAREST),
    "BILINEAR": dict(rt=BILINEAR),
    "BICUBIC": dict(rt=BICUBIC),
    "41 taps on x": dict(dst=(46, 224), rois=[(0, 0, 0, 1920, 448)]),        # 1920 / 46 = 41.7
    "41 taps on y": dict(dst=(224, 26), rois=[(0, 0, 0, 448, 1080)]),        # 1080 / 26 = 41.5
    "second box above the cap": dict(dst=(30, 30), rois=[(0, 0, 0, 64, 64), (0, 0, 0, 1920, 1080)]),
    "dst_width above 65536": dict(dst=(65538, 2)),
    "dst_height above 65536": dict(dst=(2, 65538)),
})


@pytest.mark.parametrize("name", sorted(AREA_UNSUPPORTED))
def test_unsupported_requests(native, name):
    assert _status(native, AREA_UNSUPPORTED[name]) == (UNSUPPORTED, UNSUPPORTED, "")


def test_area_is_ok_here_and_still_unsupported_there(native):
    d, c, text = _status(native, {})
    assert d == OK and c == ERROR and text.startswith("mode=area ")  # the request is fine; the context is null
    assert base.both(native, P(native, rt=AREA), [F1080], [(0, 0, 0, 64, 64)]) == (UNSUPPORTED, UNSUPPORTED, "")
    # at the cap, and a box above it that runs the up-scale rule (down on x only): fine
    assert _status(native, dict(dst=(48, 224), rois=[(0, 0, 0, 1920, 448)]))[0] == OK        # 40 taps
    assert _status(native, dict(dst=(30, 224), rois=[(0, 0, 0, 1920, 100)]))[0] == OK        # 64 on x, up on y: the 2 x 2 blend
    assert _status(native, dict(dst=(65536, 2)))[0] == OK
    import tensor_stream as ts
    fp = ts.FrameParameters(width=224, height=224, resize_type=AREA)
    with pytest.raises(RuntimeError, match="-2"):
        ts.describe_rois(fp, F1080, [(0, 0, 448, 448)])
    assert ts.describe_rois_area(fp, F1080, [(0, 0, 448, 448)])["down"] == 1
    assert hasattr(ts.VideoProcessor, "convert_rois_area")


def test_symbols_and_header(native):
    import os
    L = native.lib()
    for sym in ("tsvpp_convert_rois_area", "tsvpp_describe_rois_area", "tsvpp_roi_area_rows"):
        assert sym in native.SYMBOLS
    assert len(L.tsvpp_convert_rois_area.argtypes) == 8 and len(L.tsvpp_describe_rois_area.argtypes) == 8 and len(L.tsvpp_roi_area_rows.argtypes) == 6
    hdr = open(os.path.join(base.ROOT, "include", "tsvpp.h")).read()
    assert f"#define TSVPP_MAX_ROIS_AREA {native.TSVPP_MAX_ROIS_AREA}" in hdr
    assert "int tsvpp_roi_area_rows(float scale, int first, int n, float *out, int max_floats, int *taps);" in hdr


def test_describe_line(native):
    import tensor_stream as ts
    from tensor_stream import vpp
    limit = native.TSVPP_MAX_ROIS_AREA
    fp = ts.FrameParameters(width=224, height=224, resize_type=AREA, pixel_format=BGR24, planes_pos=0, normalization=True)
    for n in (1, limit, limit + 1):
        boxes = base._boxes(n)
        d = ts.describe_rois_area(fp, F1080, boxes)
        down = sum(1 for l, t, r, b in boxes if r - l > 224 and b - t > 224)
        tx = max([math.ceil((r - l) / 224) for l, t, r, b in boxes if r - l > 224 and b - t > 224], default=0)
        ty = max([math.ceil((b - t) / 224) for l, t, r, b in boxes if r - l > 224 and b - t > 224], default=0)
        assert d["mode"] == "area" and d["out"] == "f32_planar" and d["dst"] == "224x224" and d["rois"] == n and d["frames"] == 1
        assert d["limit"] == limit and d["launches"] == math.ceil(n / limit) and d["grid"] == 49 * min(n, limit)
        assert d["down"] == down and d["taps"] == f"{tx}x{ty}"
        assert d["kernel"].startswith("vpp_rois_area<O_F32_PLANAR,vec,") and "_kernel<" not in d["kernel"]
        assert d["tiles"] == "7x7" and d["shape"] == "8x16"
    # the raw line parses with the parser of tsvpp_describe's lines; its keys are tsvpp_describe_rois's, then down= and taps=
    bil = ts.describe_rois(ts.FrameParameters(width=224, height=224, resize_type=BILINEAR, pixel_format=BGR24, planes_pos=0, normalization=True), F1080, base._boxes(3))
    mixed = [(100, 50, 700, 550), (300, 200, 364, 248), (1000, 500, 1800, 600)]  # down-scale, up-scale, down on x only
    d = ts.describe_rois_area(fp, F1080, mixed)
    assert list(d)[:len(bil)] == list(bil) and list(d)[len(bil):] == ["down", "taps"]
    assert d["down"] == 1 and d["taps"] == "3x3" and d["launches"] == 1 and d["rois"] == 3
    buf = ctypes.create_string_buffer(512)
    fr = (native.NV12 * 1)(native.NV12(None, None, 2048, 2048, 1920, 1080))
    bx = (native.Roi * 3)(*[native.Roi(0, *b) for b in mixed])
    assert native.lib().tsvpp_describe_rois_area(ctypes.byref(fp.parameters), 1, fr, 3, bx, 1, buf, len(buf)) == OK
    assert vpp._parse_selection(buf.value.decode()) == d
    # no down-scale box at all; the weight rows are part of lds=
    up = ts.describe_rois_area(fp, F1080, [(300, 200, 364, 248), (0, 0, 224, 224)])
    assert up["down"] == 0 and up["taps"] == "0x0"
    one = ts.describe_rois_area(fp, F1080, [(0, 0, 448, 448)])
    two = ts.describe_rois_area(fp, F1080, [(0, 0, 448, 448), (0, 0, 1920, 1080)])  # 9 x 5 taps: more weight rows, and a box that gathers
    assert one["taps"] == "2x2" and two["taps"] == "9x5" and two["lds"] > one["lds"] >= 4 * 49 * 6
    # a buffer that is too small truncates, never overruns
    small = ctypes.create_string_buffer(16)
    assert native.lib().tsvpp_describe_rois_area(ctypes.byref(fp.parameters), 1, fr, 3, bx, 1, small, len(small)) == OK
    assert small.raw[-1:] == b"\0" and buf.value.startswith(small.value)


def test_y800_and_element_wise_variants(native):
    import tensor_stream as ts
    boxes = base._boxes(5)
    fp = ts.FrameParameters(width=250, height=250, resize_type=AREA, pixel_format=Y800, planes_pos=1, normalization=False)
    a = ts.describe_rois_area(fp, F1080, boxes, aligned_outputs=True)
    b = ts.describe_rois_area(fp, F1080, boxes, aligned_outputs=False)
    assert a["kernel"].startswith("vpp_rois_area<O_Y800_U8,vec,") and a["tail"] == 2
    assert b["kernel"].startswith("vpp_rois_area<O_Y800_U8,elem,") and b["tail"] == 0
    narrow = ts.FrameParameters(width=30, height=30, resize_type=AREA, pixel_format=RGB24, planes_pos=1, normalization=False)
    assert ts.describe_rois_area(narrow, F1080, boxes)["kernel"].startswith("vpp_rois_area<O_U8_MERGED,elem,")
