"""No GPU: tsvpp_convert_letterbox_p010_area's arithmetic and host side (include/tsvpp.h) -- the numpy model (tests/p010_area_util.py) against the exact rational
mean, tsvpp_box_p010_plane (the kernel's own functions, compiled for the host) against the model bit for bit, the describe line, every refusal, and the live host
path stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer against the stub HIP runtime (tests/hostcheck/hc_letterbox_p010_area.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import p010_area_util as A
import p010_util as M
from tensor_stream import _native as N

OK, UNSUPPORTED, ERROR = 0, -2, -3
# source size -> output size
GEOMETRIES = [((1920, 1080), (640, 360)), ((3840, 2160), (640, 360)), ((1366, 768), (640, 360)), ((8192, 4320), (480, 254)), ((50, 38), (32, 30)), ((7, 5), (6, 4))]
# the integer bounds: flat 1023 at the longest side either way, and the ramp of all codes at equal size
BOUNDARY = [((16384, 2), (1024, 2), 1023), ((2, 16384), (2, 1024), 1023), ((32, 32), (32, 32), None)]


def plane(size, seed, flat=None):
    w, h = size
    if flat is not None:
        return np.full((h, w), flat, np.uint16)
    if seed is None:
        return np.arange(w * h, dtype=np.uint16).reshape(h, w) % 1024
    return np.random.default_rng(seed).integers(0, 1024, (h, w), dtype=np.uint16)


@pytest.fixture(scope="module")
def planes():
    return {g: plane(g[0], 7 + k) for k, g in enumerate(GEOMETRIES)}


@pytest.mark.parametrize("src,dst", GEOMETRIES)
def test_model_is_within_half_plus_1_128_of_the_rational_mean(planes, src, dst):
    """0.5 from the final rounding, 1/128 from the rounding of the row means to 1/64 steps; flat frames come back unchanged"""
    S = planes[(src, dst)]
    assert np.abs(A.box(S, *dst) - A.box(S, *dst, exact=True)).max() <= 0.5 + 1 / 128 + 1e-9
    for v in (0, 512, 1023) if src[0] < 3840 else ():
        assert np.array_equal(A.box(plane(src, 0, flat=v), *dst), np.full(dst[::-1], v))


def native_box(S, dst):
    S = np.ascontiguousarray(S, np.uint16)
    out = np.empty(dst[::-1], np.uint16)
    sts = N.lib().tsvpp_box_p010_plane(S.ctypes.data, S.shape[1], S.shape[0], out.ctypes.data, dst[0], dst[1])
    return sts, out


@pytest.mark.parametrize("src,dst,flat", [(*g, 0) for g in GEOMETRIES] + BOUNDARY)
def test_native_plane_equals_the_model(planes, src, dst, flat):
    S = planes[(src, dst)] if flat == 0 else plane(src, None, flat)
    sts, got = native_box(S, dst)
    assert sts == OK and np.array_equal(got, A.box(S, *dst))


def both(frames=((1920, 1080, 4096),), dst=(640, 640), rects=None, rt=A.AREA, fcc=M.RGB24, planes=M.PLANAR, norm=1, spec=None, pad=(64, 512, 512)):
    # -> (status of the describe call, of the convert call with a null context, the describe line); a frame is (width, height, pitch)
    p = N.Params(0, 0, 0, 0, dst[0], dst[1], rt, fcc, planes, norm)
    fr = (N.P010 * len(frames))(*[N.P010(None, None, f[2], f[2], f[0], f[1]) for f in frames])
    rc = None if rects is None else (N.Rect * len(rects))(*[N.Rect(*r) for r in rects])
    sp = None if spec is None else ctypes.byref(N.TensorSpec(spec, (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1)))
    buf = ctypes.create_string_buffer(512)
    d = N.lib().tsvpp_describe_letterbox_p010_area(ctypes.byref(p), sp, len(frames), fr, rc, 1, buf, len(buf))
    c = N.lib().tsvpp_convert_letterbox_p010_area(None, len(frames), fr, ctypes.byref(p), sp, rc, *pad, (ctypes.c_void_p * len(frames))(), None)
    return d, c, buf.value.decode()


@pytest.mark.parametrize("req,kernel,taps", [
    (dict(), "vpp_letterbox_p010_area<O_F32_PLANAR,vec>", "3x3"),
    (dict(frames=((3840, 2160, 8192),), planes=M.MERGED, norm=0), "vpp_letterbox_p010_area<O_U8_MERGED,vec>", "6x6"),
    (dict(frames=((3840, 2160, 8192),), spec=1), "vpp_letterbox_p010_area_tensor<PLANAR,EL_HALF,vec>", "6x6")])
def test_describe_1080p_and_4k_into_640(req, kernel, taps):
    d, c, text = both(**req)
    keys = dict(item.partition("=")[::2] for item in text.split(" "))
    assert (d, c) == (OK, ERROR) and keys["kernel"] == kernel and keys["mode"] == "area" and keys["src"] == "p010" and keys["taps"] == taps, text
    assert keys["inner"] == "640x360+0+140" and keys["grid"] == "400" and keys["limit"] == "32" and keys["staged"] == "1", text
    # two band buffers and the row means of one band, inside the 40 KiB budget, with a band of more than one row
    assert 1 < int(keys["band"]) <= 32 and int(keys["lds"]) <= 40 * 1024, text


@pytest.mark.parametrize("status,req", [
    (UNSUPPORTED, dict(rt=M.BILINEAR)), (UNSUPPORTED, dict(rt=M.NEAREST)), (UNSUPPORTED, dict(rt=2)),  # any type but AREA
    (UNSUPPORTED, dict(frames=((16386, 1080, 32772),))),                                              # a side above TSVPP_BOX_P010_MAX_SIDE
    (UNSUPPORTED, dict(frames=((546, 64, 1092),), dst=(32, 32), rects=((0, 0, 32, 32),))),              # 18 taps: 546 -> 32 with gcd 2
    (ERROR, dict(pad=(1024, 512, 512))), (ERROR, dict(pad=(1024, 512, 512), rt=M.BILINEAR))])           # inherited: a pad above ten bits; it wins over the type
def test_refusals(status, req):
    """describe and convert alike -- except the pad, which is no argument of the describe call: it answers as for the request without it"""
    d, c, _ = both(**req)
    assert c == status and d == (both(**{k: v for k, v in req.items() if k != "pad"})[0] if "pad" in req else status), req


def test_the_tap_limit_itself_and_the_existing_call():
    """17 taps (514 -> 32 with gcd 2) and a side of 16384 are served; tsvpp_convert_letterbox_p010 keeps refusing AREA"""
    assert both(frames=((514, 64, 1028),), dst=(32, 32), rects=((0, 0, 32, 32),))[0] == OK
    assert both(frames=((16384, 1080, 32768),), dst=(1024, 68))[0] == OK
    p, fr, buf = N.Params(0, 0, 0, 0, 640, 640, A.AREA, M.RGB24, M.PLANAR, 1), (N.P010 * 1)(N.P010(None, None, 4096, 4096, 1920, 1080)), ctypes.create_string_buffer(512)
    assert N.lib().tsvpp_describe_letterbox_p010(ctypes.byref(p), None, 1, fr, None, 1, buf, len(buf)) == UNSUPPORTED


def test_host_path_under_asan_ubsan():
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run(["make", "-s", "-C", os.path.join(here, "hostcheck"), "-f", "letterbox_p010_area.mk", "-j16", "letterbox_p010_area"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, f"tests/hostcheck/letterbox_p010_area.mk does not build:\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    exe = os.path.join(os.path.dirname(here), "tensor-stream_amd", "lib", "hostcheck", "asan", "hc_letterbox_p010_area")
    r = subprocess.run(["timeout", "-k", "5", "300", exe], capture_output=True, text=True, timeout=330)
    assert r.returncode == 0 and " assertions, 0 failed" in r.stderr, f"status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-12000:]}"
