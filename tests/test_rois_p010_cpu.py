"""No GPU: the host side of tsvpp_convert_rois_p010 / tsvpp_describe_rois_p010 (include/tsvpp.h) -- every status of the contract through the describe call (and
the convert call with a null context: the request is checked before the context is touched) and the describe line; and the live host path, stand-alone under
AddressSanitizer + UndefinedBehaviorSanitizer against the stub HIP runtime (tests/hostcheck/hc_rois_p010.cpp, linked by rois_p010.mk from the existing Makefile's objects)."""
import ctypes
import os
import subprocess

import pytest

import p010_util as M
from tensor_stream import _native as N

OK, UNSUPPORTED, ERROR = 0, -2, -3
TALL = 2 * (0xFFFFFFF0 // 4097 // 2 + 1)  # the pitch at which 4098 rows reach TSVPP_SOURCE_SPAN_LIMIT
ODD_LEFT, ODD_TOP = (0, 101, 60, 401, 300), (0, 100, 61, 400, 301)


def both(frames=((1920, 1080, 4096),), rois=((0, 100, 60, 400, 300),), dst=(112, 112), rt=M.BILINEAR, fcc=M.RGB24, planes=M.PLANAR, norm=1, spec=None, n=None, ptr=0, crop=0):
    # -> (status of the describe call, of the convert call with a null context, the describe line); a frame is (width, height, pitch[, chroma pitch])
    p = N.Params(crop, 0, 0, 0, dst[0], dst[1], rt, fcc, planes, norm)
    fr = (N.P010 * len(frames))(*[N.P010(ptr or None, None, f[2], f[-1], f[0], f[1]) for f in frames])
    bx = (N.Roi * max(len(rois), 1))(*[N.Roi(*b) for b in rois])
    sp = None if spec is None else ctypes.byref(N.TensorSpec(spec, (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1)))
    buf, cnt = ctypes.create_string_buffer(512), len(rois) if n is None else n
    d = N.lib().tsvpp_describe_rois_p010(ctypes.byref(p), sp, len(frames), fr, cnt, bx, 1, buf, len(buf))
    c = N.lib().tsvpp_convert_rois_p010(None, len(frames), fr, cnt, bx, ctypes.byref(p), sp, (ctypes.c_void_p * max(len(rois), 1))(), None)
    return d, c, buf.value.decode()


# tsvpp_convert_rois's rules in its order with the P010 rules in their two classes: every TSVPP_ERROR rule wins over every TSVPP_UNSUPPORTED one
REFUSED = {
    ERROR: [dict(n=0), dict(crop=2), dict(dst=(0, 112)), dict(frames=((0, 1080, 4096),)),
            dict(frames=((1920, 1080, 3838),)), dict(frames=((1920, 1080, 4096, 3838),)),   # a pitch below 2 * width, of either plane
            dict(frames=((1920, 1080, 4097),)), dict(frames=((1920, 1080, 4097),), rois=(ODD_LEFT,)),  # an odd pitch; it wins over an odd left
            dict(rois=((1, 100, 60, 400, 300),)), dict(rois=((0, 100, 60, 100, 300),)),     # a frame index out of range, an empty box
            dict(rois=((0, 100, 60, 1922, 300),)), dict(rois=((0, 100, 60, 1922, 300),), rt=2)],  # a box outside its frame; it wins over BICUBIC
    UNSUPPORTED: [dict(dst=(111, 112)), dict(frames=((1921, 1080, 4096),)), dict(rois=((0, 100, 60, 401, 300),)),  # the evenness rules of the 8-bit call
                  dict(rois=(ODD_LEFT,)), dict(rois=(ODD_TOP,)), dict(rt=2), dict(rt=3), dict(rt=9),        # this call's: an odd origin, BICUBIC (AREA, unknown)
                  dict(frames=((64, 4100, TALL),), rois=((0, 0, 2, 64, 4100),)),             # a box's plane span at the limit, seen from its origin
                  dict(fcc=3), dict(spec=1, planes=M.MERGED), dict(spec=7), dict(spec=1, norm=0)],  # NV12 output; merged tensors; tensor rules 3 and 2
}


@pytest.mark.parametrize("status,req", [(s, r) for s, rs in REFUSED.items() for r in rs])
def test_refusals(status, req):
    assert both(**req)[:2] == (status, status), req


def test_accepted_and_what_the_8bit_call_accepts():
    """describe ignores a plane pointer (the 2-byte rule needs a context: hc_rois_p010.cpp); two rows below the span limit; 65 boxes; the 8-bit call's odd origins"""
    for req in [dict(), dict(spec=1), dict(ptr=0x1001), dict(frames=((64, 4100, TALL),), rois=((0, 0, 4, 64, 4100),))]:
        assert both(**req)[:2] == (OK, ERROR), req
    d, _, text = both(frames=[(1920, 1080, 4096)] * 2, rois=[(k & 1, 2 * k, 4 * k, 2 * k + 64, 4 * k + 48) for k in range(65)], dst=(66, 34))
    assert d == OK and text.index("src=p010") < text.index("rois=65") and " launches=2 " in text and " limit=64" in text and " staged=65 " in text, text
    p, buf = N.Params(0, 0, 0, 0, 112, 112, M.BILINEAR, M.RGB24, M.PLANAR, 1), ctypes.create_string_buffer(512)
    for box in (ODD_LEFT, ODD_TOP):
        assert N.lib().tsvpp_describe_rois(ctypes.byref(p), 1, (N.NV12 * 1)(N.NV12(None, None, 2048, 2048, 1920, 1080)), 1, (N.Roi * 1)(N.Roi(*box)), 1, buf, len(buf)) == OK
        assert both(rois=(box,))[:2] == (UNSUPPORTED, UNSUPPORTED)


@pytest.mark.parametrize("req,kernel,out", [
    (dict(planes=M.MERGED, norm=0), "vpp_rois_p010<M_BILINEAR,O_U8_MERGED,vec,staged>", "u8_merged"),
    (dict(fcc=M.BGR24, rt=M.NEAREST), "vpp_rois_p010<M_NEAREST,O_F32_PLANAR,vec,staged>", "f32_planar"),
    (dict(fcc=M.Y800), "vpp_rois_p010<M_BILINEAR,O_Y800_F32,vec,staged>", "y800_f32"),
    (dict(spec=1), "vpp_rois_p010_tensor<M_BILINEAR,PLANAR,EL_HALF,vec,staged>", "f16_planar"),
    (dict(spec=0, fcc=M.Y800), "vpp_rois_p010_tensor<M_BILINEAR,Y800,EL_F32,vec,staged>", "f32n_y800")])
def test_describe_kernel(req, kernel, out):
    d, _, text = both(rois=((0, 100, 60, 164, 124),), dst=(64, 64), **req)
    assert d == OK and f" kernel={kernel} " in text and f" out={out} " in text and " src=p010 " in text and text.endswith(" limit=64"), text


def test_host_path_under_asan_ubsan():
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run(["make", "-s", "-C", os.path.join(here, "hostcheck"), "-f", "rois_p010.mk", "-j16", "rois_p010"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, f"tests/hostcheck/rois_p010.mk does not build:\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    exe = os.path.join(os.path.dirname(here), "tensor-stream_amd", "lib", "hostcheck", "asan", "hc_rois_p010")
    r = subprocess.run(["timeout", "-k", "5", "300", exe], capture_output=True, text=True, timeout=330)
    assert r.returncode == 0 and " assertions, 0 failed" in r.stderr, f"status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-12000:]}"
