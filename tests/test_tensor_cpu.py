"""No GPU: the tensor entry points (tsvpp_tensor_bytes, tsvpp_describe_rois_tensor, tsvpp_describe_letterbox_tensor; include/tsvpp.h) -- the ABI of the spec, the
size function, every status rule and its order (the plan's status wins, then TSVPP_ERROR for the spec, then TSVPP_UNSUPPORTED), the describe strings per dtype,
AREA behind the one ROI name, the Python facade's scale, and tensor_util (what the GPU tests compare against) on the identity spec."""
import ctypes

import numpy as np
import pytest
import torch

import tensor_util as T
from util import synth_nv12

NEAREST, BILINEAR, BICUBIC, AREA = 0, 1, 2, 3
Y800, RGB24, BGR24, NV12, UYVY, YUV444, HSV = 0, 1, 2, 3, 4, 5, 6
PLANAR, MERGED = 0, 1
OK, ERROR, UNSUPPORTED = 0, -3, -2
W, H = 1920, 1080


@pytest.fixture(scope="module")
def native():
    from tensor_stream import _native
    _native.lib()
    return _native


def spec_of(N, dtype=1, mean=(0.5, 0.5, 0.5), scale=(2.0, 2.0, 2.0)):
    return N.TensorSpec(dtype, (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*scale))


def params_of(N, dst=(224, 224), rt=BILINEAR, fcc=RGB24, planes=PLANAR, norm=1, crop=(0, 0, 0, 0)):
    return N.Params(crop[0], crop[1], crop[2], crop[3], dst[0], dst[1], rt, fcc, planes, norm)


def rois_status(N, p, spec, boxes=((0, 100, 50, 400, 350),), frame=(W, H), aligned=1):
    fr = (N.NV12 * 1)(N.NV12(None, None, 0, 0, frame[0], frame[1]))
    bx = (N.Roi * len(boxes))(*[N.Roi(*b) for b in boxes])
    buf = ctypes.create_string_buffer(512)
    sts = N.lib().tsvpp_describe_rois_tensor(ctypes.byref(p), None if spec is None else ctypes.byref(spec), 1, fr, len(boxes), bx, aligned, buf, len(buf))
    return sts, buf.value.decode()


def letterbox_status(N, p, spec, frame=(W, H), rects=None, aligned=1):
    fr = (N.NV12 * 1)(N.NV12(None, None, 0, 0, frame[0], frame[1]))
    rc = None if rects is None else (N.Rect * 1)(N.Rect(*rects[0]))
    buf = ctypes.create_string_buffer(512)
    sts = N.lib().tsvpp_describe_letterbox_tensor(ctypes.byref(p), None if spec is None else ctypes.byref(spec), 1, fr, rc, aligned, buf, len(buf))
    return sts, buf.value.decode()


BOTH = [rois_status, letterbox_status]


def test_spec_layout_and_codes(native):
    assert ctypes.sizeof(native.TensorSpec) == 28
    assert (native.TSVPP_F32, native.TSVPP_F16, native.TSVPP_BF16) == (0, 1, 2)
    assert native.TensorSpec.mean.offset == 4 and native.TensorSpec.scale.offset == 16
    assert T.CODE == {T.F32: 0, T.F16: 1, T.BF16: 2}


def test_tensor_bytes(native):
    L = native.lib()

    def nbytes(p, s):
        return L.tsvpp_tensor_bytes(None if p is None else ctypes.byref(p), None if s is None else ctypes.byref(s))

    for dt, esz in ((0, 4), (1, 2), (2, 2)):
        assert nbytes(params_of(native), spec_of(native, dt)) == 3 * 224 * 224 * esz
        assert nbytes(params_of(native, fcc=BGR24, dst=(70, 66)), spec_of(native, dt)) == 3 * 70 * 66 * esz
        assert nbytes(params_of(native, fcc=Y800, planes=MERGED, dst=(30, 34)), spec_of(native, dt)) == 30 * 34 * esz
    # a refused pair: 0
    assert nbytes(params_of(native), None) == 0 and nbytes(None, spec_of(native)) == 0
    assert nbytes(params_of(native), spec_of(native, 3)) == 0
    assert nbytes(params_of(native, norm=0), spec_of(native)) == 0
    assert nbytes(params_of(native, planes=MERGED), spec_of(native)) == 0
    assert nbytes(params_of(native, fcc=NV12), spec_of(native)) == 0
    assert nbytes(params_of(native), spec_of(native, scale=(1.0, 0.0, 1.0))) == 0
    assert nbytes(params_of(native, dst=(224, 223)), spec_of(native)) == 0 and nbytes(params_of(native, dst=(0, 224)), spec_of(native)) == 0
    assert nbytes(params_of(native, dst=(32768, 32768)), spec_of(native)) == 0  # 4 GiB or more as fp32, the plans' limit


@pytest.mark.parametrize("status", BOTH)
def test_an_accepted_request(native, status):
    for dt in (0, 1, 2):
        for fcc, planes in ((RGB24, PLANAR), (BGR24, PLANAR), (Y800, MERGED), (Y800, PLANAR)):
            sts, _ = status(native, params_of(native, fcc=fcc, planes=planes), spec_of(native, dt))
            assert sts == OK, (dt, fcc, planes)


@pytest.mark.parametrize("status", BOTH)
def test_spec_errors(native, status):
    """rule 2: TSVPP_ERROR for a null spec, a non-finite mean or scale, a zero scale -- in a channel the format uses"""
    p = params_of(native)
    assert status(native, p, None)[0] == ERROR
    for bad in (float("nan"), float("inf"), -float("inf")):
        for c in range(3):
            m, s = [0.5] * 3, [2.0] * 3
            m[c] = bad
            assert status(native, p, spec_of(native, mean=m))[0] == ERROR, (bad, c)
            s[c] = bad
            assert status(native, p, spec_of(native, scale=s))[0] == ERROR, (bad, c)
    for c in range(3):
        s = [2.0] * 3
        s[c] = 0.0
        assert status(native, p, spec_of(native, scale=s))[0] == ERROR
        s[c] = -0.0
        assert status(native, p, spec_of(native, scale=s))[0] == ERROR
    # Y800 uses channel 0 alone: channels 1 and 2 may hold anything
    y = params_of(native, fcc=Y800, planes=MERGED)
    assert status(native, y, spec_of(native, mean=(0.5, float("nan"), float("inf")), scale=(2.0, 0.0, float("nan"))))[0] == OK
    assert status(native, y, spec_of(native, scale=(0.0, 1.0, 1.0)))[0] == ERROR
    assert status(native, y, spec_of(native, mean=(float("nan"), 0.0, 0.0)))[0] == ERROR


@pytest.mark.parametrize("status", BOTH)
def test_unsupported_pairs(native, status):
    """rule 3: an unknown dtype, normalization == 0, MERGED with RGB24 / BGR24 (a fourcc outside RGB24 / BGR24 / Y800 is the plan's own TSVPP_UNSUPPORTED already)"""
    assert status(native, params_of(native), spec_of(native, 3))[0] == UNSUPPORTED
    assert status(native, params_of(native), spec_of(native, -1))[0] == UNSUPPORTED
    assert status(native, params_of(native, norm=0), spec_of(native))[0] == UNSUPPORTED
    assert status(native, params_of(native, fcc=Y800, norm=0), spec_of(native))[0] == UNSUPPORTED
    assert status(native, params_of(native, planes=MERGED), spec_of(native))[0] == UNSUPPORTED
    assert status(native, params_of(native, fcc=BGR24, planes=MERGED), spec_of(native))[0] == UNSUPPORTED
    for fcc in (NV12, UYVY, YUV444, HSV):
        assert status(native, params_of(native, fcc=fcc), spec_of(native))[0] == UNSUPPORTED, fcc
    # rule 2 comes before rule 3
    assert status(native, params_of(native, norm=0), spec_of(native, 3, scale=(0.0, 1.0, 1.0)))[0] == ERROR
    assert status(native, params_of(native, planes=MERGED), None)[0] == ERROR


def test_the_plans_status_wins(native):
    """rule 1: whatever the existing entry point answers for the request comes first, bad spec or not"""
    N = native
    bad_specs = [None, spec_of(N, 3), spec_of(N, scale=(0.0, 0.0, 0.0)), spec_of(N, mean=(float("nan"),) * 3)]
    for s in bad_specs + [spec_of(N)]:
        # ROIs: an odd box is TSVPP_UNSUPPORTED, a box outside its frame TSVPP_ERROR, a crop in the parameters TSVPP_ERROR, an odd output TSVPP_UNSUPPORTED
        assert rois_status(N, params_of(N), s, boxes=((0, 0, 0, 101, 100),))[0] == UNSUPPORTED
        assert rois_status(N, params_of(N), s, boxes=((0, 0, 0, W + 2, 100),))[0] == ERROR
        assert rois_status(N, params_of(N, crop=(0, 0, 64, 64)), s)[0] == ERROR
        assert rois_status(N, params_of(N, dst=(224, 223)), s)[0] == UNSUPPORTED
        assert rois_status(N, params_of(N, rt=7), s)[0] == UNSUPPORTED
        # AREA's own limit: more than 40 taps on an axis
        assert rois_status(N, params_of(N, rt=AREA, dst=(32, 32)), s, boxes=((0, 0, 0, 1920, 64),))[0] == UNSUPPORTED
        # letterbox: AREA is TSVPP_UNSUPPORTED there, a rectangle outside the canvas TSVPP_ERROR, an odd rectangle TSVPP_UNSUPPORTED
        assert letterbox_status(N, params_of(N, rt=AREA), s)[0] == UNSUPPORTED
        assert letterbox_status(N, params_of(N), s, rects=[(0, 0, 226, 2)])[0] == ERROR
        assert letterbox_status(N, params_of(N), s, rects=[(0, 0, 21, 2)])[0] == UNSUPPORTED
    # an odd box (the plan: TSVPP_UNSUPPORTED) with a null spec (rule 2: TSVPP_ERROR): the plan's
    assert rois_status(N, params_of(N), None, boxes=((0, 1, 1, 100, 100),))[0] == UNSUPPORTED
    # the same requests with the existing entry points answer the same status
    fr = (N.NV12 * 1)(N.NV12(None, None, 0, 0, W, H))
    bx = (N.Roi * 1)(N.Roi(0, 0, 0, 101, 100))
    buf = ctypes.create_string_buffer(512)
    assert N.lib().tsvpp_describe_rois(ctypes.byref(params_of(N)), 1, fr, 1, bx, 1, buf, len(buf)) == UNSUPPORTED


@pytest.mark.parametrize("dt,name", [(0, "f32n"), (1, "f16"), (2, "bf16")])
def test_describe_strings_per_dtype(native, dt, name):
    import tensor_stream as ts
    el = "EL_F32" if dt == 0 else "EL_HALF"
    for fcc, planes, flav, knd in ((RGB24, PLANAR, "planar", "PLANAR"), (BGR24, PLANAR, "planar", "PLANAR"), (Y800, MERGED, "y800", "Y800")):
        sts, line = rois_status(native, params_of(native, fcc=fcc, planes=planes), spec_of(native, dt))
        assert sts == OK
        d = ts.vpp._parse_selection(line)
        assert d["out"] == f"{name}_{flav}" and d["mode"] == "bilinear" and d["limit"] == 64 and d["rois"] == 1 and d["dst"] == "224x224"
        assert d["kernel"] == f"vpp_rois_tensor<M_BILINEAR,{knd},{el},vec,staged>", d["kernel"]
        # the existing call on the same request: the same keys, the same launch geometry (the staged footprint is source bytes: lds= does not depend on the element)
        fr = (native.NV12 * 1)(native.NV12(None, None, 0, 0, W, H))
        bx = (native.Roi * 1)(native.Roi(0, 100, 50, 400, 350))
        buf = ctypes.create_string_buffer(512)
        assert native.lib().tsvpp_describe_rois(ctypes.byref(params_of(native, fcc=fcc, planes=planes)), 1, fr, 1, bx, 1, buf, len(buf)) == OK
        e = ts.vpp._parse_selection(buf.value.decode())
        assert list(d) == list(e)
        assert {k: d[k] for k in d if k not in ("out", "kernel")} == {k: e[k] for k in e if k not in ("out", "kernel")}
        sts, line = letterbox_status(native, params_of(native, fcc=fcc, planes=planes, dst=(640, 640)), spec_of(native, dt))
        assert sts == OK
        d = ts.vpp._parse_selection(line)
        assert d["out"] == f"{name}_{flav}" and d["limit"] == 32 and d["inner"] == "640x360+0+140"
        assert d["kernel"] == f"vpp_letterbox_tensor<M_BILINEAR,{knd},{el},vec,staged>", d["kernel"]
    # outputs that are not 16-byte aligned, and a width 4 k + 2 below a tile: the element-wise kernel; 4 k + 2 from a tile on: the shifted tile column
    d = ts.vpp._parse_selection(rois_status(native, params_of(native), spec_of(native, dt), aligned=0)[1])
    assert d["kernel"].split(",")[3] == "elem" and d["tail"] == 0
    d = ts.vpp._parse_selection(rois_status(native, params_of(native, dst=(30, 34)), spec_of(native, dt))[1])
    assert d["kernel"].split(",")[3] == "elem"
    d = ts.vpp._parse_selection(rois_status(native, params_of(native, dst=(70, 66)), spec_of(native, dt))[1])
    assert d["kernel"].split(",")[3] == "vec" and d["tail"] == 2


def test_area_behind_the_one_roi_name(native):
    """tsvpp_describe_rois_tensor accepts all four resize types; AREA runs the vpp_rois_area kernel with that call's keys and limits"""
    import tensor_stream as ts
    for dt, el in ((0, "EL_F32"), (1, "EL_HALF"), (2, "EL_HALF")):
        sts, line = rois_status(native, params_of(native, rt=AREA), spec_of(native, dt), boxes=((0, 100, 50, 700, 550), (0, 300, 200, 364, 248)))
        assert sts == OK
        d = ts.vpp._parse_selection(line)
        assert d["mode"] == "area" and d["kernel"].startswith("vpp_rois_area") and d["kernel"] == f"vpp_rois_area_tensor<PLANAR,{el},vec,staged>"
        assert d["down"] == 1 and d["taps"] == "3x3" and d["limit"] == 64
    for rt, m in ((NEAREST, "M_NEAREST"), (BILINEAR, "M_BILINEAR"), (BICUBIC, "M_BICUBIC")):
        sts, line = rois_status(native, params_of(native, rt=rt), spec_of(native, 1))
        assert sts == OK and f"kernel=vpp_rois_tensor<{m}," in line
    # 40 taps are accepted, 41 are not; a side of 65536 is the limit
    assert rois_status(native, params_of(native, rt=AREA, dst=(2, 2)), spec_of(native), boxes=((0, 0, 0, 80, 80),))[0] == OK
    assert rois_status(native, params_of(native, rt=AREA, dst=(2, 2)), spec_of(native), boxes=((0, 0, 0, 82, 80),))[0] == UNSUPPORTED
    # the facade: describe_rois and describe_rois_area both reach it with a spec
    fp = ts.FrameParameters(width=224, height=224, resize_type=AREA, pixel_format=BGR24, planes_pos=PLANAR, normalization=True)
    for fn in (ts.describe_rois, ts.describe_rois_area):
        d = fn(fp, (W, H), [(100, 50, 700, 550)], dtype=torch.float16)
        assert d["out"] == "f16_planar" and d["kernel"].startswith("vpp_rois_area_tensor<")
    with pytest.raises(RuntimeError, match="-2"):  # without a spec describe_rois keeps refusing AREA
        ts.describe_rois(fp, (W, H), [(100, 50, 700, 550)])
    d = ts.describe_letterbox(ts.FrameParameters(width=640, height=640, resize_type=BILINEAR, pixel_format=RGB24, planes_pos=PLANAR, normalization=True), (W, H),
                              dtype=torch.bfloat16, mean=T.IMAGENET[0], std=T.IMAGENET[1])
    assert d["out"] == "bf16_planar" and d["kernel"].startswith("vpp_letterbox_tensor<")


def test_the_facades_scale_is_one_over_std_in_float32(native):
    import tensor_stream as ts
    assert ts.tensor_spec() is None
    for std in (T.IMAGENET[1], T.CORNER[1], (0.5, 7.0, 1e-3), (255.0, 1.0 / 255.0, 3.0)):
        s = ts.tensor_spec(dtype=torch.float16, mean=T.IMAGENET[0], std=std)
        want = np.array([np.float32(1) / np.float32(v) for v in std], np.float32)
        assert np.array_equal(np.array(list(s.scale), np.float32).view(np.uint32), want.view(np.uint32)), std
        assert np.array_equal(np.array(list(s.mean), np.float32).view(np.uint32), np.array(T.IMAGENET[0], np.float32).view(np.uint32))
        assert s.dtype == native.TSVPP_F16
        assert np.array_equal(np.array(T.scales(std), np.float32).view(np.uint32), want.view(np.uint32))  # what the GPU tests expect with
    s = ts.tensor_spec(mean=0.5)  # one value for every channel; dtype defaults to float32, std to 1
    assert s.dtype == native.TSVPP_F32 and list(s.mean) == [0.5] * 3 and list(s.scale) == [1.0] * 3
    assert ts.tensor_spec(dtype=torch.bfloat16).dtype == native.TSVPP_BF16
    with pytest.raises(RuntimeError, match="-3"):
        ts.tensor_spec(dtype=torch.float64)
    with pytest.raises(ValueError):
        ts.tensor_spec(mean=(1.0, 2.0))


def test_tensor_util_with_the_identity_spec_returns_the_oracles_bits(oracle):
    y, uv = synth_nv12(128, 72, seed=5, pitch=192)
    for fcc, c in ((RGB24, 3), (BGR24, 3), (Y800, 1)):
        ref, _, _ = oracle.convert(y[:, :128], uv[:, :128], dst=(64, 64), resize_type=BILINEAR, fourcc=fcc, planes=PLANAR, normalization=True)
        assert ref.dtype == np.float32
        assert np.array_equal(T.expected(ref, c, T.IDENTITY, T.F32), ref.view(np.uint8).ravel())
        # ... and the half-precision forms are numpy's / torch's own round-to-nearest-even conversions of them
        assert np.array_equal(T.expected(ref, c, T.IDENTITY, T.F16), ref.astype(np.float16).view(np.uint8).ravel())
        assert np.array_equal(T.expected(ref, c, T.IDENTITY, T.BF16), T.bits(torch.from_numpy(ref).to(torch.bfloat16)))
    # the corner spec does what it is there for: exact zeros, negative values, fp16 subnormals
    q = (np.arange(256, dtype=np.float32) / np.float32(255))
    e = T.expected(np.stack([q, q, q]), 3, T.CORNER, T.F16).view(np.float16).reshape(3, 256)
    assert e[0, 0] == 0 and np.all(e[0, 1:] < 0) and e[1, 114] == 0 and e[2, 255] == 0
    assert np.any((np.abs(e[1]) > 0) & (np.abs(e[1]) < 2.0 ** -14))
    with np.errstate(over="ignore"):
        big = T.apply(q, 1, (0.0,), (np.float32(1e6),), T.F16).view(np.float16)
    bf = torch.from_numpy(T.apply(q, 1, (0.0,), (np.float32(1e6),), T.BF16).view(np.int16).copy()).view(torch.bfloat16).float()
    assert np.isinf(big[-1]) and bool(torch.isfinite(bf).all()) and float(bf[-1]) == 999424.0  # (1e6 to 8 bits)
