"""CPU: tsvpp_convert_remap's host side and its reference model (tests/remap_util.py) -- the model against the oracle (identity, exact ratios, even translation),
the ABI (symbols, struct sizes, every status from tsvpp_describe_remap without a context), the describe line, the footprint property (every tap of a tile lies
inside the box tsvpp_remap_footprint returns -- the function the kernel evaluates on its own extremes), the LDS hint, the proof that the GPU test's budgets run
both the staged and the gathering path, the Python helpers and the C++ facade's symbol."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import remap_util as R
from warp_util import BGR24, BILINEAR, MERGED, PLANAR, RGB24, Y800, F32
from util import knob_run, synth_nv12

OK, UNSUPPORTED, ERROR = 0, -2, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GEO = [(128, 72, 192), (72, 128, 96), (322, 182, 384), (32, 18, 48)]
DSTS = [(64, 64), (70, 66), (30, 34), (112, 112)]


@pytest.fixture(scope="module")
def native():
    from tensor_stream import _native
    _native.lib()
    return _native


# ---- 1. the model against the oracle ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("border", [None, (114, 128, 128)])
def test_model_identities(oracle, border):
    """the identity map is the frame itself; the exact 2 : 1 and 4 : 1 maps are the oracle's BILINEAR resize stage; an even translation is the crop -- as virtual
    frames, byte for byte, and through the oracle's conversion"""
    for k, (w, h, pitch) in enumerate([(128, 72, 192), (72, 128, 96), (32, 18, 48)]):
        y, uv = synth_nv12(w, h, seed=60 + k, pitch=pitch)
        Y, UV = R.virtual_frame_from_map(y, uv, w, h, R.identity(w, h), border)
        assert np.array_equal(Y, y[:h, :w]) and np.array_equal(UV, uv[:h // 2, :w]), (w, h)
        ref = oracle.convert(y, uv, fourcc=BGR24, planes=PLANAR, normalization=True, width=w)[0].ravel().view(np.uint8)
        assert np.array_equal(R.expected(oracle, y, uv, w, h, R.identity(w, h), BGR24, PLANAR, True, border), ref)
    w, h, pitch = 128, 72, 192
    y, uv = synth_nv12(w, h, seed=63, pitch=pitch)
    for r in (2, 4):
        dw, dh = w // r, h // r
        Y, UV = R.virtual_frame_from_map(y, uv, w, h, R.exact_ratio(dw, dh, r), border)
        ry, ruv = oracle.resize_stage(y, uv, dw, dh, BILINEAR, width=w)
        assert np.array_equal(Y, ry) and np.array_equal(UV, ruv), r
        ref = oracle.convert(y, uv, dst=(dw, dh), resize_type=BILINEAR, fourcc=RGB24, planes=MERGED, normalization=False, width=w)[0].ravel().view(np.uint8)
        assert np.array_equal(R.expected(oracle, y, uv, w, h, R.exact_ratio(dw, dh, r), RGB24, MERGED, False, border), ref), r
    dx, dy, dw, dh = 20, 6, 64, 48
    Y, UV = R.virtual_frame_from_map(y, uv, w, h, R.translation(dw, dh, dx, dy), border)
    assert np.array_equal(Y, y[dy:dy + dh, dx:dx + dw]) and np.array_equal(UV, uv[dy // 2:(dy + dh) // 2, dx:dx + dw])
    ref = oracle.convert(np.ascontiguousarray(y[dy:dy + dh, dx:dx + dw]), np.ascontiguousarray(uv[dy // 2:(dy + dh) // 2, dx:dx + dw]), fourcc=BGR24, planes=PLANAR,
                         normalization=True)[0].ravel().view(np.uint8)
    assert np.array_equal(R.expected(oracle, y, uv, w, h, R.translation(dw, dh, dx, dy), BGR24, PLANAR, True, border), ref)


def test_model_takes_every_bit_pattern():
    """NaN counts as -1 (fmax first), the NaN of +inf + -inf in a chroma sum included; infinities clamp to the ends; nothing but numbers leaves the clamp"""
    assert np.array_equal(R.clamp(np.array([np.nan, -np.inf, np.inf, -7, 3.5, 1e30], F32), 10), np.array([-1, -1, 10, -1, 3.5, 10], F32))
    x = np.array([[np.inf, -np.inf], [0, 0]], F32)
    assert np.isnan(R.chroma_coord(x)[0, 0]) and R.clamp(R.chroma_coord(x), 8)[0, 0] == -1
    assert R.chroma_coord(np.array([[10, 11], [10, 11]], F32))[0, 0] == F32(5.0)  # the block's mean position 10.5 on the pair grid: (10.5 + 0.5) / 2 - 0.5
    g = R.garbage(70, 66, 5)
    for c in R.coords(g, 322, 182):
        assert np.isfinite(c).all()
    y, uv = synth_nv12(322, 182, seed=9, pitch=384)
    Y, UV = R.virtual_frame_from_map(y, uv, 322, 182, g, (3, 250, 7))
    assert Y.shape == (66, 70) and UV.shape == (33, 70)


# ---- 2. ABI and statuses ---------------------------------------------------------------------------------------------------------------------------------

def _params(native, dst=(64, 64), rt=BILINEAR, fcc=RGB24, planes=MERGED, norm=0, crop=(0, 0, 0, 0)):
    return native.Params(crop[0], crop[1], crop[2], crop[3], dst[0], dst[1], rt, fcc, planes, norm)


def _describe(native, p, frames, maps, remaps, border=(-1, -1, -1), spec=None, n_frames=None, n_maps=None, n=None, aligned=1):
    L = native.lib()
    buf = ctypes.create_string_buffer(512)
    fr = (native.NV12 * max(len(frames), 1))(*frames) if frames is not None else None
    ms = (native.Map * max(len(maps), 1))(*maps) if maps is not None else None
    rs = (native.Remap * max(len(remaps), 1))(*remaps) if remaps is not None else None
    nf = len(frames) if n_frames is None else n_frames
    nm = len(maps) if n_maps is None else n_maps
    nr = len(remaps) if n is None else n
    pp = ctypes.byref(p) if p is not None else None
    if spec is None:
        sts = L.tsvpp_describe_remap(pp, nf, fr, nm, ms, nr, rs, border[0], border[1], border[2], aligned, buf, len(buf))
    else:
        sp = ctypes.byref(spec) if spec != "null" else None
        sts = L.tsvpp_describe_remap_tensor(pp, sp, nf, fr, nm, ms, nr, rs, border[0], border[1], border[2], aligned, buf, len(buf))
    return sts, buf.value.decode()


def test_symbols_and_struct_sizes(native):
    assert ctypes.sizeof(native.Map) == 16 and ctypes.sizeof(native.Remap) == 8
    assert native.TSVPP_MAX_REMAPS == 32
    header = open(os.path.join(ROOT, "include", "tsvpp.h")).read()
    assert "#define TSVPP_MAX_REMAPS 32" in header
    L = native.lib()
    for s in ("tsvpp_convert_remap", "tsvpp_describe_remap", "tsvpp_convert_remap_tensor", "tsvpp_describe_remap_tensor", "tsvpp_remap_footprint", "tsvpp_remap_lds_need"):
        assert s in native.SYMBOLS
        getattr(L, s)


def test_statuses_in_their_order_without_a_context(native):
    N = native
    fr = [N.NV12(None, None, 192, 192, 128, 72)]
    ms = [N.Map(None, 0, 0)]
    rs = [N.Remap(0, 0)]
    p = _params(N)
    assert _describe(N, p, fr, ms, rs)[0] == OK
    # TSVPP_ERROR
    assert _describe(N, None, fr, ms, rs)[0] == ERROR
    assert _describe(N, p, None, ms, rs, n_frames=1)[0] == ERROR
    assert _describe(N, p, fr, None, rs, n_maps=1)[0] == ERROR
    assert _describe(N, p, fr, ms, None, n=1)[0] == ERROR
    assert N.lib().tsvpp_describe_remap(ctypes.byref(p), 1, (N.NV12 * 1)(*fr), 1, (N.Map * 1)(*ms), 1, (N.Remap * 1)(*rs), -1, -1, -1, 1, None, 0) == ERROR
    assert _describe(N, p, fr, ms, rs, n_frames=0)[0] == ERROR
    assert _describe(N, p, fr, ms, rs, n_maps=0)[0] == ERROR
    assert _describe(N, p, fr, ms, rs, n=0)[0] == ERROR
    assert _describe(N, p, [N.NV12(None, None, 192, 192, 0, 72)], ms, rs)[0] == ERROR
    assert _describe(N, p, [N.NV12(None, None, 100, 192, 128, 72)], ms, rs)[0] == ERROR
    assert _describe(N, p, [N.NV12(None, None, 192, 100, 128, 72)], ms, rs)[0] == ERROR
    for bad in (N.Remap(1, 0), N.Remap(-1, 0), N.Remap(0, 1), N.Remap(0, -1)):
        assert _describe(N, p, fr, ms, [bad])[0] == ERROR
    assert _describe(N, _params(N, dst=(0, 64)), fr, ms, rs)[0] == ERROR
    assert _describe(N, _params(N, dst=(64, -2)), fr, ms, rs)[0] == ERROR
    assert _describe(N, _params(N, crop=(0, 0, 32, 32)), fr, ms, rs)[0] == ERROR
    for border in ((256, 128, 128), (-2, -2, -2), (-1, 128, 128), (114, -1, 128), (114, 128, -1), (0, 0, 300)):
        assert _describe(N, p, fr, ms, rs, border=border)[0] == ERROR, border
    assert _describe(N, p, fr, [N.Map(None, 8 * 64, 0)], rs)[0] == OK
    assert _describe(N, p, fr, [N.Map(None, 8 * 64 + 48, 4096)], rs)[0] == OK
    assert _describe(N, p, fr, [N.Map(None, 8 * 64 - 8, 0)], rs)[0] == ERROR   # below 8 * dst_width
    assert _describe(N, p, fr, [N.Map(None, 8 * 64 + 4, 0)], rs)[0] == ERROR   # no multiple of 8
    assert _describe(N, p, fr, [N.Map(None, -512, 0)], rs)[0] == ERROR
    assert _describe(N, p, fr, [N.Map(None, 0, -1)], rs)[0] == ERROR           # a negative hint
    assert _describe(N, p, fr, [N.Map(None, 0, 0), N.Map(None, 0, -1)], rs)[0] == ERROR  # ... on a map no output uses, too
    # TSVPP_UNSUPPORTED
    assert _describe(N, _params(N, dst=(63, 64)), fr, ms, rs)[0] == UNSUPPORTED
    assert _describe(N, _params(N, dst=(64, 33)), fr, ms, rs)[0] == UNSUPPORTED
    assert _describe(N, p, [N.NV12(None, None, 192, 192, 127, 72)], ms, rs)[0] == UNSUPPORTED
    assert _describe(N, p, [N.NV12(None, None, 192, 192, 128, 71)], ms, rs)[0] == UNSUPPORTED
    for rt in (0, 2, 3, 7):  # NEAREST, BICUBIC, AREA, unknown
        assert _describe(N, _params(N, rt=rt), fr, ms, rs)[0] == UNSUPPORTED, rt
    for fcc in (3, 4, 5, 6):  # NV12, UYVY, YUV444, HSV in the header's numbering, whichever they are: none is in the list
        if fcc not in (Y800, RGB24, BGR24):
            assert _describe(N, _params(N, fcc=fcc), fr, ms, rs)[0] == UNSUPPORTED, fcc
    assert _describe(N, _params(N, dst=(32768, 32768), norm=1), fr, ms, rs)[0] == UNSUPPORTED  # 12 GiB
    # an ERROR condition wins over an UNSUPPORTED one
    assert _describe(N, _params(N, dst=(63, 64), rt=3), fr, ms, rs, border=(256, 0, 0))[0] == ERROR
    assert _describe(N, _params(N, rt=2), fr, [N.Map(None, 12, 0)], rs)[0] == ERROR
    assert _describe(N, _params(N, dst=(63, 64)), fr, ms, [N.Remap(0, 5)])[0] == ERROR


def test_tensor_describe_adds_the_spec_rules_behind_the_request(native):
    N = native
    fr = [N.NV12(None, None, 192, 192, 128, 72)]
    ms, rs = [N.Map(None, 0, 0)], [N.Remap(0, 0)]
    spec = N.TensorSpec(N.TSVPP_F16, (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1))
    ok = _params(N, fcc=BGR24, planes=PLANAR, norm=1)
    sts, line = _describe(N, ok, fr, ms, rs, spec=spec, border=(114, 128, 128))
    assert sts == OK
    if not knob_run():
        assert "kernel=vpp_remap_tensor<PLANAR,EL_HALF,vec,staged,border>" in line and "out=f16_planar" in line and line.endswith("border=114,128,128")
    # rule 1 first: the request's own status
    assert _describe(N, _params(N, fcc=BGR24, planes=PLANAR, norm=1, rt=2), fr, ms, rs, spec="null")[0] == UNSUPPORTED
    assert _describe(N, ok, fr, ms, [N.Remap(0, 3)], spec=N.TensorSpec(9, (ctypes.c_float * 3)(), (ctypes.c_float * 3)(1, 1, 1)))[0] == ERROR
    # rule 2
    assert _describe(N, ok, fr, ms, rs, spec="null")[0] == ERROR
    assert _describe(N, ok, fr, ms, rs, spec=N.TensorSpec(N.TSVPP_F16, (ctypes.c_float * 3)(0, float("nan"), 0), (ctypes.c_float * 3)(1, 1, 1)))[0] == ERROR
    assert _describe(N, ok, fr, ms, rs, spec=N.TensorSpec(N.TSVPP_F16, (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 0, 1)))[0] == ERROR
    # rule 3
    assert _describe(N, ok, fr, ms, rs, spec=N.TensorSpec(9, (ctypes.c_float * 3)(), (ctypes.c_float * 3)(1, 1, 1)))[0] == UNSUPPORTED
    assert _describe(N, _params(N, fcc=BGR24, planes=PLANAR, norm=0), fr, ms, rs, spec=spec)[0] == UNSUPPORTED
    assert _describe(N, _params(N, fcc=BGR24, planes=MERGED, norm=1), fr, ms, rs, spec=spec)[0] == UNSUPPORTED
    assert _describe(N, _params(N, fcc=Y800, planes=MERGED, norm=1), fr, ms, rs, spec=spec)[0] == OK


# ---- 3. describe -----------------------------------------------------------------------------------------------------------------------------------------

REDUCE_LDS = 64  # the staged kernels' static LDS: eight extremes per wave


def test_describe_line(native, monkeypatch):
    import tensor_stream as ts
    if knob_run():  # (replayed under A/B knobs: the selections are the knobs')
        return
    fp = ts.FrameParameters(width=112, height=112, resize_type=ts.ResizeType.BILINEAR, pixel_format=ts.FourCC.BGR24, planes_pos=ts.Planes.PLANAR, normalization=True)
    budget = 40 * 1024 - REDUCE_LDS
    for n, launches in ((32, 1), (33, 2)):
        d = ts.describe_remap(fp, (1920, 1080, 2048), (0, 0), remaps=[(0, 0)] * n)
        assert d["mode"] == "remap_bilinear" and d["out"] == "f32_planar" and d["dst"] == "112x112" and d["remaps"] == n and d["maps"] == 1 and d["frames"] == 1
        assert d["launches"] == launches and d["limit"] == 32 and d["tiles"] == "4x4" and d["shape"] == "8x16" and "staged" not in d
        assert d["grid"] == 16 * min(n, 32) and d["kernel"] == "vpp_remap<O_F32_PLANAR,vec,staged,replicate>" and d["border"] == "replicate"
        assert d["lds"] == budget  # no hint: the budget
    d = ts.describe_remap(fp, (1920, 1080, 2048), (0, 0), border=(114, 128, 128), aligned_outputs=False)
    assert d["kernel"] == "vpp_remap<O_F32_PLANAR,elem,staged,border>" and d["border"] == "114,128,128"
    # a hint; the largest of mixed hints; a map without one counts as the budget; a hint above the budget is capped; a hint on a map the FIRST launch does not use
    assert ts.describe_remap(fp, (1920, 1080, 2048), (0, 3000))["lds"] == 3000
    two = [(1920, 1080, 2048)] * 2
    assert ts.describe_remap(fp, two, [(0, 3000), (8 * 112 + 16, 5000)])["lds"] == 5000
    assert ts.describe_remap(fp, two, [(0, 3000), (0, 0)])["lds"] == budget
    assert ts.describe_remap(fp, two, [(0, 3000), (0, 1 << 20)])["lds"] == budget
    d = ts.describe_remap(fp, two, [(0, 3000), (0, 0)], remaps=[(0, 0)] * 32 + [(1, 1)])
    assert d["lds"] == 3000 and d["launches"] == 2 and d["maps"] == 2 and d["remaps"] == 33
    # the merged vector-store kernels' exchange slabs count against the budget, as everywhere
    mg = ts.FrameParameters(width=112, height=112, resize_type=ts.ResizeType.BILINEAR, pixel_format=ts.FourCC.RGB24, planes_pos=ts.Planes.MERGED, normalization=True)
    d = ts.describe_remap(mg, (1920, 1080, 2048), (0, 0))
    assert d["kernel"] == "vpp_remap<O_F32_MERGED,vec,staged,replicate>" and d["lds"] == budget - 256 * 48
    assert ts.describe_remap(mg, (1920, 1080, 2048), (0, 0), aligned_outputs=False)["lds"] == budget
    # 4 k + 2 columns: the shifted tile column; narrower than a tile: element-wise
    for dst, kind, tail in (((70, 66), "vec", 2), ((30, 34), "elem", 0)):
        q = ts.FrameParameters(width=dst[0], height=dst[1], resize_type=ts.ResizeType.BILINEAR, pixel_format=ts.FourCC.RGB24, planes_pos=ts.Planes.PLANAR, normalization=False)
        d = ts.describe_remap(q, (322, 182, 384), (0, 0))
        assert d["kernel"] == f"vpp_remap<O_U8_PLANAR,{kind},staged,replicate>" and d["tail"] == tail
    # no budget: the gather kernel, whatever the hint
    monkeypatch.setenv("TSVPP_LDS_KB", "0")
    d = ts.describe_remap(fp, (1920, 1080, 2048), (0, 3000))
    assert d["lds"] == 0 and d["kernel"] == "vpp_remap<O_F32_PLANAR,vec,gather,replicate>"
    monkeypatch.setenv("TSVPP_LDS_KB", "3")
    assert ts.describe_remap(fp, (1920, 1080, 2048), (0, 0))["lds"] == 3 * 1024 - REDUCE_LDS
    assert ts.describe_remap(fp, (1920, 1080, 2048), (0, 2000))["lds"] == 2000


def test_python_argument_forms_raise_before_the_c_call():
    import torch
    import tensor_stream as ts
    fp = ts.FrameParameters(width=64, height=64, resize_type=ts.ResizeType.BILINEAR, pixel_format=ts.FourCC.BGR24, planes_pos=ts.Planes.PLANAR, normalization=True)
    good = torch.zeros(64, 64, 2)
    assert ts.describe_remap(fp, (128, 72), good)["remaps"] == 1
    assert ts.describe_remap(fp, [(128, 72)] * 3, good)["remaps"] == 3                      # one map: every frame through it
    assert ts.describe_remap(fp, [(128, 72)] * 2, [good, (good, 4096)])["remaps"] == 2      # as many maps as frames: they pair up
    wide = torch.zeros(64, 70, 2)[:, :64]                                                     # a row stride of 140 floats
    if not knob_run():
        assert ts.describe_remap(fp, (128, 72), (wide, 2048))["lds"] == 2048
    for bad in (torch.zeros(64, 64, 2, dtype=torch.float64), torch.zeros(64, 64, 3), torch.zeros(64, 62, 2), torch.zeros(64, 64), torch.zeros(2, 64, 64).permute(1, 2, 0),
                torch.zeros(64, 128, 2)[:, ::2]):
        with pytest.raises(ValueError):
            ts.describe_remap(fp, (128, 72), bad)
    with pytest.raises(ValueError):
        ts.describe_remap(fp, [(128, 72)] * 3, [good, good])
    with pytest.raises(ValueError):
        ts.describe_remap(fp, (128, 72), good, remaps=[(0, 0, 0)])
    with pytest.raises(ValueError):
        ts.describe_remap(fp, (128, 72), [])
    with pytest.raises(RuntimeError, match="-3"):
        ts.describe_remap(fp, (128, 72), good, remaps=[(0, 1)])


# ---- 4. the footprint, the hint, and which path the GPU test's tiles take ------------------------------------------------------------------------------------

def _footprint(native, xy, w, h, j0, j1, i0, i1, pitch=0, back=None):
    out = (ctypes.c_int32 * 8)()
    host = np.ascontiguousarray(xy) if back is None else back
    dst_h, dst_w = xy.shape[:2]
    sts = native.lib().tsvpp_remap_footprint(host.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), pitch, dst_w, dst_h, w, h, j0, j1, i0, i1, out)
    assert sts == OK, sts
    return tuple(out)


def test_every_tap_of_a_tile_lies_inside_the_footprint(native):
    """every map of the set on every geometry and output size, every tile of both tilings: first and second tap of every pixel and of every chroma pair lie inside
    the box (the second tap where its weight was not forced to zero at the low edge), the box lies inside the frame, and pitch padding changes nothing"""
    for (w, h, _) in GEO:
        for (dw, dh) in DSTS:
            for name, xy in R.map_set(w, h, dw, dh).items():
                for (j0, j1, i0, i1) in sorted(set(R.tiles(dw, dh, False)) | set(R.tiles(dw, dh, True))):
                    f = _footprint(native, xy, w, h, j0, j1, i0, i1)
                    assert 0 <= f[0] <= f[1] < w and 0 <= f[2] <= f[3] < h and 0 <= f[4] <= f[5] < w // 2 and 0 <= f[6] <= f[7] < h // 2, (name, f)
                    t = R.tap_boxes(xy, w, h, j0, j1, i0, i1)
                    for k in range(0, 8, 2):
                        assert f[k] <= t[k] and t[k + 1] <= f[k + 1], (name, (w, h), (dw, dh), (j0, j1, i0, i1), f, t)
            view, back = R.padded(R.map_set(w, h, dw, dh)["barrel"])
            assert _footprint(native, view, w, h, 0, min(dw, 32) - 1, 0, min(dh, 32) - 1, pitch=back.strides[0], back=back) == \
                _footprint(native, R.map_set(w, h, dw, dh)["barrel"], w, h, 0, min(dw, 32) - 1, 0, min(dh, 32) - 1)


def test_footprint_is_tight_and_refuses_what_it_cannot_read(native):
    xy = R.translation(64, 64, 20, 6)
    assert _footprint(native, xy, 128, 72, 0, 31, 0, 31) == (20, 52, 6, 38, 10, 26, 3, 19)  # floor(min) .. floor(max) + 1 on both grids
    assert _footprint(native, R.split(64, 64, 128, 72), 128, 72, 16, 47, 0, 31) == (0, 127, 0, 71, 0, 63, 0, 35)
    assert _footprint(native, R.far(64, 64), 128, 72, 0, 31, 0, 31) == (127, 127, 0, 0, 63, 63, 0, 0)
    L = native.lib()
    out = (ctypes.c_int32 * 8)()
    p = np.ascontiguousarray(xy).ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert L.tsvpp_remap_footprint(None, 0, 64, 64, 128, 72, 0, 31, 0, 31, out) == ERROR
    assert L.tsvpp_remap_footprint(p, 0, 64, 64, 128, 72, 0, 31, 0, 31, None) == ERROR
    assert L.tsvpp_remap_footprint(p, 0, 64, 64, 128, 72, 0, 64, 0, 31, out) == ERROR    # leaves the map
    assert L.tsvpp_remap_footprint(p, 0, 64, 64, 128, 72, 0, 31, 32, 65, out) == ERROR
    assert L.tsvpp_remap_footprint(p, 0, 64, 64, 128, 72, 1, 31, 0, 31, out) == ERROR    # half a pair
    assert L.tsvpp_remap_footprint(p, 0, 64, 64, 128, 72, 8, 7, 0, 31, out) == ERROR     # empty
    assert L.tsvpp_remap_footprint(p, 500, 64, 64, 128, 72, 0, 31, 0, 31, out) == ERROR  # pitch below 8 * dst_w
    assert L.tsvpp_remap_footprint(p, 0, 64, 64, 0, 72, 0, 31, 0, 31, out) == ERROR
    assert L.tsvpp_remap_lds_need(None, 0, 64, 64, 128, 72, 0) == ERROR
    assert L.tsvpp_remap_lds_need(p, 0, 64, 63, 128, 72, 0) == ERROR


def test_lds_need_is_the_largest_tile(native):
    import tensor_stream as ts
    for (w, h, _) in GEO[:3]:
        for (dw, dh) in DSTS:
            for name, xy in R.map_set(w, h, dw, dh).items():
                boxes = [_footprint(native, xy, w, h, *t) for t in sorted(set(R.tiles(dw, dh, False)) | set(R.tiles(dw, dh, True)))]
                for luma_only in (False, True):
                    assert ts.remap_lds_hint(xy, w, h, luma_only=luma_only) == max(R.lds_need(b, luma_only) for b in boxes), (name, (w, h), (dw, dh), luma_only)
    # a smooth undistortion of a 1080p frame: a few KiB per tile, not 40
    need = ts.remap_lds_hint(R.barrel(640, 360, 1920, 1080), 1920, 1080)
    assert 0 < need < 40 * 1024 - REDUCE_LDS


def test_the_gpu_tests_budgets_run_both_paths(native):
    """the maps tests/test_gpu_remap.py sends through contexts of TSVPP_LDS_KB = default / 0 / 3: from the footprints, every tile stages under the default budget,
    none under 0, and under 3 KiB some do and some do not -- so that test runs the staged path, the gathering path and a launch that mixes them"""
    (w, h, _), dst, names = R.STAGING_CASE
    maps = R.map_set(w, h, *dst)
    needs = [R.lds_need(b) for name in names for b in (_footprint(native, maps[name], w, h, *t) for t in R.tiles(dst[0], dst[1], True))
             if R.stageable(b)]
    assert len(needs) == len(names) * 16  # (every box is stageable)
    for kb, want in ((40, "all"), (0, "none"), (3, "mix")):
        budget = max(kb * 1024 - REDUCE_LDS, 0)
        fit = sum(1 for n in needs if n <= budget)
        assert {"all": fit == len(needs), "none": fit == 0, "mix": 0 < fit < len(needs)}[want], (kb, fit, len(needs))
    # ... and the set's folding maps gather under the default budget: the map-set test mixes both paths as well
    for name in ("split", "garbage"):
        assert max(R.lds_need(_footprint(native, maps[name], w, h, *t)) for t in R.tiles(dst[0], dst[1], True)) > 40 * 1024


# ---- 5. the helpers and the C++ facade -----------------------------------------------------------------------------------------------------------------------

def test_remap_helpers():
    import torch
    import torch.nn.functional as F
    import tensor_stream as ts
    rng = np.random.default_rng(3)
    g = rng.uniform(-1.3, 1.3, (66, 70, 2)).astype(F32)
    w, h = 322, 182
    want = np.stack((((g[..., 0] + F32(1)) * F32(w) - F32(1)) * F32(0.5), ((g[..., 1] + F32(1)) * F32(h) - F32(1)) * F32(0.5)), axis=-1)
    got = ts.remap_from_grid(g, w, h)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    got_t = ts.remap_from_grid(torch.from_numpy(g), w, h)
    assert isinstance(got_t, torch.Tensor) and got_t.is_contiguous() and np.array_equal(got_t.numpy().view(np.uint32), want.view(np.uint32))
    ident = F.affine_grid(torch.tensor([[[1.0, 0, 0], [0, 1.0, 0]]]), (1, 1, h, w), align_corners=False)[0]
    m = ts.remap_from_grid(ident, w, h).numpy()
    j, i = R.grid(w, h)
    assert np.abs(m[..., 0] - j).max() < 1e-3 and np.abs(m[..., 1] - i).max() < 1e-3
    mx, my = rng.uniform(0, 300, (66, 70)), rng.uniform(0, 180, (66, 70))
    s = ts.remap_from_opencv(mx, my)
    assert s.shape == (66, 70, 2) and s.dtype == np.float32 and s.flags["C_CONTIGUOUS"]
    assert np.array_equal(s[..., 0], mx.astype(F32)) and np.array_equal(s[..., 1], my.astype(F32))
    st = ts.remap_from_opencv(torch.from_numpy(mx), torch.from_numpy(my))
    assert st.dtype == torch.float32 and st.is_contiguous() and np.array_equal(st.numpy(), s)
    with pytest.raises(ValueError):
        ts.remap_from_opencv(mx, my[:, :5])
    with pytest.raises(ValueError):
        ts.remap_from_grid(g[..., 0], w, h)
    with pytest.raises(ValueError):
        ts.remap_lds_hint(g.astype(np.float64), w, h)


def test_the_cpp_facade_exports_convert_remap():
    lib = os.path.join(ROOT, "tensor-stream_amd", "lib", "libtsvpp_host.so")
    assert os.path.exists(lib), "build() makes it"
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    mangled = [s for s in syms.split() if "VideoProcessor" in s and "ConvertRemap" in s]
    assert len(mangled) == 2, mangled  # without and with a tensor spec
