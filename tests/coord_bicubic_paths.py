"""The BICUBIC warp calls (tsvpp_convert_warp_bicubic, tsvpp_convert_perspective_bicubic) as tests/coord_suite.py's descriptors, WARP_BICUBIC and
PERSP_BICUBIC, and the bodies of the GPU cases the two calls have beyond the suite's: tests/test_gpu_warp_bicubic.py and tests/test_gpu_persp_bicubic.py call
them from tests of a line or two.

The descriptors are tests/coord_paths.py's rows of coefficients -- the same item sets, staging expectations and shared-case items as the BILINEAR calls -- with
the model of tests/warp_bicubic_util.py, and a call / describe that ask for BICUBIC whatever resize type the suite's parameters name (the suite builds its
parameters for the BILINEAR calls).  The suite's refusal case pins BICUBIC as refused and does not apply: the new calls' refusals are live_refusals() below."""
import ctypes
import dataclasses
import math

import numpy as np
import pytest
import torch

import coord_paths as cp
import coord_suite as cs
import edge_content as E
import persp_util as P
import sampler64 as S
import sampler64_cubic as C
import tensor_util as T
import warp_bicubic_util as B
import warp_util as W
from letterbox_util import BGR24, BICUBIC, FLAVOURS, MERGED, PLANAR, RGB24, Y800, bits
from util import synth_nv12

GEO = C.FRAMES    # 322 x 182 (pitch 384), 32 x 18 (pitch 48), 4 x 2: every upper tap collapses, the chroma plane is 2 x 1 pairs
DSTS = C.DSTS     # 70 x 66 (shifted last tile column), 30 x 34 (narrower than a tile), 112 x 112
BORDERS = [None, (3, 250, 7)]
# the tensor forms of the bits case: (dtype, spec, fourcc, planes)
TENSORS = [(T.F16, "imagenet", BGR24, PLANAR), (T.BF16, "corner", RGB24, PLANAR), (T.F32, "imagenet", Y800, MERGED)]


def bicubic(fp):
    """the parameters `fp` (FrameParameters or tsvpp_params) with resize_type BICUBIC, as a tsvpp_params"""
    from tensor_stream import _native as N
    p = fp.parameters if hasattr(fp, "parameters") else fp
    q = N.Params.from_buffer_copy(p)
    q.resize_type = BICUBIC
    return q


def _descriptor(name, item_set, record, valid, staging, split, guard, gterm, capture, picks):
    import tensor_stream as ts
    rows = cp._rows(name, B, item_set, record, valid, staging, None, split=split, guard=guard, gterm=gterm, capture=capture)
    d = dataclasses.replace(
        rows,
        call=lambda v, ys, uvs, items, fp, **kw: getattr(v, "convert_" + name)(ys, uvs, [(k,) + c for k, c in items], bicubic(fp), **kw),
        describe=lambda fp, geo, items, **kw: getattr(ts, "describe_" + name)(bicubic(fp), list(geo), [(k,) + c for k, c in items], **kw))
    return d, picks


# the items of the bits case, per frame: a rotation inside, an up-scale with shear (weights on every phase), one that leaves the frame, one far outside
WARP_BICUBIC, WARP_PICKS = _descriptor("warp_bicubic", cp.matrices, lambda N: N.Warp, lambda w, h: W.scale_only(w, h, 64, 64), cp._warp_staging,
                                       ["rot30", "up_shear", "left", "bottom"], ("rot30", "right"), ("rot30", "top"), ("rot30", "left"),
                                       ("rot30", "up_shear", "left", "far"))
PERSP_BICUBIC, PERSP_PICKS = _descriptor("perspective_bicubic", cp.homographies, lambda N: N.Persp, lambda w, h: P.affine(W.scale_only(w, h, 64, 64)),
                                         cp._persp_staging, ["mild", "strong", "left", "keyrot"], ("keyrot", "right"), ("strong", "top"), ("strong", "left"),
                                         ("mild", "strong", "left", "x3"))


def frames_fixture(seed):
    """the module-scoped fixture `frames3`: the frames of GEO above, [(y, uv)] on the host and the same on the device"""
    @pytest.fixture(scope="module")
    def frames3():
        return cs.device_frames(GEO, seed)
    return frames3


def _call(path, v, dev, items, fp, border, **kw):
    got = path.call(v, [d[0] for d in dev], [d[1] for d in dev], items, fp, border=border, width=[g[0] for g in GEO], height=[g[1] for g in GEO], **kw)
    torch.cuda.synchronize()
    return got


def bits_and_bracket(path, picks, vpp, oracle, frames3, dst):
    """one call per flavour for `picks` on each of the three frames: raw bits against the model in all colour flavours and the tensor forms, replicate and a
    border; and the fp32, uint8 and fp16 results inside the output bracket of the float64 judge (tests/sampler64_cubic.py), every element"""
    import tensor_stream as ts
    host, dev = frames3
    items = path.pick([(k, nm) for k in range(len(GEO)) for nm in picks], GEO, dst)
    for border in BORDERS:
        got = {}
        for fcc, planes, norm in FLAVOURS:
            got[fcc, planes, norm] = cs.check(path, vpp, oracle, host, dev, GEO, items, dst, fcc, planes, norm, border, what="bits")
        tensors = {}
        for dtype, spec, fcc, planes in TENSORS:
            t = _call(path, vpp, dev, items, cs.params(ts, dst, fcc, planes, True), border, dtype=T.TORCH[dtype], mean=T.SPECS[spec][0], std=T.SPECS[spec][1])
            assert t.dtype == T.TORCH[dtype]
            tensors[dtype] = t
            for i in range(len(items)):
                k, arg, tag, words = path.output(items, i, dst)
                q = path.expected(oracle, arg, dst, fcc, planes, True, border, cs.virtual(path, host, k, GEO, arg, tag, dst, border)).view(np.float32)
                assert np.array_equal(T.bits(t[i]), T.expected(q, 1 if fcc == Y800 else 3, T.SPECS[spec], dtype)), (i, words, dst, dtype, spec, border)
        for i, (k, c) in enumerate(items):
            w, h, _ = GEO[k]
            vb = C.virtual_bracket(host[k][0], host[k][1], w, h, C.positions(c, *dst), border)
            for (fcc, planes, norm), dt in (((BGR24, PLANAR, True), np.float32), ((RGB24, MERGED, False), np.uint8)):
                lo, hi = S.output_bracket(oracle, vb, fcc, planes, norm)
                g = got[fcc, planes, norm][i].cpu().numpy().ravel().view(dt)
                assert S.outside(g, lo, hi).size == 0, (i, k, c, dst, border, fcc)
            lo, hi = S.tensor_bracket(oracle, vb, BGR24, T.SPECS["imagenet"], T.F16)
            assert S.outside(S.tensor_values(T.bits(tensors[T.F16][i]), T.F16), lo, hi).size == 0, (i, k, c, dst, border, "f16")


def scale_only_is_convert_bicubic(path, scale_item, vpp, oracle, frames3, dst):
    """the scale-only item: the call is Convert(BICUBIC, dst) of the whole frame and the oracle's, bit for bit, under both border modes"""
    import tensor_stream as ts
    host, dev = frames3
    items = [(k, scale_item(w, h, *dst)) for k, (w, h, _) in enumerate(GEO)]
    for fcc, planes, norm in ((BGR24, PLANAR, True), (RGB24, MERGED, False), (Y800, MERGED, False)):
        fp = ts.FrameParameters(width=dst[0], height=dst[1], resize_type=BICUBIC, pixel_format=fcc, planes_pos=planes, normalization=norm)
        refs = [oracle.convert(host[k][0], host[k][1], dst=dst, resize_type=BICUBIC, fourcc=fcc, planes=planes, normalization=norm, width=w)[0].ravel().view(np.uint8)
                for k, (w, h, _) in enumerate(GEO)]
        ones = [vpp.Convert(dev[k][0], dev[k][1], fp, width=w, height=h) for k, (w, h, _) in enumerate(GEO)]
        for border in (None, (114, 128, 128)):
            got = _call(path, vpp, dev, items, fp, border)
            for k in range(len(GEO)):
                assert np.array_equal(bits(got[k]), refs[k]) and np.array_equal(bits(got[k]), bits(ones[k])), (k, dst, fcc, planes, norm, border)


def edge_content_classes(path, items_of, vpp, oracle):
    """the eight classes of tests/edge_content.py -- content that sits on the rounding boundaries, pitch padding that shows a read past the picture -- through
    items_of(w, h, dw, dh), a rotated and a keystone item: the model's bits, replicate and a border"""
    w, h, pitch = GEO[0]
    dst = (70, 66)
    items = [(0, c) for c in items_of(w, h, *dst)]
    for name in E.CLASSES:
        y, uv = E.frame(name, w, h, pitch, pitch)
        dev = [(torch.from_numpy(np.ascontiguousarray(y)).cuda(), torch.from_numpy(np.ascontiguousarray(uv)).cuda())]
        for border, (fcc, planes, norm) in ((None, (BGR24, PLANAR, True)), ((3, 250, 7), (RGB24, MERGED, False))):
            cs.check(path, vpp, oracle, [(y, uv)], dev, [GEO[0]], items, dst, fcc, planes, norm, border, what=name, key=lambda k: ("edge", name))


def fuzz_chunk(path, draw_item, vpp, oracle, seed, n_calls=10):
    """a seeded chunk of calls: frame size, pitch, output size, flavour, border, 1 .. 4 items of draw_item(rng, w, h, dw, dh) per call -- the model's bits"""
    rng = np.random.default_rng(seed)
    for call in range(n_calls):
        w, h = 2 * int(rng.integers(2, 120)), 2 * int(rng.integers(1, 70))
        pitch = w + int(rng.choice([0, 2, 16, 62]))
        dst = (2 * int(rng.integers(1, 50)), 2 * int(rng.integers(1, 40)))
        y, uv = synth_nv12(w, h, seed=seed + 100 + call, pitch=pitch)
        dev = [(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda())]
        items = [(0, draw_item(rng, w, h, *dst)) for _ in range(int(rng.integers(1, 5)))]
        fcc, planes, norm = FLAVOURS[int(rng.integers(len(FLAVOURS)))]
        border = None if rng.random() < 0.5 else tuple(int(v) for v in rng.integers(0, 256, 3))
        geo = [(w, h, pitch)]
        cs.check(path, vpp, oracle, [(y, uv)], dev, geo, items, dst, fcc, planes, norm, border, what=f"seed {seed} call {call}", key=lambda k: ("fuzz", seed, call))


def draw_matrix(rng, w, h, dw, dh):
    """scales 0.3 .. 5, any angle, shear, centred / partly outside / wholly outside"""
    sx, sy = rng.uniform(0.3, 5.0, 2)
    ang, shear = rng.uniform(0, 2 * math.pi), rng.uniform(-0.5, 0.5)
    c, s = math.cos(ang), math.sin(ang)
    a, b, d, e = sx * c, -sy * s + shear * sx * c, sx * s, sy * c + shear * sx * s
    kind = int(rng.integers(4))
    cx = w / 2 + (0, rng.uniform(-w, w), rng.choice([-1, 1]) * (w + 40), rng.choice([-1, 1]) * 5000)[kind]
    cy = h / 2 + (0, rng.uniform(-h, h), rng.choice([-1, 1]) * (h + 40), rng.choice([-1, 1]) * 7000)[kind]
    return cp.f32((a, b, cx - a * dw / 2 - b * dh / 2, d, e, cy - d * dw / 2 - e * dh / 2))


def draw_homography(rng, w, h, dw, dh):
    """the quad of a jittered rectangle, shifted as draw_matrix's kinds; a draw whose horizon crosses the output falls back to its affine part"""
    x0, y0, x1, y1 = rng.uniform(-0.2, 0.4) * w, rng.uniform(-0.2, 0.4) * h, rng.uniform(0.6, 1.2) * w, rng.uniform(0.6, 1.2) * h
    jit = lambda: (rng.uniform(-0.15, 0.15) * w, rng.uniform(-0.15, 0.15) * h)
    quad = [(x + jit()[0], y + jit()[1]) for x, y in ((x0, y0), (x1, y0), (x1, y1), (x0, y1))]
    q = P.from_quad(quad, dw, dh)
    if q is None or not P.in_domain(q, dw, dh):
        q = P.affine(draw_matrix(rng, w, h, dw, dh))
    return cp.f32(q)


def live_refusals(path, kind, vpp, frames):
    """with a live context the request's status answers before any launch: every resize type but BICUBIC is -2, the BILINEAR call refuses BICUBIC (-2), a broken
    item, border or frame index is -3; at the C entry point a null plane, output, output list or context is -3 -- with a spec and without -- and the valid
    request launches.  frames: coord_suite's (GEO[0] is used)"""
    import tensor_stream as ts
    from tensor_stream import _native as N
    host, dev = frames
    (y, uv), (w, h, pitch) = dev[0], cs.GEO[0]
    c = path.valid(w, h)[0][1]
    convert = getattr(vpp, "convert_" + path.name)

    def call(items=[(0,) + c], rt=BICUBIC, fcc=RGB24, planes=MERGED, norm=False, **kw):
        fp = ts.FrameParameters(width=64, height=64, resize_type=rt, pixel_format=fcc, planes_pos=planes, normalization=norm)
        return convert(y, uv, items, fp, width=w, height=h, **kw)
    for rt in (0, 1, 3):  # NEAREST, BILINEAR, AREA
        with pytest.raises(RuntimeError, match="-2"):
            call(rt=rt)
    with pytest.raises(RuntimeError, match="-2"):  # the BILINEAR call keeps refusing BICUBIC
        getattr(vpp, "convert_" + kind)(y, uv, [(0,) + c], ts.FrameParameters(width=64, height=64, resize_type=BICUBIC, pixel_format=RGB24, planes_pos=MERGED,
                                                                           normalization=False), width=w, height=h)
    for bad in (dict(items=[(1,) + c]), dict(border=(256, 128, 128)), dict(border=(114, -1, 128)), dict(items=[(0, float("nan")) + c[1:]]), dict(items=[])):
        with pytest.raises(RuntimeError, match="-3"):
            call(**bad)
    with pytest.raises(RuntimeError, match="-2"):
        call(items=[(0, 2.0 ** 25) + c[1:]])
    with pytest.raises(RuntimeError, match="-2"):  # tensor rule 3 behind the request's own status: a merged tensor
        call(dtype=torch.float16, norm=True)
    with pytest.raises(RuntimeError, match="-3"):  # rule 2
        call(fcc=BGR24, planes=PLANAR, norm=True, dtype=torch.float16, std=0.0)
    out = call(fcc=Y800, norm=True, dtype=torch.float16)
    torch.cuda.synchronize()
    assert out.dtype == torch.float16 and tuple(out.shape) == (1, 1, 64, 64)
    # the C entry point
    fr = (N.NV12 * 1)(N.NV12(y.data_ptr(), uv.data_ptr(), pitch, pitch, w, h))
    buf = torch.empty(64 * 64 * 3 * 4, dtype=torch.uint8, device="cuda")
    outs = (ctypes.c_void_p * 1)(buf.data_ptr())
    T_ = N.Warp if len(c) == 6 else N.Persp
    recs = (T_ * 1)(T_(0, (ctypes.c_float * len(c))(*c)))
    entry = getattr(N.lib(), "tsvpp_convert_" + path.name)
    spec = N.TensorSpec(N.TSVPP_F32, (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1))
    for p, sp in ((N.Params(0, 0, 0, 0, 64, 64, BICUBIC, RGB24, MERGED, 0), None), (N.Params(0, 0, 0, 0, 64, 64, BICUBIC, BGR24, PLANAR, 1), ctypes.byref(spec))):
        def raw(ctx, outs):
            return entry(ctx, 1, fr, 1, recs, ctypes.byref(p), sp, -1, -1, -1, outs, None)
        fr[0].uv = None
        assert raw(vpp._ctx, outs) == -3
        fr[0].uv = uv.data_ptr()
        outs[0] = None
        assert raw(vpp._ctx, outs) == -3
        assert raw(vpp._ctx, None) == -3
        outs[0] = buf.data_ptr()
        assert raw(None, outs) == -3
        assert raw(vpp._ctx, outs) == 0
    torch.cuda.synchronize()
