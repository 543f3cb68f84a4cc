"""GPU: tsvpp_convert_warp, tsvpp_convert_perspective, tsvpp_convert_remap and their tensor forms against tests/sampler64.py -- the independent float64 evaluation
of what include/tsvpp.h promises in words, with its derived bound -- and not against the models of tests/*_util.py, which tests/test_sampler64_cpu.py holds to
the same judge.  Every output element must lie in its bracket lo <= got <= hi, which is equality wherever the sample brackets are single-valued (all but about
one sample in a hundred); no element is left out, there is no tolerance beyond the derived delta.  The tests name no kernel: they run unchanged under the knob
matrix."""
import numpy as np
import pytest
import torch

import remap_util as R  # (the map generators only: inputs, not the model)
import sampler64 as S
import tensor_util as T
from letterbox_util import BGR24, BILINEAR, FLAVOURS, MERGED, PLANAR, RGB24
from util import synth_nv12

pytestmark = pytest.mark.gpu

# the frames of a call: the three noise frames of sampler64.FRAMES, then the band-limited frame at the largest size
GEO = S.FRAMES + [S.FRAMES[0]]
TABLES = {"warp": S.AFFINE, "perspective": S.PERSPECTIVE, "remap": S.REMAP}
CALLS = list(TABLES)
BORDER = (3, 250, 7)
BRIEF = [(RGB24, PLANAR, False), (BGR24, MERGED, True)]  # uint8 planar plus fp32 merged


@pytest.fixture(scope="module")
def frames():
    host = [synth_nv12(w, h, seed=6400 + k, pitch=p) for k, (w, h, p) in enumerate(S.FRAMES)] + [S.smooth_nv12(*S.FRAMES[0][:2], seed=6400, pitch=S.FRAMES[0][2])]
    dev = [(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()) for y, uv in host]
    return host, dev


def params(dst, fcc, planes, norm):
    import tensor_stream as ts
    return ts.FrameParameters(width=dst[0], height=dst[1], resize_type=BILINEAR, pixel_format=fcc, planes_pos=planes, normalization=norm)


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def argument(call, name, k, dst):
    """the matrix, homography or map of case `name` on frame k"""
    w, h, _ = GEO[k]
    return cached(("arg", call, name, (w, h), dst), lambda: TABLES[call][name](R, w, h, *dst) if call == "remap" else TABLES[call][name](w, h, *dst))


def samples(host, call, name, k, dst, border):
    """the sample brackets of (case, frame, dst, border), once per module"""
    def make():
        arg = argument(call, name, k, dst)
        grids = {"warp": S.affine_positions, "perspective": S.perspective_positions}[call](arg, *dst) if call != "remap" else S.remap_positions(arg)
        return S.virtual_bracket(host[k][0], host[k][1], GEO[k][0], GEO[k][1], grids, border)
    return cached(("vb", call, name, k, dst, border), make)


def to_device(xy):
    return torch.from_numpy(np.ascontiguousarray(xy)).cuda()


def launch(v, call, dev, items, dst, fp, border, dev_maps=None, **tensor):
    """one call for items = [(frame, case name)]"""
    ys, uvs = [d[0] for d in dev], [d[1] for d in dev]
    kw = dict(border=border, width=[g[0] for g in GEO], height=[g[1] for g in GEO], **tensor)
    args = [argument(call, name, k, dst) for k, name in items]
    if call == "warp":
        got = v.convert_warp(ys, uvs, [(k,) + a for (k, _), a in zip(items, args)], fp, **kw)
    elif call == "perspective":
        got = v.convert_perspective(ys, uvs, [(k,) + a for (k, _), a in zip(items, args)], fp, **kw)
    else:
        maps = [to_device(a) for a in args] if dev_maps is None else dev_maps
        got = v.convert_remap(ys, uvs, maps, fp, remaps=[(k, i) for i, (k, _) in enumerate(items)], **kw)
    torch.cuda.synchronize()
    return got


def check(v, oracle, host, dev, call, items, dst, fcc, planes, norm, border, what="", dev_maps=None):
    got = launch(v, call, dev, items, dst, params(dst, fcc, planes, norm), border, dev_maps)
    for i, (k, name) in enumerate(items):
        lo, hi = cached(("out", call, name, k, dst, border, fcc, planes, norm),
                        lambda: S.output_bracket(oracle, samples(host, call, name, k, dst, border), fcc, planes, norm))
        g = T.bits(got[i])
        bad = S.outside(g.view(np.float32) if norm else g, lo, hi)
        assert bad.size == 0, (f"{what} {call} output {i}: case {name} on frame {k} {GEO[k]} -> {dst} fcc={fcc} planes={planes} norm={norm} border={border}: "
                               f"{bad.size} elements outside their bracket, first at {bad[:4]}")
    return got


def everything(call):
    return [(k, name) for k in range(len(GEO)) for name in TABLES[call]]


@pytest.mark.parametrize("dst", S.DSTS)
@pytest.mark.parametrize("call", CALLS)
def test_case_set_inside_the_bracket(vpp, oracle, frames, call, dst):
    """every case on every frame in one call, replicate and a constant border; every flavour at 70 x 66, uint8 planar and fp32 merged at the other sizes"""
    host, dev = frames
    for border in (None, BORDER):
        for fcc, planes, norm in (FLAVOURS if dst == S.DSTS[0] else BRIEF):
            check(vpp, oracle, host, dev, call, everything(call), dst, fcc, planes, norm, border)


@pytest.mark.parametrize("call", CALLS)
def test_more_than_one_launch(vpp, oracle, frames, call):
    """one call of 38 outputs over all frames: the split into launches and the frame index"""
    host, dev = frames
    names = list(TABLES[call])
    items = [(i % len(GEO), names[(i // len(GEO)) % len(names)]) for i in range(38)]
    assert len({k for k, _ in items}) == len(GEO) and len(set(items)) > 12
    check(vpp, oracle, host, dev, call, items, (30, 34), BGR24, PLANAR, True, BORDER, what="38 outputs")
    check(vpp, oracle, host, dev, call, items, (30, 34), RGB24, MERGED, False, None, what="38 outputs")


@pytest.mark.parametrize("call", CALLS)
def test_staged_gather_and_mixed_launches(oracle, frames, monkeypatch, call):
    """a context of its own per TSVPP_LDS_KB (read when a context is created): the default budget, 0 (every tile gathers) and 3 KiB (tiles that stage and tiles
    that gather in one launch) all stay inside the bracket"""
    import tensor_stream as ts
    host, dev = frames
    items = [(0, name) for name in TABLES[call]] + [(3, name) for name in TABLES[call]]
    for kb in (None, "0", "3"):
        if kb is not None:
            monkeypatch.setenv("TSVPP_LDS_KB", kb)
        v = ts.VideoProcessor(device=0, max_consumers=1)
        try:
            check(v, oracle, host, dev, call, items, (112, 112), BGR24, PLANAR, True, None, what=f"LDS_KB={kb}")
            check(v, oracle, host, dev, call, items, (112, 112), RGB24, MERGED, False, BORDER, what=f"LDS_KB={kb}")
        finally:
            v.Close()


def test_remap_padded_map_and_a_hint_too_small(vpp, oracle, frames):
    """the maps with a row stride of 2 * dst_w + 6 floats and NaN in the padding; and with an LDS hint of 256 bytes, which no tile's footprint fits"""
    host, dev = frames
    dst = (70, 66)
    items = [(2, "barrel"), (0, "affine"), (1, "leaving")]
    tight = [to_device(argument("remap", name, k, dst)) for k, name in items]
    padded = []
    for k, name in items:
        view, back = R.padded(argument("remap", name, k, dst))
        t = torch.from_numpy(back).cuda()
        assert torch.isnan(t[:, 2 * dst[0]:]).all()
        padded.append(t[:, :2 * dst[0]].unflatten(1, (dst[0], 2)))
    for dev_maps, what in ((padded, "padded"), ([(t, 256) for t in tight], "hint 256")):
        for border in (None, BORDER):
            for fcc, planes, norm in BRIEF:
                check(vpp, oracle, host, dev, "remap", items, dst, fcc, planes, norm, border, what=what, dev_maps=dev_maps)


@pytest.mark.parametrize("call", CALLS)
def test_tensor_forms_inside_the_bracket(vpp, oracle, frames, call):
    """fp16 and bf16 with ImageNet mean / std, and the corner spec with its scale of -1 (the order of lo and hi swaps): the bracket sent through
    tests/tensor_util.py's expression, compared as values"""
    host, dev = frames
    dst = (70, 66)
    items = everything(call)
    for dtype, spec, fcc in ((T.F16, "imagenet", RGB24), (T.BF16, "imagenet", BGR24), (T.F16, "corner", RGB24)):
        mean, std = T.SPECS[spec]
        for border in (None, BORDER):
            got = launch(vpp, call, dev, items, dst, params(dst, fcc, PLANAR, True), border, dtype=T.TORCH[dtype], mean=mean, std=std)
            assert got.dtype == T.TORCH[dtype]
            for i, (k, name) in enumerate(items):
                lo, hi = S.tensor_bracket(oracle, samples(host, call, name, k, dst, border), fcc, T.SPECS[spec], dtype)
                bad = S.outside(S.tensor_values(T.bits(got[i]), dtype), lo, hi)
                assert bad.size == 0, f"{call} {dtype} {spec} output {i}: case {name} on frame {k} border={border}: {bad.size} elements outside, first at {bad[:4]}"
