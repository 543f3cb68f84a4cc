"""GPU: tsvpp_convert_warp_tensor -- the warps of tests/test_gpu_warp.py as what a network takes: fp32 / fp16 / bf16 elements of (q - mean[c]) * scale[c], planar
RGB / BGR or Y800.  q is the fp32 value tsvpp_convert_warp stores (the oracle's conversion of the model's virtual frame, tests/warp_util.py); the element is
tests/tensor_util.py's restatement of the store.  Every comparison is np.array_equal on the raw bytes."""
import numpy as np
import pytest
import torch

import tensor_util as T
import warp_util as W
from letterbox_util import BGR24, MERGED, PLANAR, RGB24, Y800
from test_gpu_warp import BORDERS, DSTS, GEO, check, frames, matrices, params, virtual  # noqa: F401  (frames: the module's fixture)

pytestmark = pytest.mark.gpu

FORMATS = [(RGB24, PLANAR), (BGR24, PLANAR), (Y800, MERGED)]


def check_tensor(v, oracle, host, dev, warps, dst, fcc, planes, dtype, spec, border, what=""):
    channels = 1 if fcc == Y800 else 3
    got = v.convert_warp([d[0] for d in dev], [d[1] for d in dev], [(k,) + m for k, m in warps], _fp(dst, fcc, planes), border=border, width=[g[0] for g in GEO],
                         height=[g[1] for g in GEO], dtype=T.TORCH[dtype], mean=SPEC[spec][0], std=SPEC[spec][1])
    torch.cuda.synchronize()
    assert got.dtype == T.TORCH[dtype]
    for i, (k, m) in enumerate(warps):
        q = W.expected(oracle, None, None, 0, 0, m, dst, fcc, planes, True, border, virtual=virtual(host, k, GEO, m, dst, border)).view(np.float32)
        ref = T.expected(q, channels, SPEC[spec], dtype)
        g = T.bits(got[i])
        assert g.size == ref.size, (what, i, g.size, ref.size)
        bad = np.flatnonzero(g != ref)
        assert bad.size == 0, f"{what} warp {i}: frame {k} m={m} -> {dst} fcc={fcc} {dtype} {spec} border={border}: {bad.size} bytes differ, first at {bad[:4]}"
    return got


SPEC = T.SPECS


def _fp(dst, fcc, planes, norm=True):
    import tensor_stream as ts
    return params(ts, dst, fcc, planes, norm)


@pytest.mark.parametrize("dst", DSTS)
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_scale_only_and_matrix_set(vpp, oracle, frames, dtype, dst):
    """cases 1 and 2 of tests/test_gpu_warp.py in every dtype x spec, planar RGB / BGR and Y800: scale-only matrices under both border modes, the matrix set under
    replicate and two constant borders (the border pixel goes through the spec like every sample)"""
    host, dev = frames
    scale = [(k, W.scale_only(w, h, *dst)) for k, (w, h, _) in enumerate(GEO)]
    full = [(k, m) for k, (w, h, _) in enumerate(GEO) for m in matrices(w, h, *dst).values()]
    for spec in SPEC:
        for fcc, planes in FORMATS:
            for border in (None, (114, 128, 128)):
                check_tensor(vpp, oracle, host, dev, scale, dst, fcc, planes, dtype, spec, border, what="scale-only")
            for border in BORDERS:
                check_tensor(vpp, oracle, host, dev, full, dst, fcc, planes, dtype, spec, border, what="set")


def test_identity_fp32_is_convert_warp(vpp, frames):
    """mean 0, std 1, float32: (q - 0) * 1 is q -- the tensor call stores the bits of tsvpp_convert_warp"""
    host, dev = frames
    dst = (70, 66)
    warps = [(k,) + m for k, (w, h, _) in enumerate(GEO) for m in matrices(w, h, *dst).values()]
    kw = dict(width=[g[0] for g in GEO], height=[g[1] for g in GEO], border=(3, 250, 7))
    ys, uvs = [d[0] for d in dev], [d[1] for d in dev]
    for fcc, planes in FORMATS:
        a = vpp.convert_warp(ys, uvs, warps, _fp(dst, fcc, planes), **kw)
        b = vpp.convert_warp(ys, uvs, warps, _fp(dst, fcc, planes), dtype=torch.float32, mean=0.0, std=1.0, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(T.bits(a), T.bits(b)), (fcc, planes)


def test_border_pixel_goes_through_the_spec(vpp, oracle, frames):
    """a warp wholly outside the frame is the border sample everywhere: one value per channel, the spec's image of the colour conversion of (Y, U, V)"""
    from letterbox_util import pad_pixel
    host, dev = frames
    border = (114, 128, 128)
    for dtype in T.DTYPES:
        got = vpp.convert_warp(dev[0][0], dev[0][1], [(1, 0, 5000, 0, 1, -3000)], _fp((64, 64), BGR24, PLANAR), border=border, width=GEO[0][0], height=GEO[0][1],
                               dtype=T.TORCH[dtype], mean=T.IMAGENET[0], std=T.IMAGENET[1])
        torch.cuda.synchronize()
        px = pad_pixel(oracle, border, BGR24, PLANAR, True)
        want = T.expected(np.repeat(px.astype(np.float32), 64 * 64), 3, T.IMAGENET, dtype)
        assert np.array_equal(T.bits(got[0]), want), dtype


def test_refusals(vpp, frames):
    host, dev = frames
    y, uv = dev[0]
    m = W.scale_only(GEO[0][0], GEO[0][1], 64, 64)
    kw = dict(width=GEO[0][0], height=GEO[0][1], dtype=torch.float16)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_warp(y, uv, [m], _fp((64, 64), RGB24, MERGED), **kw)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_warp(y, uv, [m], _fp((64, 64), RGB24, PLANAR, norm=False), **kw)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_warp(y, uv, [m], _fp((64, 64), RGB24, PLANAR), std=0.0, **kw)
    with pytest.raises(RuntimeError, match="-3"):  # rule 1 first: the request's own status
        vpp.convert_warp(y, uv, [(3,) + m], _fp((64, 64), RGB24, MERGED), **kw)
    out = vpp.convert_warp(y, uv, [m], _fp((64, 64), Y800, MERGED), **kw)
    torch.cuda.synchronize()
    assert out.dtype == torch.float16 and tuple(out.shape) == (1, 1, 64, 64)
