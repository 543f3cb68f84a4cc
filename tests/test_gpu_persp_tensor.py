"""GPU: tsvpp_convert_perspective_tensor -- the homographies of tests/test_gpu_persp.py as what a network takes: fp32 / fp16 / bf16 elements of
(q - mean[c]) * scale[c], planar RGB / BGR or Y800.  q is the fp32 value tsvpp_convert_perspective stores (the oracle's conversion of the model's virtual frame,
tests/persp_util.py); the element is tests/tensor_util.py's restatement of the store.  Every comparison is np.array_equal on the raw bytes."""
import numpy as np
import pytest
import torch

import persp_util as P
import tensor_util as T
from letterbox_util import BGR24, MERGED, PLANAR, RGB24, Y800
from test_gpu_persp import BORDERS, DSTS, GEO, frames, full_set, homographies, params, virtual  # noqa: F401  (frames: the fixture)

pytestmark = pytest.mark.gpu

FORMATS = [(RGB24, PLANAR), (BGR24, PLANAR), (Y800, MERGED)]
SPEC = T.SPECS


def _fp(dst, fcc, planes, norm=True):
    import tensor_stream as ts
    return params(ts, dst, fcc, planes, norm)


def check_tensor(v, oracle, host, dev, persps, dst, fcc, planes, dtype, spec, border, what=""):
    channels = 1 if fcc == Y800 else 3
    got = v.convert_perspective([d[0] for d in dev], [d[1] for d in dev], [(k,) + h for k, h in persps], _fp(dst, fcc, planes), border=border,
                                width=[g[0] for g in GEO], height=[g[1] for g in GEO], dtype=T.TORCH[dtype], mean=SPEC[spec][0], std=SPEC[spec][1])
    torch.cuda.synchronize()
    assert got.dtype == T.TORCH[dtype]
    for i, (k, h) in enumerate(persps):
        q = P.expected(oracle, None, None, 0, 0, h, dst, fcc, planes, True, border, virtual=virtual(host, k, GEO, h, dst, border)).view(np.float32)
        ref = T.expected(q, channels, SPEC[spec], dtype)
        g = T.bits(got[i])
        assert g.size == ref.size, (what, i, g.size, ref.size)
        bad = np.flatnonzero(g != ref)
        assert bad.size == 0, f"{what} output {i}: frame {k} h={h} -> {dst} fcc={fcc} {dtype} {spec} border={border}: {bad.size} bytes differ, first at {bad[:4]}"
    return got


@pytest.mark.parametrize("dst", DSTS)
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_homography_set(vpp, oracle, frames, dtype, dst):
    """the homography set in every dtype x spec (ImageNet mean / std and identity), planar RGB / BGR and Y800, under replicate and two constant borders (the
    border pixel goes through the spec like every sample)"""
    host, dev = frames
    full = full_set(dst)
    for spec in SPEC:
        for fcc, planes in FORMATS:
            for border in BORDERS:
                check_tensor(vpp, oracle, host, dev, full, dst, fcc, planes, dtype, spec, border, what="set")


def test_identity_fp32_is_convert_perspective(vpp, frames):
    """mean 0, std 1, float32: (q - 0) * 1 is q -- the tensor call stores the bits of tsvpp_convert_perspective"""
    host, dev = frames
    dst = (70, 66)
    persps = [(k,) + h for k, h in full_set(dst)]
    kw = dict(width=[g[0] for g in GEO], height=[g[1] for g in GEO], border=(3, 250, 7))
    ys, uvs = [d[0] for d in dev], [d[1] for d in dev]
    for fcc, planes in FORMATS:
        a = vpp.convert_perspective(ys, uvs, persps, _fp(dst, fcc, planes), **kw)
        b = vpp.convert_perspective(ys, uvs, persps, _fp(dst, fcc, planes), dtype=torch.float32, mean=0.0, std=1.0, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(T.bits(a), T.bits(b)), (fcc, planes)


def test_refusals(vpp, frames):
    host, dev = frames
    y, uv = dev[0]
    q = homographies(GEO[0][0], GEO[0][1], 64, 64)["mild"]
    kw = dict(width=GEO[0][0], height=GEO[0][1], dtype=torch.float16)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_perspective(y, uv, [q], _fp((64, 64), RGB24, MERGED), **kw)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_perspective(y, uv, [q], _fp((64, 64), RGB24, PLANAR, norm=False), **kw)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_perspective(y, uv, [q], _fp((64, 64), RGB24, PLANAR), std=0.0, **kw)
    with pytest.raises(RuntimeError, match="-3"):  # rule 1 first: the request's own status
        vpp.convert_perspective(y, uv, [(3,) + q], _fp((64, 64), RGB24, MERGED), **kw)
    out = vpp.convert_perspective(y, uv, [q], _fp((64, 64), Y800, MERGED), **kw)
    torch.cuda.synchronize()
    assert out.dtype == torch.float16 and tuple(out.shape) == (1, 1, 64, 64)
