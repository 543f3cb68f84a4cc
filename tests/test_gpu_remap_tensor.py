"""GPU: tsvpp_convert_remap_tensor -- the maps of tests/test_gpu_remap.py as what a network takes: fp32 / fp16 / bf16 elements of (q - mean[c]) * scale[c], planar
RGB / BGR or Y800.  q is the fp32 value tsvpp_convert_remap stores (the oracle's conversion of the model's virtual frame, tests/remap_util.py); the element is
tests/tensor_util.py's restatement of the store.  Every comparison is np.array_equal on the raw bytes."""
import numpy as np
import pytest
import torch

import remap_util as R
import tensor_util as T
from letterbox_util import BGR24, MERGED, PLANAR, RGB24, Y800
from test_gpu_remap import GEO, frames, full_set, padded_to_device, params, to_device, virtual  # noqa: F401  (frames: the module's fixture)

pytestmark = pytest.mark.gpu

FORMATS = [(RGB24, PLANAR), (BGR24, PLANAR), (Y800, MERGED)]
DSTS = [(70, 66), (112, 112)]


def _fp(dst, fcc, planes, norm=True):
    import tensor_stream as ts
    return params(ts, dst, fcc, planes, norm)


@pytest.mark.parametrize("dst", DSTS)
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_map_set_with_imagenet_statistics(vpp, oracle, frames, dtype, dst):
    """the whole map set of tests/test_gpu_remap.py in one call, planar RGB / BGR and Y800, replicate and a constant border (the border sample goes through the
    spec like every sample)"""
    host, dev = frames
    maps, remaps = full_set(dst)
    dev_maps = [to_device(xy) for _, xy in maps[:-1]] + [padded_to_device(maps[-1][1])]
    for fcc, planes in FORMATS:
        channels = 1 if fcc == Y800 else 3
        for border in (None, (114, 128, 128)):
            got = vpp.convert_remap([d[0] for d in dev], [d[1] for d in dev], dev_maps, _fp(dst, fcc, planes), remaps=remaps, border=border,
                                    width=[g[0] for g in GEO], height=[g[1] for g in GEO], dtype=T.TORCH[dtype], mean=T.IMAGENET[0], std=T.IMAGENET[1])
            torch.cuda.synchronize()
            assert got.dtype == T.TORCH[dtype]
            for i, (k, m) in enumerate(remaps):
                name, xy = maps[m]
                q = R.expected(oracle, None, None, 0, 0, xy, fcc, planes, True, border, virtual=virtual(host, k, GEO, (name, None), xy, border)).view(np.float32)
                ref = T.expected(q, channels, T.IMAGENET, dtype)
                g = T.bits(got[i])
                assert g.size == ref.size, (i, g.size, ref.size)
                bad = np.flatnonzero(g != ref)
                assert bad.size == 0, f"output {i}: frame {k} map {name} -> {dst} fcc={fcc} {dtype} border={border}: {bad.size} bytes differ, first at {bad[:4]}"


def test_identity_fp32_is_convert_remap(vpp, frames):
    """mean 0, std 1, float32: (q - 0) * 1 is q -- the tensor call stores the bits of tsvpp_convert_remap"""
    host, dev = frames
    for dst in DSTS:
        maps, remaps = full_set(dst)
        dev_maps = [to_device(xy) for _, xy in maps]
        kw = dict(remaps=remaps, width=[g[0] for g in GEO], height=[g[1] for g in GEO], border=(3, 250, 7))
        ys, uvs = [d[0] for d in dev], [d[1] for d in dev]
        for fcc, planes in FORMATS:
            a = vpp.convert_remap(ys, uvs, dev_maps, _fp(dst, fcc, planes), **kw)
            b = vpp.convert_remap(ys, uvs, dev_maps, _fp(dst, fcc, planes), dtype=torch.float32, mean=0.0, std=1.0, **kw)
            torch.cuda.synchronize()
            assert np.array_equal(T.bits(a), T.bits(b)), (dst, fcc, planes)


def test_refusals(vpp, frames):
    host, dev = frames
    y, uv = dev[0]
    xy = to_device(R.translation(64, 64, 4, 2))
    kw = dict(width=GEO[0][0], height=GEO[0][1], dtype=torch.float16)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_remap(y, uv, xy, _fp((64, 64), RGB24, MERGED), **kw)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_remap(y, uv, xy, _fp((64, 64), RGB24, PLANAR, norm=False), **kw)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_remap(y, uv, xy, _fp((64, 64), RGB24, PLANAR), std=0.0, **kw)
    with pytest.raises(RuntimeError, match="-3"):  # rule 1 first: the request's own status
        vpp.convert_remap(y, uv, xy, _fp((64, 64), RGB24, MERGED), remaps=[(0, 3)], **kw)
    out = vpp.convert_remap(y, uv, xy, _fp((64, 64), Y800, MERGED), **kw)
    torch.cuda.synchronize()
    assert out.dtype == torch.float16 and tuple(out.shape) == (1, 1, 64, 64)
