"""GPU: tsvpp_convert_mesh_tensor -- the meshes of tests/test_gpu_mesh.py as what a network takes: fp32 / fp16 / bf16 elements of (q - mean[c]) * scale[c], planar
RGB / BGR or Y800.  q is the fp32 value tsvpp_convert_mesh stores (the oracle's conversion of the model's virtual frame of E(mesh), tests/mesh_util.py and
tests/remap_util.py); the element is tests/tensor_util.py's restatement of the store.  Every comparison is np.array_equal on the raw bytes."""
import numpy as np
import pytest
import torch

import mesh_util as M
import remap_util as R
import tensor_util as T
from letterbox_util import BGR24, MERGED, PLANAR, RGB24, Y800
from test_gpu_mesh import full_set, padded_to_device
from test_gpu_remap import GEO, frames, params, to_device, virtual  # noqa: F401  (frames: the module's fixture)

pytestmark = pytest.mark.gpu

FORMATS = [(RGB24, PLANAR), (BGR24, PLANAR), (Y800, MERGED)]
CASES = [((70, 66), (16, 8)), ((112, 112), (4, 4))]


def _fp(dst, fcc, planes, norm=True):
    import tensor_stream as ts
    return params(ts, dst, fcc, planes, norm)


@pytest.mark.parametrize("dst,cell", CASES)
@pytest.mark.parametrize("dtype", [T.F16, T.BF16])
def test_mesh_set_with_imagenet_statistics(vpp, oracle, frames, dtype, dst, cell):
    """the whole mesh set of tests/test_gpu_mesh.py in one call (two launches), planar RGB / BGR and Y800, replicate and a constant border (the border sample goes
    through the spec like every sample)"""
    host, dev = frames
    meshes, remaps = full_set(dst, cell)
    dev_meshes = [to_device(m) for _, m in meshes[:-1]] + [padded_to_device(meshes[-1][1])]
    dense = [M.expand(m, *dst, cell) for _, m in meshes]
    for fcc, planes in FORMATS:
        channels = 1 if fcc == Y800 else 3
        for border in (None, (114, 128, 128)):
            got = vpp.convert_mesh([d[0] for d in dev], [d[1] for d in dev], dev_meshes, _fp(dst, fcc, planes), cell=cell, remaps=remaps, border=border,
                                   width=[g[0] for g in GEO], height=[g[1] for g in GEO], dtype=T.TORCH[dtype], mean=T.IMAGENET[0], std=T.IMAGENET[1])
            torch.cuda.synchronize()
            assert got.dtype == T.TORCH[dtype]
            for i, (k, m) in enumerate(remaps):
                name = meshes[m][0]
                q = R.expected(oracle, None, None, 0, 0, dense[m], fcc, planes, True, border,
                               virtual=virtual(host, k, GEO, ("mesh", name, cell, None), dense[m], border)).view(np.float32)
                ref = T.expected(q, channels, T.IMAGENET, dtype)
                g = T.bits(got[i])
                assert g.size == ref.size, (i, g.size, ref.size)
                bad = np.flatnonzero(g != ref)
                assert bad.size == 0, f"output {i}: frame {k} mesh {name} cell {cell} -> {dst} fcc={fcc} {dtype} border={border}: {bad.size} bytes differ, first at {bad[:4]}"


def test_identity_fp32_is_convert_mesh(vpp, frames):
    """mean 0, std 1, float32: (q - 0) * 1 is q -- the tensor call stores the bits of tsvpp_convert_mesh"""
    host, dev = frames
    for dst, cell in CASES:
        meshes, remaps = full_set(dst, cell)
        dev_meshes = [to_device(m) for _, m in meshes]
        kw = dict(cell=cell, remaps=remaps, width=[g[0] for g in GEO], height=[g[1] for g in GEO], border=(3, 250, 7))
        ys, uvs = [d[0] for d in dev], [d[1] for d in dev]
        for fcc, planes in FORMATS:
            a = vpp.convert_mesh(ys, uvs, dev_meshes, _fp(dst, fcc, planes), **kw)
            b = vpp.convert_mesh(ys, uvs, dev_meshes, _fp(dst, fcc, planes), dtype=torch.float32, mean=0.0, std=1.0, **kw)
            torch.cuda.synchronize()
            assert np.array_equal(T.bits(a), T.bits(b)), (dst, fcc, planes)


def test_refusals(vpp, frames):
    host, dev = frames
    y, uv = dev[0]
    mesh = to_device(M.translation(64, 64, (16, 16), 4, 2))
    kw = dict(width=GEO[0][0], height=GEO[0][1], dtype=torch.float16, cell=(16, 16))
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_mesh(y, uv, mesh, _fp((64, 64), RGB24, MERGED), **kw)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_mesh(y, uv, mesh, _fp((64, 64), RGB24, PLANAR, norm=False), **kw)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_mesh(y, uv, mesh, _fp((64, 64), RGB24, PLANAR), std=0.0, **kw)
    with pytest.raises(RuntimeError, match="-3"):  # rule 1 first: the request's own status
        vpp.convert_mesh(y, uv, mesh, _fp((64, 64), RGB24, MERGED), remaps=[(0, 3)], **kw)
    out = vpp.convert_mesh(y, uv, mesh, _fp((64, 64), Y800, MERGED), **kw)
    torch.cuda.synchronize()
    assert out.dtype == torch.float16 and tuple(out.shape) == (1, 1, 64, 64)
