"""GPU: tsvpp_convert_mesh_bicubic is, bit for bit, tsvpp_convert_remap_bicubic of tsvpp_mesh_expand(mesh), which tests/test_gpu_remap_bicubic.py holds to the
model; the cases every coordinate path has run there too, for both calls."""
import numpy as np
import pytest
import torch

import coord_paths as cp
import coord_suite as cs
import mesh_util as M
import tensor_util as T
from coord_bicubic_paths import BORDERS, DSTS, GEO, TENSORS
from letterbox_util import FLAVOURS
from map_bicubic_paths import MESH_BICUBIC as PATH, REMAP_BICUBIC as DENSE

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cell", [(16, 16), (4, 4)])
@pytest.mark.parametrize("dst", DSTS)
def test_bits_are_the_dense_calls_on_the_expanded_mesh(vpp, dst, cell):
    """every frame through its four meshes (garbage holds NaN, infinities and subnormals; the last mesh travels pitch-padded with NaN) in every colour flavour
    and three tensor forms, replicate and a border"""
    import tensor_stream as ts
    _, dev = cs.device_frames(GEO, 1900 + 5)
    items = cp.mesh_pick([(k, nm) for k in range(len(GEO)) for nm in cp.MESH_NAMES], GEO, dst, cell=cell)
    items.dev = [cs.to_device(t) for _, t in items.tables[:-1]] + [cp.padded_to_device(items.tables[-1][1])]
    dense = cp.remap_tables([(nm, M.expand(t, *dst, cell)) for nm, t in items.tables], items.remaps)
    kw = dict(width=[g[0] for g in GEO], height=[g[1] for g in GEO])
    forms = [(f, {}) for f in FLAVOURS] + [((fcc, planes, True), dict(dtype=T.TORCH[dt], mean=T.SPECS[sp][0], std=T.SPECS[sp][1])) for dt, sp, fcc, planes in TENSORS]
    for border in BORDERS:
        for flavour, tensor in forms:
            fp = cs.params(ts, dst, *flavour)
            a, b = (path.call(vpp, [d[0] for d in dev], [d[1] for d in dev], its, fp, border=border, **kw, **tensor) for path, its in ((PATH, items), (DENSE, dense)))
            torch.cuda.synchronize()
            for i in range(len(items.remaps)):
                assert np.array_equal(T.bits(a[i]), T.bits(b[i])), (items.tables[items.remaps[i][1]][0], dst, cell, flavour, sorted(tensor), border)
