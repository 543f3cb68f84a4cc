"""GPU: tsvpp_convert_mesh_tensor -- the meshes of tests/test_gpu_mesh.py as what a network takes: fp32 / fp16 / bf16 elements of (q - mean[c]) * scale[c], planar
RGB / BGR or Y800.  q is the fp32 value tsvpp_convert_mesh stores (the oracle's conversion of the model's virtual frame of E(mesh), tests/mesh_util.py and
tests/remap_util.py); the element is tests/tensor_util.py's restatement of the store.  Every comparison is np.array_equal on the raw bytes."""
import pytest

import coord_suite as cs
import tensor_util as T
from coord_paths import MESH as PATH, mesh_full_set as full_set, padded_to_device
from coord_suite import FORMATS, to_device

pytestmark = pytest.mark.gpu

CASES = [((70, 66), (16, 8)), ((112, 112), (4, 4))]
frames = cs.frames_fixture(1500)


@pytest.mark.parametrize("dst,cell", CASES)
@pytest.mark.parametrize("dtype", [T.F16, T.BF16])
def test_mesh_set_with_imagenet_statistics(vpp, oracle, frames, dtype, dst, cell):
    """the whole mesh set of tests/test_gpu_mesh.py in one call (two launches), planar RGB / BGR and Y800, replicate and a constant border (the border sample goes
    through the spec like every sample)"""
    host, dev = frames
    items = full_set(dst, cell)
    items.dev = [to_device(m) for _, m in items.tables[:-1]] + [padded_to_device(items.tables[-1][1])]
    for fcc, planes in FORMATS:
        for border in (None, (114, 128, 128)):
            cs.check_tensor(PATH, vpp, oracle, host, dev, items, dst, fcc, planes, dtype, "imagenet", border)


def test_identity_fp32_is_convert_mesh(vpp, frames):
    for dst, cell in CASES:
        cs.identity_fp32_is_the_plain_call(PATH, vpp, frames, PATH.resident(full_set(dst, cell)), dst)


def test_refusals(vpp, frames):
    cs.tensor_refusals(PATH, vpp, frames)
