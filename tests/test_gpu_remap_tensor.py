"""GPU: tsvpp_convert_remap_tensor -- the maps of tests/test_gpu_remap.py as what a network takes: fp32 / fp16 / bf16 elements of (q - mean[c]) * scale[c], planar
RGB / BGR or Y800.  q is the fp32 value tsvpp_convert_remap stores (the oracle's conversion of the model's virtual frame, tests/remap_util.py); the element is
tests/tensor_util.py's restatement of the store.  Every comparison is np.array_equal on the raw bytes."""
import pytest

import coord_suite as cs
import tensor_util as T
from coord_paths import REMAP as PATH, padded_to_device, remap_full_set as full_set
from coord_suite import FORMATS, to_device

pytestmark = pytest.mark.gpu

DSTS = [(70, 66), (112, 112)]
frames = cs.frames_fixture(1500)


@pytest.mark.parametrize("dst", DSTS)
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_map_set_with_imagenet_statistics(vpp, oracle, frames, dtype, dst):
    """the whole map set of tests/test_gpu_remap.py in one call, planar RGB / BGR and Y800, replicate and a constant border (the border sample goes through the
    spec like every sample)"""
    host, dev = frames
    items = full_set(dst)
    items.dev = [to_device(xy) for _, xy in items.tables[:-1]] + [padded_to_device(items.tables[-1][1])]
    for fcc, planes in FORMATS:
        for border in (None, (114, 128, 128)):
            cs.check_tensor(PATH, vpp, oracle, host, dev, items, dst, fcc, planes, dtype, "imagenet", border)


def test_identity_fp32_is_convert_remap(vpp, frames):
    for dst in DSTS:
        cs.identity_fp32_is_the_plain_call(PATH, vpp, frames, PATH.resident(full_set(dst)), dst)


def test_refusals(vpp, frames):
    cs.tensor_refusals(PATH, vpp, frames)
