"""GPU: tsvpp_convert_perspective_tensor -- the homographies of tests/test_gpu_persp.py as what a network takes: fp32 / fp16 / bf16 elements of
(q - mean[c]) * scale[c], planar RGB / BGR or Y800.  q is the fp32 value tsvpp_convert_perspective stores (the oracle's conversion of the model's virtual frame,
tests/persp_util.py); the element is tests/tensor_util.py's restatement of the store.  Every comparison is np.array_equal on the raw bytes."""
import pytest

import coord_suite as cs
import tensor_util as T
from coord_paths import PERSP as PATH, homographies, persp_full_set as full_set
from coord_suite import BORDERS, DSTS, FORMATS, GEO

pytestmark = pytest.mark.gpu

frames = cs.frames_fixture(1300)


@pytest.mark.parametrize("dst", DSTS)
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_homography_set(vpp, oracle, frames, dtype, dst):
    """the homography set in every dtype x spec (ImageNet mean / std and identity), planar RGB / BGR and Y800, under replicate and two constant borders (the
    border pixel goes through the spec like every sample)"""
    host, dev = frames
    full = full_set(dst)
    for spec in T.SPECS:
        for fcc, planes in FORMATS:
            for border in BORDERS:
                cs.check_tensor(PATH, vpp, oracle, host, dev, full, dst, fcc, planes, dtype, spec, border, what="set")


def test_identity_fp32_is_convert_perspective(vpp, frames):
    cs.identity_fp32_is_the_plain_call(PATH, vpp, frames, full_set((70, 66)), (70, 66))


def test_refusals(vpp, frames):
    cs.tensor_refusals(PATH, vpp, frames, items=[(0, homographies(GEO[0][0], GEO[0][1], 64, 64)["mild"])])  # a true projective row
