"""GPU: tsvpp_convert_warp_tensor -- the warps of tests/test_gpu_warp.py as what a network takes: fp32 / fp16 / bf16 elements of (q - mean[c]) * scale[c], planar
RGB / BGR or Y800.  q is the fp32 value tsvpp_convert_warp stores (the oracle's conversion of the model's virtual frame, tests/warp_util.py); the element is
tests/tensor_util.py's restatement of the store.  Every comparison is np.array_equal on the raw bytes."""
import numpy as np
import pytest
import torch

import coord_suite as cs
import tensor_util as T
import warp_util as W
from coord_paths import WARP as PATH, warp_full_set
from coord_suite import BORDERS, DSTS, FORMATS, GEO, tensor_params
from letterbox_util import BGR24, PLANAR

pytestmark = pytest.mark.gpu

frames = cs.frames_fixture(1300)


@pytest.mark.parametrize("dst", DSTS)
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_scale_only_and_matrix_set(vpp, oracle, frames, dtype, dst):
    """cases 1 and 2 of tests/test_gpu_warp.py in every dtype x spec, planar RGB / BGR and Y800: scale-only matrices under both border modes, the matrix set under
    replicate and two constant borders (the border pixel goes through the spec like every sample)"""
    host, dev = frames
    scale = [(k, W.scale_only(w, h, *dst)) for k, (w, h, _) in enumerate(GEO)]
    full = warp_full_set(dst)
    for spec in T.SPECS:
        for fcc, planes in FORMATS:
            for border in (None, (114, 128, 128)):
                cs.check_tensor(PATH, vpp, oracle, host, dev, scale, dst, fcc, planes, dtype, spec, border, what="scale-only")
            for border in BORDERS:
                cs.check_tensor(PATH, vpp, oracle, host, dev, full, dst, fcc, planes, dtype, spec, border, what="set")


def test_identity_fp32_is_convert_warp(vpp, frames):
    cs.identity_fp32_is_the_plain_call(PATH, vpp, frames, warp_full_set((70, 66)), (70, 66))


def test_border_pixel_goes_through_the_spec(vpp, oracle, frames):
    """a warp wholly outside the frame is the border sample everywhere: one value per channel, the spec's image of the colour conversion of (Y, U, V)"""
    from letterbox_util import pad_pixel
    host, dev = frames
    border = (114, 128, 128)
    for dtype in T.DTYPES:
        got = vpp.convert_warp(dev[0][0], dev[0][1], [(1, 0, 5000, 0, 1, -3000)], tensor_params((64, 64), BGR24, PLANAR), border=border, width=GEO[0][0], height=GEO[0][1],
                               dtype=T.TORCH[dtype], mean=T.IMAGENET[0], std=T.IMAGENET[1])
        torch.cuda.synchronize()
        px = pad_pixel(oracle, border, BGR24, PLANAR, True)
        want = T.expected(np.repeat(px.astype(np.float32), 64 * 64), 3, T.IMAGENET, dtype)
        assert np.array_equal(T.bits(got[0]), want), dtype


def test_refusals(vpp, frames):
    cs.tensor_refusals(PATH, vpp, frames)
