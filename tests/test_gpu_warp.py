"""GPU: tsvpp_convert_warp -- rotated and affine-warped boxes, each sampled BILINEAR through its own 2 x 3 matrix into one output size, one launch per 32.

The contract (include/tsvpp.h): the output is, bit for bit, what the oracle's conversion WITHOUT a resize returns for the virtual NV12 frame that the stated
coordinate and blend arithmetic samples (tests/warp_util.py: a numpy restatement, checked on the CPU in tests/test_warp_cpu.py).  Every comparison is
np.array_equal on the raw bits (uint8 bytes; fp32 viewed as bytes).  The cases every coordinate path has are tests/coord_suite.py's, run on the descriptor
WARP of tests/coord_paths.py."""
import numpy as np
import pytest
import torch

import coord_suite as cs
import warp_util as W
from coord_paths import WARP as PATH, warp_full_set
from coord_suite import BORDERS, DSTS, GEO, params
from letterbox_util import BILINEAR, FLAVOURS, MERGED, RGB24, Y800, bits

pytestmark = pytest.mark.gpu

LIMIT = PATH.LIMIT  # TSVPP_MAX_WARPS
frames = cs.frames_fixture(1300)


def check(v, oracle, host, dev, geo, warps, dst, fcc, planes, norm, border=None, **kw):
    """cs.check for `warps` = [(frame, m)]"""
    return cs.check(PATH, v, oracle, host, dev, geo, warps, dst, fcc, planes, norm, border, **kw)


@pytest.mark.parametrize("dst", DSTS)
def test_scale_only_is_convert_bilinear_and_the_oracle(vpp, oracle, frames, dst):
    """m = (w / dst_w, 0, 0, 0, h / dst_h, 0): the call is Convert(BILINEAR, dst) of the whole frame, bit for bit, in every flavour under both border modes"""
    import tensor_stream as ts
    host, dev = frames
    warps = [(k, W.scale_only(w, h, *dst)) for k, (w, h, _) in enumerate(GEO)]
    for fcc, planes, norm in FLAVOURS:
        refs = [oracle.convert(host[k][0], host[k][1], dst=dst, resize_type=BILINEAR, fourcc=fcc, planes=planes, normalization=norm, width=w)[0].ravel().view(np.uint8)
                for k, (w, h, _) in enumerate(GEO)]
        for border in (None, (114, 128, 128)):
            got = check(vpp, oracle, host, dev, GEO, warps, dst, fcc, planes, norm, border, what="scale-only")
            for k, (w, h, _) in enumerate(GEO):
                assert np.array_equal(bits(got[k]), refs[k]), (k, dst, fcc, planes, norm, border)
        for k, (w, h, _) in enumerate(GEO):
            one = vpp.Convert(dev[k][0], dev[k][1], params(ts, dst, fcc, planes, norm), width=w, height=h)
            torch.cuda.synchronize()
            assert np.array_equal(bits(one), refs[k]) and np.array_equal(bits(got[k]), bits(one)), (k, dst, fcc, planes, norm)


@pytest.mark.parametrize("dst", DSTS)
def test_matrix_set_against_the_model(vpp, oracle, frames, dst):
    """every frame of GEO x {30 degrees at scale 1.7, transpose, mirror, up-scale with shear, down-scale by 4.6, half outside on each side, thousands of pixels
    outside, singular} in ONE call (44 outputs: two launches, frames of different size and pitch), every flavour, replicate and two constant borders"""
    host, dev = frames
    warps = warp_full_set(dst)
    assert len(warps) == 44
    for border in BORDERS:
        for fcc, planes, norm in FLAVOURS:
            check(vpp, oracle, host, dev, GEO, warps, dst, fcc, planes, norm, border, what="set")


def test_closed_forms_on_the_device(vpp, frames):
    """transpose and mirror need no model: pixel centres map to pixel centres"""
    import tensor_stream as ts
    host, dev = frames
    w, h, _ = GEO[0]
    y = host[0][0][:h, :w]
    got = vpp.convert_warp(dev[0][0], dev[0][1], [(0, 1, 0, 1, 0, 0)], params(ts, (h, w), Y800, MERGED, False), width=w, height=h)
    torch.cuda.synchronize()
    assert np.array_equal(got[0].cpu().numpy().reshape(w, h), y.T)
    got = vpp.convert_warp(dev[0][0], dev[0][1], [(-1, 0, w, 0, 1, 0)], params(ts, (w, h), Y800, MERGED, False), border=(9, 9, 9), width=w, height=h)
    torch.cuda.synchronize()
    assert np.array_equal(got[0].cpu().numpy().reshape(h, w), y[:, ::-1])


def test_staged_gather_and_mixed_launches(oracle, frames, monkeypatch):
    cs.staged_gather_and_mixed_launches(PATH, oracle, frames, monkeypatch)


@pytest.mark.parametrize("n", [1, LIMIT, LIMIT + 1, 2 * LIMIT + 6])
def test_splitting_over_launches(vpp, oracle, frames, n):
    cs.splitting_over_launches(PATH, vpp, oracle, frames, n)


@pytest.mark.parametrize("dst", cs.GUARD_DSTS)
@pytest.mark.parametrize("fcc,planes,norm,off", cs.GUARD_FLAVOURS)
def test_unaligned_outputs_and_guard_bytes(vpp, oracle, frames, fcc, planes, norm, off, dst):
    cs.unaligned_outputs_and_guard_bytes(PATH, vpp, oracle, frames, fcc, planes, norm, off, dst)


@pytest.mark.parametrize("g_term,ct_bits", [(1, 0), (2, 2048)])
def test_colour_g_term_variants(oracle, frames, g_term, ct_bits):
    cs.colour_g_term_variants(PATH, oracle, frames, g_term, ct_bits)


def test_graph_capture_replays_bit_exact(vpp, oracle):
    cs.graph_capture_replays(PATH, vpp, oracle, seed=1310)


def test_status_codes_with_a_live_context(vpp, frames):
    cs.status_codes_with_a_live_context(PATH, vpp, frames)
    # ... and the Python surface's short form, rows without a frame index
    import tensor_stream as ts
    (y, uv), (w, h, _) = frames[1][0], GEO[0]
    m, fp = W.scale_only(w, h, 64, 64), params(ts, (64, 64), RGB24, MERGED, False)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_warp(y, uv, [(float("nan"),) + m[1:]], fp, width=w, height=h)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_warp(y, uv, [m], fp, border=(256, 128, 128), width=w, height=h)
