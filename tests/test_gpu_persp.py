"""GPU: tsvpp_convert_perspective -- homography-warped outputs, each sampled BILINEAR through its own 3 x 3 map into one output size, one launch per 32.

The contract (include/tsvpp.h): the output is, bit for bit, what the oracle's conversion WITHOUT a resize returns for the virtual NV12 frame that the stated
coordinate -- three fused multiply-add pairs, one correctly rounded reciprocal, two products -- and the affine call's blend sample (tests/persp_util.py: a numpy
restatement, checked on the CPU in tests/test_persp_cpu.py).  Every comparison is np.array_equal on the raw bits (uint8 bytes; fp32 viewed as bytes).  The cases
every coordinate path has are tests/coord_suite.py's, run on the descriptor PERSP of tests/coord_paths.py; the frames and output sizes are the warp file's."""
import numpy as np
import pytest
import torch

import coord_suite as cs
import persp_util as P
import warp_util as W
from coord_paths import PERSP as PATH, homographies, persp_full_set as full_set, warp_full_set
from coord_suite import BORDERS, DSTS, GEO, params
from letterbox_util import BILINEAR, FLAVOURS, MERGED, RGB24, bits

pytestmark = pytest.mark.gpu

LIMIT = PATH.LIMIT  # TSVPP_MAX_PERSP
frames = cs.frames_fixture(1300)


def check(v, oracle, host, dev, geo, persps, dst, fcc, planes, norm, border=None, **kw):
    """cs.check for `persps` = [(frame, h)]"""
    return cs.check(PATH, v, oracle, host, dev, geo, persps, dst, fcc, planes, norm, border, **kw)


@pytest.mark.parametrize("dst", DSTS)
def test_homography_set_against_the_model(vpp, oracle, frames, dst):
    """every frame of GEO x {mild keystone, strong keystone, keystone with rotation, half outside on each side, far outside, 4 x the mild one, 3 x another,
    affine} in ONE call (44 outputs: two launches, frames of different size and pitch), every flavour, replicate and two constant borders"""
    host, dev = frames
    persps = full_set(dst)
    assert len(persps) == 44
    for border in BORDERS:
        for fcc, planes, norm in FLAVOURS:
            check(vpp, oracle, host, dev, GEO, persps, dst, fcc, planes, norm, border, what="set")


@pytest.mark.parametrize("dst", DSTS)
def test_affine_rows_are_convert_warp(vpp, frames, dst):
    """h = (m, 0, 0, 1): bit for bit tsvpp_convert_warp with m, for the whole matrix set of tests/test_gpu_warp.py, in every flavour under both border modes"""
    import tensor_stream as ts
    host, dev = frames
    ys, uvs = [d[0] for d in dev], [d[1] for d in dev]
    kw = dict(width=[g[0] for g in GEO], height=[g[1] for g in GEO])
    ms = warp_full_set(dst)
    for fcc, planes, norm in FLAVOURS:
        for border in (None, (114, 128, 128)):
            a = vpp.convert_warp(ys, uvs, [(k,) + m for k, m in ms], params(ts, dst, fcc, planes, norm), border=border, **kw)
            b = vpp.convert_perspective(ys, uvs, [(k,) + P.affine(m) for k, m in ms], params(ts, dst, fcc, planes, norm), border=border, **kw)
            torch.cuda.synchronize()
            assert np.array_equal(bits(a), bits(b)), (dst, fcc, planes, norm, border)


@pytest.mark.parametrize("dst", DSTS)
def test_scale_only_is_convert_bilinear_and_the_oracle(vpp, oracle, frames, dst):
    """h = (w / dst_w, 0, 0, 0, h / dst_h, 0, 0, 0, 1): the call is Convert(BILINEAR, dst) of the whole frame, bit for bit, in every flavour"""
    import tensor_stream as ts
    host, dev = frames
    persps = [(k, P.affine(W.scale_only(w, h, *dst))) for k, (w, h, _) in enumerate(GEO)]
    for fcc, planes, norm in FLAVOURS:
        refs = [oracle.convert(host[k][0], host[k][1], dst=dst, resize_type=BILINEAR, fourcc=fcc, planes=planes, normalization=norm, width=w)[0].ravel().view(np.uint8)
                for k, (w, h, _) in enumerate(GEO)]
        for border in (None, (114, 128, 128)):
            got = check(vpp, oracle, host, dev, GEO, persps, dst, fcc, planes, norm, border, what="scale-only")
            for k in range(len(GEO)):
                assert np.array_equal(bits(got[k]), refs[k]), (k, dst, fcc, planes, norm, border)
        for k, (w, h, _) in enumerate(GEO):
            one = vpp.Convert(dev[k][0], dev[k][1], params(ts, dst, fcc, planes, norm), width=w, height=h)
            torch.cuda.synchronize()
            assert np.array_equal(bits(one), refs[k]), (k, dst, fcc, planes, norm)


@pytest.mark.parametrize("dst", DSTS)
def test_4h_is_h(vpp, frames, dst):
    """every operation scales exactly by a power of two: the outputs of h and 4 h (and h / 8) are the same bits"""
    import tensor_stream as ts
    host, dev = frames
    ys, uvs = [d[0] for d in dev], [d[1] for d in dev]
    kw = dict(width=[g[0] for g in GEO], height=[g[1] for g in GEO], border=(3, 250, 7))
    base = [(k, h) for k, (w, hh, _) in enumerate(GEO) for name, h in homographies(w, hh, *dst).items() if name not in ("x4", "x3")]
    fp = params(ts, dst, RGB24, MERGED, False)
    a = vpp.convert_perspective(ys, uvs, [(k,) + h for k, h in base], fp, **kw)
    for s in (4.0, 0.125):
        b = vpp.convert_perspective(ys, uvs, [(k,) + tuple(s * v for v in h) for k, h in base], fp, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(bits(a), bits(b)), (dst, s)


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
    cs.graph_capture_replays(PATH, vpp, oracle, seed=1510)


def test_status_codes_with_a_live_context(vpp, frames):
    cs.status_codes_with_a_live_context(PATH, vpp, frames)
    # ... and the Python surface's short form, rows without a frame index
    import tensor_stream as ts
    (y, uv), (w, h, _) = frames[1][0], GEO[0]
    q, fp = P.affine(W.scale_only(w, h, 64, 64)), params(ts, (64, 64), RGB24, MERGED, False)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_perspective(y, uv, [q[:7] + (float("nan"),) + q[8:]], fp, width=w, height=h)
    with pytest.raises(RuntimeError, match="-2"):  # the horizon crosses the output
        vpp.convert_perspective(y, uv, [q[:6] + (-1 / 32, 0.0, 1.0)], fp, width=w, height=h)
