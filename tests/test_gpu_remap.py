"""GPU: tsvpp_convert_remap -- every output samples one NV12 frame BILINEAR where a device-resident coordinate map says, one launch per 32 outputs, the tile's
footprint found by the kernel itself.

The contract (include/tsvpp.h): the output is, bit for bit, what the oracle's conversion WITHOUT a resize returns for the virtual NV12 frame that the stated
coordinate and blend arithmetic samples (tests/remap_util.py: a numpy restatement, checked on the CPU in tests/test_remap_cpu.py).  Every comparison is
np.array_equal on the raw bits (uint8 bytes; fp32 viewed as bytes).  The cases every coordinate path has are tests/coord_suite.py's, run on the descriptor
REMAP of tests/coord_paths.py."""
import numpy as np
import pytest
import torch

import coord_suite as cs
import remap_util as R
from coord_paths import REMAP as PATH, padded_to_device, remap_full_set as full_set, remap_tables
from coord_suite import BORDERS, DSTS, GEO, params, to_device
from letterbox_util import BGR24, FLAVOURS, MERGED, PLANAR, RGB24, Y800, bits

pytestmark = pytest.mark.gpu

LIMIT = PATH.LIMIT  # TSVPP_MAX_REMAPS
frames = cs.frames_fixture(1500)


def check(v, oracle, host, dev, geo, items, dst, fcc, planes, norm, border=None, **kw):
    """cs.check for `items` = remap_tables([(name, host map)], [(frame, map)], the device maps if the caller has them)"""
    return cs.check(PATH, v, oracle, host, dev, geo, items, dst, fcc, planes, norm, border, **kw)


@pytest.mark.parametrize("dst", DSTS)
def test_map_set_against_the_model(vpp, oracle, frames, dst):
    """every frame of GEO x {exact 2 : 1 where it fits, even translation, 30 degrees at scale 1.7, barrel distortion, transpose, constant, split, thousands of
    pixels outside, seeded garbage with NaN / inf / subnormals} in ONE call -- frames of different size and pitch, shared and distinct maps, two launches, tiles
    that stage and tiles that gather --, every flavour, replicate and two constant borders; then the barrel map pitch-padded with NaN in the padding"""
    host, dev = frames
    items = full_set(dst)
    assert len(items.remaps) > LIMIT and len(items.tables) < len(items.remaps)
    barrel = items.tables[-1][1]
    pad = padded_to_device(barrel)
    assert pad.stride(0) == 2 * dst[0] + 6 and tuple(pad.shape) == (dst[1], dst[0], 2)
    items.dev = [to_device(xy) for _, xy in items.tables[:-1]] + [pad]
    for border in BORDERS:
        for fcc, planes, norm in FLAVOURS:
            check(vpp, oracle, host, dev, GEO, items, dst, fcc, planes, norm, border, what="set")
    for fcc, planes, norm in ((BGR24, PLANAR, True), (RGB24, MERGED, False)):
        a = check(vpp, oracle, host, dev, GEO, remap_tables([("barrel@2", barrel)], [(2, 0)], [pad]), dst, fcc, planes, norm, (114, 128, 128), what="padded")
        b = check(vpp, oracle, host, dev, GEO, remap_tables([("barrel@2", barrel)], [(2, 0)]), dst, fcc, planes, norm, (114, 128, 128), what="tight")
        assert np.array_equal(bits(a), bits(b))


def test_identities_against_convert(vpp, oracle, frames):
    """the identity map with dst equal to the frame is Convert without a resize; the exact 2 : 1 map is Convert(BILINEAR) at that ratio; an even translation is
    Convert of the crop -- on the device, bit for bit, in every flavour"""
    import tensor_stream as ts
    host, dev = frames
    for k in (0, 1, 3):
        w, h, _ = GEO[k]
        y, uv = dev[k]
        exact = (w // 2) % 2 == 0 and (h // 2) % 2 == 0  # (32 x 18 has no even half)
        ident, half = to_device(R.identity(w, h)), to_device(R.exact_ratio(w // 2, h // 2, 2)) if exact else None
        dx, dy, cw, ch = 2 * (w // 8), 2 * (h // 8), (w // 2) & ~1, (h // 2) & ~1
        shift = to_device(R.translation(cw, ch, dx, dy))
        for fcc, planes, norm in FLAVOURS:
            for border in (None, (114, 128, 128)):
                a = vpp.convert_remap(y, uv, ident, params(ts, (w, h), fcc, planes, norm), border=border, width=w, height=h)
                b = vpp.convert_remap(y, uv, half, params(ts, (w // 2, h // 2), fcc, planes, norm), border=border, width=w, height=h) if exact else None
                c = vpp.convert_remap(y, uv, shift, params(ts, (cw, ch), fcc, planes, norm), border=border, width=w, height=h)
                torch.cuda.synchronize()
                one = vpp.Convert(y, uv, ts.FrameParameters(pixel_format=fcc, planes_pos=planes, normalization=norm), width=w, height=h)
                two = vpp.Convert(y, uv, params(ts, (w // 2, h // 2), fcc, planes, norm), width=w, height=h) if exact else None
                crop = vpp.Convert(y, uv, ts.FrameParameters(crop_coords=(dx, dy, dx + cw, dy + ch), pixel_format=fcc, planes_pos=planes, normalization=norm),
                                   width=w, height=h)
                torch.cuda.synchronize()
                assert np.array_equal(bits(a[0]), bits(one)), ("identity", k, fcc, planes, norm, border)
                assert not exact or np.array_equal(bits(b[0]), bits(two)), ("2:1", k, fcc, planes, norm, border)
                assert np.array_equal(bits(c[0]), bits(crop)), ("crop", k, fcc, planes, norm, border)


def test_transpose_in_closed_form(vpp, frames):
    """x = i, y = j: pixel centres map to pixel centres, every weight is zero -- no model needed"""
    import tensor_stream as ts
    host, dev = frames
    w, h, _ = GEO[0]
    y = host[0][0][:h, :w]
    got = vpp.convert_remap(dev[0][0], dev[0][1], to_device(R.transpose(h, w)), params(ts, (h, w), Y800, MERGED, False), border=(9, 9, 9), width=w, height=h)
    torch.cuda.synchronize()
    assert np.array_equal(got[0].cpu().numpy().reshape(w, h), y.T)


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


def test_graph_capture_replays_frames_and_maps(vpp, oracle):
    cs.graph_capture_replays(PATH, vpp, oracle, seed=1510)


def test_status_codes_with_a_live_context(vpp, frames):
    cs.status_codes_with_a_live_context(PATH, vpp, frames)
    # ... and the Python surface's short forms: one bare map with the default remaps, a bare (map, hint), two maps for one frame with the default remaps
    import tensor_stream as ts
    (y, uv), (w, h, _) = frames[1][0], GEO[0]
    xy, fp = to_device(R.translation(64, 64, 4, 2)), params(ts, (64, 64), RGB24, MERGED, False)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_remap(y, uv, xy, fp, border=(256, 128, 128), width=w, height=h)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_remap(y, uv, (xy, -5), fp, width=w, height=h)
    for bad in (xy.cpu(), [xy, xy]):
        with pytest.raises(ValueError):
            vpp.convert_remap(y, uv, bad, fp, width=w, height=h)
