"""GPU: tsvpp_convert_mesh -- every output samples one NV12 frame BILINEAR where a device-resident control grid says; the coordinate of a pixel is interpolated
from the four control points of its cell.

The contract (include/tsvpp.h): the result is, bit for bit, tsvpp_convert_remap of the dense map E(mesh).  E(mesh) comes from tests/mesh_util.py (a numpy
restatement, checked on the CPU in tests/test_mesh_cpu.py), is uploaded for the dense call, and goes through tests/remap_util.py's model: the mesh call equals
both.  Every comparison is on the raw bits.  The cases every coordinate path has are tests/coord_suite.py's, run on the descriptor MESH of
tests/coord_paths.py, whose call adaptor makes the dense call where a request says dense_call."""
import numpy as np
import pytest
import torch

import coord_suite as cs
import mesh_util as M
from coord_paths import MESH as PATH, mesh_full_set as full_set, mesh_pick, padded_to_device
from coord_suite import BORDERS, DSTS, GEO, params, to_device
from letterbox_util import BGR24, FLAVOURS, MERGED, PLANAR, RGB24, bits

pytestmark = pytest.mark.gpu

LIMIT = PATH.LIMIT  # TSVPP_MAX_MESHES
CELLS = [(4, 4), (16, 8), (256, 256)]
frames = cs.frames_fixture(1500)


def check(v, oracle, host, dev, geo, items, dst, fcc, planes, norm, border=None, **kw):
    """cs.check for `items` = mesh_tables([(name, host mesh)], [(frame, mesh)], cell, ...): the outputs equal the model's of E(mesh) and -- items.dense_call --
    the whole result equals convert_remap's on the uploaded E(mesh)"""
    return cs.check(PATH, v, oracle, host, dev, geo, items, dst, fcc, planes, norm, border, **kw)


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("dst", DSTS)
def test_mesh_set_is_the_dense_call_on_the_expanded_mesh(vpp, oracle, frames, dst, cell):
    """THE statement: frames of different size and pitch, shared and distinct meshes, more than 32 outputs (two launches), every flavour, replicate and two constant
    borders; barrel, 30 degrees at scale 1.7, far outside and seeded garbage; the last mesh pitch-padded with NaN in the padding.  70 x 66 runs the shifted tile
    column, whose thread tiles straddle two cells at cell width 4 and 16"""
    host, dev = frames
    items = full_set(dst, cell, dense_call=True)
    assert len(items.remaps) > LIMIT and len(items.tables) < len(items.remaps)
    pad = padded_to_device(items.tables[-1][1])
    rows, cols = M.dims(*dst, cell)
    assert pad.stride(0) == 2 * cols + 6 and tuple(pad.shape) == (rows, cols, 2)
    items.dev = [to_device(m) for _, m in items.tables[:-1]] + [pad]
    for border in BORDERS:
        for fcc, planes, norm in FLAVOURS:
            check(vpp, oracle, host, dev, GEO, items, dst, fcc, planes, norm, border, what="set")


@pytest.mark.parametrize("cell", [(4, 4), (16, 8), (8, 32)])
def test_identities_against_convert(vpp, frames, cell):
    """the identity mesh with dst equal to the frame is Convert without a resize; the mesh of x = 2 j + 0.5, y = 2 i + 0.5 is Convert(BILINEAR) at 2 : 1; an even
    translation is Convert of the crop -- on the device, bit for bit, in every flavour: the interpolation of such control points is exact"""
    import tensor_stream as ts
    host, dev = frames
    for k in (0, 1, 3):
        w, h, _ = GEO[k]
        y, uv = dev[k]
        exact = (w // 2) % 2 == 0 and (h // 2) % 2 == 0  # (32 x 18 has no even half)
        ident, half = to_device(M.identity(w, h, cell)), to_device(M.exact2(w // 2, h // 2, cell)) if exact else None
        dx, dy, cw, ch = 2 * (w // 8), 2 * (h // 8), (w // 2) & ~1, (h // 2) & ~1
        shift = to_device(M.translation(cw, ch, cell, dx, dy))
        for fcc, planes, norm in FLAVOURS:
            for border in (None, (114, 128, 128)):
                a = vpp.convert_mesh(y, uv, ident, params(ts, (w, h), fcc, planes, norm), cell=cell, border=border, width=w, height=h)
                b = vpp.convert_mesh(y, uv, half, params(ts, (w // 2, h // 2), fcc, planes, norm), cell=cell, border=border, width=w, height=h) if exact else None
                c = vpp.convert_mesh(y, uv, shift, params(ts, (cw, ch), fcc, planes, norm), cell=cell, border=border, width=w, height=h)
                torch.cuda.synchronize()
                one = vpp.Convert(y, uv, ts.FrameParameters(pixel_format=fcc, planes_pos=planes, normalization=norm), width=w, height=h)
                two = vpp.Convert(y, uv, params(ts, (w // 2, h // 2), fcc, planes, norm), width=w, height=h) if exact else None
                crop = vpp.Convert(y, uv, ts.FrameParameters(crop_coords=(dx, dy, dx + cw, dy + ch), pixel_format=fcc, planes_pos=planes, normalization=norm),
                                   width=w, height=h)
                torch.cuda.synchronize()
                assert np.array_equal(bits(a[0]), bits(one)), ("identity", k, fcc, planes, norm, border)
                assert not exact or np.array_equal(bits(b[0]), bits(two)), ("2:1", k, fcc, planes, norm, border)
                assert np.array_equal(bits(c[0]), bits(crop)), ("crop", k, fcc, planes, norm, border)


def test_staged_gather_and_mixed_launches(oracle, frames, monkeypatch):
    cs.staged_gather_and_mixed_launches(PATH, oracle, frames, monkeypatch)


@pytest.mark.parametrize("n", [LIMIT, LIMIT + 1, 2 * LIMIT + 6])
def test_splitting_over_launches_with_a_mesh_per_output(vpp, oracle, frames, n):
    cs.splitting_over_launches(PATH, vpp, oracle, frames, n)


@pytest.mark.parametrize("dst", cs.GUARD_DSTS)
@pytest.mark.parametrize("fcc,planes,norm,off", cs.GUARD_FLAVOURS)
def test_unaligned_outputs_and_guard_bytes(vpp, oracle, frames, fcc, planes, norm, off, dst):
    cs.unaligned_outputs_and_guard_bytes(PATH, vpp, oracle, frames, fcc, planes, norm, off, dst)


@pytest.mark.parametrize("g_term,ct_bits", [(0, None), (1, 0), (2, 2048)])
def test_colour_g_term_variants(oracle, frames, g_term, ct_bits):
    """TSVPP_OPT_COLOR_G_TERM 0 (the default), 1 and 2 against the oracle's matching contraction variant (bits as tests/test_gpu_parity.py sets them), border included.
    Written out here: the default is a variant of its own, so nothing is checked a second time after the option goes back"""
    import tensor_stream as ts
    from tensor_stream import vpp as V
    host, dev = frames
    dst = (64, 64)
    items = mesh_pick([(k, nm) for k in range(len(GEO)) for nm in ("barrel", "affine30")], GEO, dst, cell=(16, 16), dense_call=True)
    v = ts.VideoProcessor(device=0, max_consumers=1)
    try:
        v.set_option(V.OPT_COLOR_G_TERM, g_term)
        if ct_bits is not None:
            oracle.set_contract(cs.CT_RESIZE | cs.CT_INNER | ct_bits)
        check(v, oracle, host, dev, GEO, items, dst, RGB24, PLANAR, False, border=(77, 201, 33))
        check(v, oracle, host, dev, GEO, items, dst, BGR24, MERGED, True, border=(77, 201, 33))
    finally:
        oracle.set_contract(-1)
        v.Close()


def test_graph_capture_replays_frames_and_meshes(vpp, oracle):
    cs.graph_capture_replays(PATH, vpp, oracle, seed=1710)


def test_status_codes_with_a_live_context(vpp, frames):
    cs.status_codes_with_a_live_context(PATH, vpp, frames)
    # ... and the Python surface's short forms: one bare mesh with the default remaps, a bare (mesh, hint), two meshes for one frame with the default remaps
    import tensor_stream as ts
    (y, uv), (w, h, _) = frames[1][0], GEO[0]
    mesh, fp = to_device(M.translation(64, 64, (16, 16), 4, 2)), params(ts, (64, 64), RGB24, MERGED, False)
    one = dict(width=w, height=h, cell=(16, 16))
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_mesh(y, uv, mesh, fp, border=(256, 128, 128), **one)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_mesh(y, uv, (mesh, -5), fp, **one)
    for bad in (mesh.cpu(), [mesh, mesh]):
        with pytest.raises(ValueError):
            vpp.convert_mesh(y, uv, bad, fp, **one)
