"""GPU: tsvpp_convert_mesh -- every output samples one NV12 frame BILINEAR where a device-resident control grid says; the coordinate of a pixel is interpolated
from the four control points of its cell.

The contract (include/tsvpp.h): the result is, bit for bit, tsvpp_convert_remap of the dense map E(mesh).  E(mesh) comes from tests/mesh_util.py (a numpy
restatement, checked on the CPU in tests/test_mesh_cpu.py), is uploaded for the dense call, and goes through tests/remap_util.py's model: the mesh call equals
both.  Every comparison is on the raw bits."""
import ctypes

import numpy as np
import pytest
import torch

import mesh_util as M
import remap_util as R
from letterbox_util import BGR24, FLAVOURS, MERGED, PLANAR, RGB24, Y800, bits
from test_gpu_remap import BORDERS, DSTS, GEO, frames, params, to_device, virtual  # noqa: F401  (frames: the module's fixture)
from util import frame_k, knob_run, synth_nv12

pytestmark = pytest.mark.gpu

LIMIT = 32  # TSVPP_MAX_MESHES
CELLS = [(4, 4), (16, 8), (256, 256)]
NAMES = ("barrel", "affine30", "far", "garbage")


def padded_to_device(mesh):
    """the mesh with a row stride of 2 * cols + 6 floats and NaN in the padding, as a strided device view"""
    view, back = M.padded(mesh)
    t = torch.from_numpy(back).cuda()
    assert torch.isnan(t[:, 2 * mesh.shape[1]:]).all()
    return t[:, :2 * mesh.shape[1]].unflatten(1, (mesh.shape[1], 2))


def full_set(dst, cell):
    """every frame of GEO through its own mesh set and through the next frame's, the frame-independent mesh shared, and the barrel mesh of frame 2 a second time,
    pitch-padded -- the last mesh: (meshes [(name, mesh)], remaps)"""
    meshes, index = [], {}
    for k, (w, h, _) in enumerate(GEO):
        for name, mesh in M.mesh_set(w, h, *dst, cell).items():
            key = name if name == "far" else f"{name}@{k}"
            if key not in index:
                index[key] = len(meshes)
                meshes.append((key, mesh))
    remaps = []
    for k in range(len(GEO)):
        for own in (k, (k + 1) % len(GEO)):
            remaps += [(k, index[n if n == "far" else f"{n}@{own}"]) for n in NAMES]
    remaps.append((2, len(meshes)))
    meshes.append(("barrel@2", M.mesh_set(GEO[2][0], GEO[2][1], *dst, cell)["barrel"]))
    return meshes, remaps


def check(v, oracle, host, dev, geo, meshes, remaps, dst, cell, fcc, planes, norm, border=None, out=None, only=None, what="", dev_meshes=None, dense=None, key=None,
          dense_call=True):
    """one convert_mesh call; meshes: [(name, host mesh)], remaps: [(frame, mesh)].  The outputs (all, or the indices `only`) equal the model's of E(mesh) and --
    dense_call -- the whole result equals convert_remap's on the uploaded E(mesh).  Returns the output tensor"""
    import tensor_stream as ts
    dm = [to_device(m) for _, m in meshes] if dev_meshes is None else dev_meshes
    exp = [M.expand(m, *dst, cell) for _, m in meshes] if dense is None else dense
    kw = dict(remaps=remaps, border=border, width=[g[0] for g in geo], height=[g[1] for g in geo])
    ys, uvs = [d[0] for d in dev], [d[1] for d in dev]
    got = v.convert_mesh(ys, uvs, dm, params(ts, dst, fcc, planes, norm), cell=cell, out=out, **kw)
    torch.cuda.synchronize()
    if dense_call:
        ref = v.convert_remap(ys, uvs, [to_device(e) for e in exp], params(ts, dst, fcc, planes, norm), **kw)
        torch.cuda.synchronize()
        for i in range(len(remaps)):
            assert np.array_equal(bits(got[i]), bits(ref[i])), (what, "differs from convert_remap of the expanded mesh", i, remaps[i], dst, cell, fcc, planes, norm, border)
    for i in (range(len(remaps)) if only is None else only):
        k, m = remaps[i]
        name = meshes[m][0]
        ref = R.expected(oracle, None, None, 0, 0, exp[m], fcc, planes, norm, border,
                         virtual=virtual(host, k, geo, ("mesh", name, cell, None if key is None else key(k)), exp[m], border))
        g = bits(got[i])
        bad = np.flatnonzero(g != ref) if g.size == ref.size else np.arange(1)
        assert bad.size == 0, (f"{what} output {i}: frame {k} {geo[k]} mesh {name} cell {cell} -> {dst} fcc={fcc} planes={planes} norm={norm} border={border}: "
                               f"{bad.size} bytes differ, first at {bad[:4]}")
    return got


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("dst", DSTS)
def test_mesh_set_is_the_dense_call_on_the_expanded_mesh(vpp, oracle, frames, dst, cell):
    """THE statement: frames of different size and pitch, shared and distinct meshes, more than 32 outputs (two launches), every flavour, replicate and two constant
    borders; barrel, 30 degrees at scale 1.7, far outside and seeded garbage; the last mesh pitch-padded with NaN in the padding.  70 x 66 runs the shifted tile
    column, whose thread tiles straddle two cells at cell width 4 and 16"""
    host, dev = frames
    meshes, remaps = full_set(dst, cell)
    assert len(remaps) > LIMIT and len(meshes) < len(remaps)
    pad = padded_to_device(meshes[-1][1])
    rows, cols = M.dims(*dst, cell)
    assert pad.stride(0) == 2 * cols + 6 and tuple(pad.shape) == (rows, cols, 2)
    dev_meshes = [to_device(m) for _, m in meshes[:-1]] + [pad]
    dense = [M.expand(m, *dst, cell) for _, m in meshes]
    for border in BORDERS:
        for fcc, planes, norm in FLAVOURS:
            check(vpp, oracle, host, dev, GEO, meshes, remaps, dst, cell, fcc, planes, norm, border, what="set", dev_meshes=dev_meshes, dense=dense)


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
    """TSVPP_LDS_KB (read when a context is created): the default budget, 0 (every tile gathers), 3 KiB (some tiles stage, the 30 degree warp and the barrel do not:
    the decisions are the dense call's on E(mesh), which tests/test_remap_cpu.py proves mixed for these warps) and the default budget with the hints of
    mesh_lds_hint -- the same bits four times, the model's and the dense call's"""
    import tensor_stream as ts
    host, dev = frames
    geo, dst, _ = R.STAGING_CASE
    assert geo == GEO[2]
    w, h, _ = geo
    cell = (16, 16)
    meshes = [("barrel@2", M.barrel(*dst, cell, w, h)), ("affine30@2", M.affine(*dst, cell, w, h)), ("translate@2", M.translation(*dst, cell, 104, 34)),
              ("far", M.far(*dst, cell))]
    remaps = [(2, m) for m in range(len(meshes))]
    dev_meshes = [to_device(m) for _, m in meshes]
    hints = [ts.mesh_lds_hint(m, dst, cell, w, h) for _, m in meshes]
    needs = [ts.remap_lds_hint(M.expand(m, *dst, cell), w, h) for _, m in meshes]
    assert hints == needs and min(needs) < 3 * 1024 - 64 < max(needs) < 40 * 1024 - 64  # 3 KiB: a mixed launch
    fp = params(ts, dst, BGR24, PLANAR, True)
    results = []
    for kb, hinted in ((None, False), ("0", False), ("3", False), (None, True)):
        if kb is not None:
            monkeypatch.setenv("TSVPP_LDS_KB", kb)
        else:
            monkeypatch.delenv("TSVPP_LDS_KB", raising=False)
        v = ts.VideoProcessor(device=0, max_consumers=1)
        try:
            dm = [(t, hint) for t, hint in zip(dev_meshes, hints)] if hinted else dev_meshes
            if not knob_run(("TSVPP_LDS_KB",)):
                d = ts.describe_mesh(fp, GEO, dm, cell=cell, remaps=remaps)
                if kb == "0":
                    assert d["kernel"] == "vpp_mesh<O_F32_PLANAR,vec,gather,replicate>" and d["lds"] == 0
                else:
                    assert d["kernel"] == "vpp_mesh<O_F32_PLANAR,vec,staged,replicate>"
                    assert d["lds"] == (max(hints) if hinted else (40 if kb is None else 3) * 1024 - 64)
            got = check(v, oracle, host, dev, GEO, meshes, remaps, dst, cell, BGR24, PLANAR, True, what=f"LDS_KB={kb} hints={hinted}", dev_meshes=dm)
            results.append(bits(got))
            check(v, oracle, host, dev, GEO, meshes, remaps, dst, cell, RGB24, MERGED, False, border=(114, 128, 128), what=f"LDS_KB={kb} hints={hinted}", dev_meshes=dm)
        finally:
            v.Close()
    for r in results[1:]:
        assert np.array_equal(results[0], r), "staged, gathering, mixed and hinted launches differ"


@pytest.mark.parametrize("n", [LIMIT, LIMIT + 1, 2 * LIMIT + 6])
def test_splitting_over_launches_with_a_mesh_per_output(vpp, oracle, frames, n):
    """the stabiliser's case: a frame and a mesh of its own per output; the first and the last output of every launch are right"""
    host, dev = frames
    geo = [GEO[k % 3] for k in range(n)]
    h = [(frame_k(host[k % 3][0], k), frame_k(host[k % 3][1], k)) for k in range(n)]
    d = [(dev[k % 3][0] + (37 * k) % 256, dev[k % 3][1] + (37 * k) % 256) for k in range(n)]
    dst, cell = (70, 66), (16, 16)
    meshes = [(f"shake{k}", M.affine(*dst, cell, geo[k][0], geo[k][1], degrees=3.0 * k - 40, scale=0.8 + 0.01 * k)) for k in range(n)]
    remaps = [(k, k) for k in range(n)]
    only = sorted({0, n - 1} | {k for k in (LIMIT - 1, LIMIT, 2 * LIMIT - 1, 2 * LIMIT) if k < n})
    dense = [M.expand(m, *dst, cell) if k in only else None for k, (_, m) in enumerate(meshes)]
    check(vpp, oracle, h, d, geo, meshes, remaps, dst, cell, BGR24, PLANAR, True, only=only, what=f"n={n}", dense=dense, key=lambda k: ("split", k), dense_call=False)
    check(vpp, oracle, h, d, geo, meshes, remaps, dst, cell, RGB24, MERGED, False, border=(114, 128, 128), only=only, what=f"n={n}", dense=dense,
          key=lambda k: ("split", k), dense_call=False)


GUARD = 256


@pytest.mark.parametrize("dst", [(64, 64), (70, 66), (30, 34)])
@pytest.mark.parametrize("fcc,planes,norm,off", [(BGR24, PLANAR, True, 0), (BGR24, PLANAR, True, 4), (RGB24, MERGED, True, 4), (RGB24, MERGED, False, 0),
                                                 (RGB24, MERGED, False, 1), (BGR24, PLANAR, False, 1), (Y800, MERGED, False, 1), (RGB24, MERGED, True, 0)])
def test_unaligned_outputs_and_guard_bytes(vpp, oracle, frames, fcc, planes, norm, off, dst):
    """outputs 0 / 1 / 4 bytes past a 16-byte boundary (vector-store and element-wise kernels); the bytes before and after every output stay as they were"""
    import tensor_stream as ts
    host, dev = frames
    cell = (16, 8)
    sets = [M.mesh_set(w, h, *dst, cell) for (w, h, _) in GEO]
    meshes = [(f"{nm}@{k}", sets[k][nm]) for k in range(len(GEO)) for nm in ("affine30", "garbage")]
    remaps = [(m // 2, m) for m in range(len(meshes))]
    n = len(remaps)
    nbytes = (1 if fcc == Y800 else 3) * dst[0] * dst[1] * (4 if norm else 1)
    stride = ((GUARD + off + nbytes + 15) // 16 * 16 + GUARD + 255) // 256 * 256
    total = n * stride + GUARD
    tile = (torch.arange(4096, device="cuda", dtype=torch.int32) * 131 + 17).remainder(251).to(torch.uint8)
    pat = tile.repeat((total + 4095) // 4096)[:total]
    buf = pat.clone()
    assert buf.data_ptr() % 16 == 0
    starts = [k * stride + GUARD + off for k in range(n)]
    slots = []
    for s in starts:
        buf[s:s + nbytes] = 0xA5
        slots.append(buf[s:s + nbytes])
        assert slots[-1].data_ptr() % 16 == off
    out = [s.view(torch.float32) if norm else s for s in slots]
    check(vpp, oracle, host, dev, GEO, meshes, remaps, dst, cell, fcc, planes, norm, border=(114, 128, 128), out=out, what=f"offset {off}", dense_call=False)
    want = buf.clone()
    for s in starts:
        want[s:s + nbytes] = pat[s:s + nbytes]
    if not torch.equal(want, pat):
        bad = torch.nonzero(want != pat).flatten()[0].item()
        k = min(bad // stride, n - 1)
        raise AssertionError(f"guard byte damaged at {bad - starts[k]} relative to output {k} of {nbytes} bytes (offset {off}, dst {dst})")
    if not knob_run():
        d = ts.describe_mesh(params(ts, dst, fcc, planes, norm), GEO, [(0, 0)] * len(meshes), cell=cell, remaps=remaps, border=(114, 128, 128), aligned_outputs=(off == 0))
        assert d["kernel"].split(",")[1] == ("vec" if off == 0 and dst[0] >= 32 else "elem")
        assert d["tail"] == (2 if (off == 0 and dst[0] == 70) else 0)


@pytest.mark.parametrize("g_term,ct_bits", [(0, None), (1, 0), (2, 2048)])
def test_colour_g_term_variants(oracle, frames, g_term, ct_bits):
    """TSVPP_OPT_COLOR_G_TERM 0 (the default), 1 and 2 against the oracle's matching contraction variant (bits as tests/test_gpu_parity.py sets them), border included"""
    import tensor_stream as ts
    from tensor_stream import vpp as V
    CT_RESIZE, CT_INNER = 1 | 2 | 8 | 16 | 64, 256
    host, dev = frames
    dst, cell = (64, 64), (16, 16)
    sets = [M.mesh_set(w, h, *dst, cell) for (w, h, _) in GEO]
    meshes = [(f"{nm}@{k}", sets[k][nm]) for k in range(len(GEO)) for nm in ("barrel", "affine30")]
    remaps = [(m // 2, m) for m in range(len(meshes))]
    v = ts.VideoProcessor(device=0, max_consumers=1)
    try:
        v.set_option(V.OPT_COLOR_G_TERM, g_term)
        if ct_bits is not None:
            oracle.set_contract(CT_RESIZE | CT_INNER | ct_bits)
        check(v, oracle, host, dev, GEO, meshes, remaps, dst, cell, RGB24, PLANAR, False, border=(77, 201, 33))
        check(v, oracle, host, dev, GEO, meshes, remaps, dst, cell, BGR24, MERGED, True, border=(77, 201, 33))
    finally:
        oracle.set_contract(-1)
        v.Close()


def test_graph_capture_replays_frames_and_meshes(vpp, oracle):
    """the records travel in the kernarg segment and hold the meshes' ADDRESSES: the call allocates, copies and synchronises nothing, is legal during capture, and
    the graph replays the captured request on whatever the frames AND the meshes hold at replay time, onto re-poisoned outputs"""
    import tensor_stream as ts
    geo = [GEO[0], GEO[1], GEO[2]]
    dst, cell = (70, 66), (16, 8)
    a = [synth_nv12(w, h, seed=1710 + k, pitch=p) for k, (w, h, p) in enumerate(geo)]
    dev = [(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()) for y, uv in a]
    kinds = [("affine30", "barrel"), ("barrel", "garbage"), ("far", "affine30")]  # the meshes before capture, then what each replay overwrites them with
    sets = [M.mesh_set(w, h, *dst, cell) for (w, h, _) in geo]
    dev_meshes = [to_device(sets[k][kinds[0][0]]) for k in range(3)] + [to_device(sets[k][kinds[0][1]]) for k in range(3)]
    remaps = [(k, k) for k in range(3)] + [(k, 3 + k) for k in range(3)]
    fp = params(ts, dst, RGB24, MERGED, False)
    out = vpp._alloc(fp.parameters, dst[0], dst[1], len(remaps))
    kw = dict(cell=cell, remaps=remaps, width=[g[0] for g in geo], height=[g[1] for g in geo], out=out, border=(114, 128, 128))
    ys, uvs = [d[0] for d in dev], [d[1] for d in dev]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        vpp.convert_mesh(ys, uvs, dev_meshes, fp, **kw)  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        vpp.convert_mesh(ys, uvs, dev_meshes, fp, **kw)
    for step, seed in enumerate((1720, 1730), start=1):
        b = [synth_nv12(w, h, seed=seed + k, pitch=p) for k, (w, h, p) in enumerate(geo)]
        for k in range(len(geo)):
            dev[k][0].copy_(torch.from_numpy(b[k][0]).cuda())
            dev[k][1].copy_(torch.from_numpy(b[k][1]).cuda())
        now = [sets[k][kinds[step][0]] for k in range(3)] + [sets[k][kinds[step][1]] for k in range(3)]
        for t, mesh in zip(dev_meshes, now):
            t.copy_(torch.from_numpy(mesh).cuda())
        out.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        for i, (k, m) in enumerate(remaps):
            ref = R.expected(oracle, b[k][0], b[k][1], geo[k][0], geo[k][1], M.expand(now[m], *dst, cell), RGB24, MERGED, False, (114, 128, 128))
            assert np.array_equal(bits(out[i]), ref), (seed, i)


def test_status_codes_with_a_live_context(vpp, frames):
    """the validation of tests/test_mesh_cpu.py answers before any launch; a null or misaligned mesh, a null plane or output and a null context are TSVPP_ERROR;
    the Python surface refuses a wrong dtype, device, shape or cell with ValueError before the C call"""
    import tensor_stream as ts
    from tensor_stream import _native as N
    host, dev = frames
    y, uv = dev[0]
    w, h, pitch = GEO[0]
    fp = params(ts, (64, 64), RGB24, MERGED, False)
    one = dict(width=w, height=h, cell=(16, 16))
    mesh = to_device(M.translation(64, 64, (16, 16), 4, 2))
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_mesh(y, uv, mesh, fp, remaps=[(1, 0)], **one)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_mesh(y, uv, mesh, fp, remaps=[(0, 1)], **one)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_mesh(y, uv, mesh, fp, border=(256, 128, 128), **one)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_mesh(y, uv, (mesh, -5), fp, **one)
    for rt in (0, 2, 3):  # NEAREST, BICUBIC, AREA: out of scope
        with pytest.raises(RuntimeError, match="-2"):
            vpp.convert_mesh(y, uv, mesh, params(ts, (64, 64), RGB24, MERGED, False, rt=rt), **one)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_mesh(y, uv, mesh, fp, width=w - 1, height=h, cell=(16, 16))
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_mesh(y, uv, torch.zeros((2, 2, 2), device="cuda"), fp, width=w, height=h, cell=(512, 512))
    for bad in (mesh.cpu(), mesh.double(), mesh[:, :4], torch.zeros((5, 2, 5), device="cuda").permute(0, 2, 1), [mesh, mesh]):
        with pytest.raises(ValueError):
            vpp.convert_mesh(y, uv, bad, fp, **one)
    with pytest.raises(ValueError):
        vpp.convert_mesh(y, uv, mesh, fp, width=w, height=h, cell=(16, 12))
    fr = (N.NV12 * 1)(N.NV12(y.data_ptr(), uv.data_ptr(), pitch, pitch, w, h))
    ms = (N.Mesh * 1)(N.Mesh(None, 0, 4, 4, 0))
    rs = (N.Remap * 1)(N.Remap(0, 0))
    out = torch.empty(64 * 64 * 3, dtype=torch.uint8, device="cuda")
    outs = (ctypes.c_void_p * 1)(out.data_ptr())
    L = N.lib()
    p = ctypes.byref(fp.parameters)
    assert L.tsvpp_convert_mesh(vpp._ctx, 1, fr, 1, ms, 1, rs, p, -1, -1, -1, outs, None) == -3       # a null mesh
    ms[0].xy = mesh.data_ptr() + 4
    assert L.tsvpp_convert_mesh(vpp._ctx, 1, fr, 1, ms, 1, rs, p, -1, -1, -1, outs, None) == -3       # ... one that is not 8-byte aligned
    ms[0].xy = mesh.data_ptr()
    ms[0].log2_cw = 9
    assert L.tsvpp_convert_mesh(vpp._ctx, 1, fr, 1, ms, 1, rs, p, -1, -1, -1, outs, None) == -2
    ms[0].log2_cw = 4
    fr[0].uv = None
    assert L.tsvpp_convert_mesh(vpp._ctx, 1, fr, 1, ms, 1, rs, p, -1, -1, -1, outs, None) == -3
    fr[0].uv = uv.data_ptr()
    outs[0] = None
    assert L.tsvpp_convert_mesh(vpp._ctx, 1, fr, 1, ms, 1, rs, p, -1, -1, -1, outs, None) == -3
    assert L.tsvpp_convert_mesh(vpp._ctx, 1, fr, 1, ms, 1, rs, p, -1, -1, -1, None, None) == -3
    outs[0] = out.data_ptr()
    assert L.tsvpp_convert_mesh(None, 1, fr, 1, ms, 1, rs, p, -1, -1, -1, outs, None) == -3
    assert L.tsvpp_convert_mesh(vpp._ctx, 1, fr, 1, ms, 1, rs, p, -1, -1, -1, outs, None) == 0
    torch.cuda.synchronize()
