"""GPU: tsvpp_convert_remap -- every output samples one NV12 frame BILINEAR where a device-resident coordinate map says, one launch per 32 outputs, the tile's
footprint found by the kernel itself.

The contract (include/tsvpp.h): the output is, bit for bit, what the oracle's conversion WITHOUT a resize returns for the virtual NV12 frame that the stated
coordinate and blend arithmetic samples (tests/remap_util.py: a numpy restatement, checked on the CPU in tests/test_remap_cpu.py).  Every comparison is
np.array_equal on the raw bits (uint8 bytes; fp32 viewed as bytes)."""
import ctypes

import numpy as np
import pytest
import torch

import remap_util as R
from letterbox_util import BGR24, BILINEAR, FLAVOURS, MERGED, PLANAR, RGB24, Y800, bits
from util import frame_k, knob_run, synth_nv12

pytestmark = pytest.mark.gpu

LIMIT = 32  # TSVPP_MAX_REMAPS
# (width, height, pitch): landscape, portrait, a frame several tiles' footprints large, one smaller than a tile
GEO = [(128, 72, 192), (72, 128, 96), (322, 182, 384), (32, 18, 48)]
# 70 x 66: 4 k + 2 columns (the shifted tile column); 30 x 34: narrower than a tile (element-wise stores)
DSTS = [(64, 64), (70, 66), (30, 34), (112, 112)]
BORDERS = [None, (114, 128, 128), (3, 250, 7)]
SHARED = ("transpose", "far")  # maps of the set that do not depend on the frame: one device map serves every frame


def params(ts, dst, fcc, planes, norm, rt=BILINEAR):
    return ts.FrameParameters(width=dst[0], height=dst[1], resize_type=rt, pixel_format=fcc, planes_pos=planes, normalization=norm)


def to_device(xy):
    return torch.from_numpy(np.ascontiguousarray(xy)).cuda()


def padded_to_device(xy):
    """the map with a row stride of 2 * dst_w + 6 floats and NaN in the padding, as a strided device view"""
    view, back = R.padded(xy)
    t = torch.from_numpy(back).cuda()
    assert torch.isnan(t[:, 2 * xy.shape[1]:]).all()
    return t[:, :2 * xy.shape[1]].unflatten(1, (xy.shape[1], 2))


@pytest.fixture(scope="module")
def frames():
    """the frames of GEO: [(y, uv)] on the host, the same on the device"""
    host = [synth_nv12(w, h, seed=1500 + k, pitch=p) for k, (w, h, p) in enumerate(GEO)]
    dev = [(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()) for y, uv in host]
    return host, dev


_virtual = {}


def virtual(host, k, geo, key, xy, border):
    """the virtual frame of (frame k, the map named `key`, border), computed once per module"""
    kk = (k, geo[k][:2], key, xy.shape, border)
    if kk not in _virtual:
        _virtual[kk] = R.virtual_frame_from_map(host[k][0], host[k][1], geo[k][0], geo[k][1], xy, border)
    return _virtual[kk]


def check(v, oracle, host, dev, geo, maps, remaps, dst, fcc, planes, norm, border=None, out=None, only=None, what="", dev_maps=None, key=None):
    """one convert_remap call; maps: [(name, host map)], remaps: [(frame, map)].  Outputs (all, or the indices `only`) are compared with the model's; returns the
    output tensor.  dev_maps: the device maps, if the caller has them (else the host maps are uploaded); key: frame index -> cache key of that frame's content"""
    import tensor_stream as ts
    dm = [to_device(xy) for _, xy in maps] if dev_maps is None else dev_maps
    got = v.convert_remap([d[0] for d in dev], [d[1] for d in dev], dm, params(ts, dst, fcc, planes, norm), remaps=remaps, border=border, out=out,
                          width=[g[0] for g in geo], height=[g[1] for g in geo])
    torch.cuda.synchronize()
    for i in (range(len(remaps)) if only is None else only):
        k, m = remaps[i]
        name, xy = maps[m]
        ref = R.expected(oracle, None, None, 0, 0, xy, fcc, planes, norm, border,
                         virtual=virtual(host, k, geo, (name, None if key is None else key(k)), xy, border))
        g = bits(got[i])
        assert g.size == ref.size, (what, i, g.size, ref.size)
        bad = np.flatnonzero(g != ref)
        assert bad.size == 0, (f"{what} output {i}: frame {k} {geo[k]} map {name} -> {dst} fcc={fcc} planes={planes} norm={norm} border={border}: {bad.size} bytes "
                               f"differ, first at {bad[:4]}")
    return got


def full_set(dst):
    """every frame of GEO through its map set in one call: (maps, remaps) with the frame-independent maps shared between the frames, and the barrel map of
    frame 2 a second time, pitch-padded -- the last map"""
    maps, remaps, shared = [], [], {}
    for k, (w, h, _) in enumerate(GEO):
        for name, xy in R.map_set(w, h, *dst).items():
            if name in SHARED:
                if name not in shared:
                    shared[name] = len(maps)
                    maps.append((name, xy))
                remaps.append((k, shared[name]))
            else:
                remaps.append((k, len(maps)))
                maps.append((f"{name}@{k}", xy))
    remaps.append((2, len(maps)))
    maps.append(("barrel@2", R.map_set(GEO[2][0], GEO[2][1], *dst)["barrel"]))
    return maps, remaps


@pytest.mark.parametrize("dst", DSTS)
def test_map_set_against_the_model(vpp, oracle, frames, dst):
    """every frame of GEO x {exact 2 : 1 where it fits, even translation, 30 degrees at scale 1.7, barrel distortion, transpose, constant, split, thousands of
    pixels outside, seeded garbage with NaN / inf / subnormals} in ONE call -- frames of different size and pitch, shared and distinct maps, two launches, tiles
    that stage and tiles that gather --, every flavour, replicate and two constant borders; then the barrel map pitch-padded with NaN in the padding"""
    host, dev = frames
    maps, remaps = full_set(dst)
    assert len(remaps) > LIMIT and len(maps) < len(remaps)
    barrel = maps[-1][1]
    pad = padded_to_device(barrel)
    assert pad.stride(0) == 2 * dst[0] + 6 and tuple(pad.shape) == (dst[1], dst[0], 2)
    dev_maps = [to_device(xy) for _, xy in maps[:-1]] + [pad]
    for border in BORDERS:
        for fcc, planes, norm in FLAVOURS:
            check(vpp, oracle, host, dev, GEO, maps, remaps, dst, fcc, planes, norm, border, what="set", dev_maps=dev_maps)
    for fcc, planes, norm in ((BGR24, PLANAR, True), (RGB24, MERGED, False)):
        a = check(vpp, oracle, host, dev, GEO, [("barrel@2", barrel)], [(2, 0)], dst, fcc, planes, norm, (114, 128, 128), what="padded", dev_maps=[pad])
        b = check(vpp, oracle, host, dev, GEO, [("barrel@2", barrel)], [(2, 0)], dst, fcc, planes, norm, (114, 128, 128), what="tight")
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
    """TSVPP_LDS_KB (read when a context is created): the default budget stages every tile of these maps, 0 gathers every tile, 3 KiB stages some tiles and gathers
    others in one launch (tests/test_remap_cpu.py proves all three from the footprints); and the default budget with the hints of remap_lds_hint -- the same
    bits four times, and the model's"""
    import tensor_stream as ts
    host, dev = frames
    geo, dst, names = R.STAGING_CASE
    assert geo == GEO[2]
    w, h, _ = geo
    ms = R.map_set(w, h, *dst)
    maps = [(f"{n}@2", ms[n]) for n in names]
    remaps = [(2, m) for m in range(len(maps))]
    dev_maps = [to_device(xy) for _, xy in maps]
    hints = [ts.remap_lds_hint(xy, w, h) for _, xy in maps]
    fp = params(ts, dst, BGR24, PLANAR, True)
    results = []
    for kb, hinted in ((None, False), ("0", False), ("3", False), (None, True)):
        if kb is not None:
            monkeypatch.setenv("TSVPP_LDS_KB", kb)
        else:
            monkeypatch.delenv("TSVPP_LDS_KB", raising=False)
        v = ts.VideoProcessor(device=0, max_consumers=1)
        try:
            dm = [(t, hint) for t, hint in zip(dev_maps, hints)] if hinted else dev_maps
            if not knob_run(("TSVPP_LDS_KB",)):
                d = ts.describe_remap(fp, GEO, dm, remaps=remaps)
                if hinted:
                    assert d["kernel"].endswith("staged,replicate>") and d["lds"] == max(hints) < 40 * 1024 - 64
                elif kb is None:
                    assert d["kernel"].endswith("staged,replicate>") and d["lds"] == 40 * 1024 - 64
                elif kb == "0":
                    assert d["kernel"].endswith("gather,replicate>") and d["lds"] == 0
                else:
                    assert d["kernel"].endswith("staged,replicate>") and d["lds"] == 3 * 1024 - 64
            got = check(v, oracle, host, dev, GEO, maps, remaps, dst, BGR24, PLANAR, True, what=f"LDS_KB={kb} hints={hinted}", dev_maps=dm)
            results.append(bits(got))
            check(v, oracle, host, dev, GEO, maps, remaps, dst, RGB24, MERGED, False, border=(114, 128, 128), what=f"LDS_KB={kb} hints={hinted}", dev_maps=dm)
        finally:
            v.Close()
    for r in results[1:]:
        assert np.array_equal(results[0], r), "staged, gathering, mixed and hinted launches differ"


@pytest.mark.parametrize("n", [1, LIMIT, LIMIT + 1, 2 * LIMIT + 6])
def test_splitting_over_launches(vpp, oracle, frames, n):
    """one call, a frame of its own per output -- different sizes and pitches, distinct content (every byte + 37 k) --: the first and the last output of every
    launch are right"""
    host, dev = frames
    geo = [GEO[k % 3] for k in range(n)]
    h = [(frame_k(host[k % 3][0], k), frame_k(host[k % 3][1], k)) for k in range(n)]
    d = [(dev[k % 3][0] + (37 * k) % 256, dev[k % 3][1] + (37 * k) % 256) for k in range(n)]
    dst = (64, 64)
    names = ["affine30", "barrel", "translate", "garbage"]
    sets = [R.map_set(w, hh, *dst) for (w, hh, _) in GEO[:3]]
    maps = [(f"{nm}@{g}", sets[g][nm]) for g in range(3) for nm in names]
    remaps = [(k, (k % 3) * len(names) + k % len(names)) for k in range(n)]
    only = sorted({0, n - 1} | {k for k in (LIMIT - 1, LIMIT, 2 * LIMIT - 1, 2 * LIMIT) if k < n})
    dev_maps = [to_device(xy) for _, xy in maps]
    check(vpp, oracle, h, d, geo, maps, remaps, dst, BGR24, PLANAR, True, only=only, what=f"n={n}", dev_maps=dev_maps, key=lambda k: ("split", k))
    check(vpp, oracle, h, d, geo, maps, remaps, dst, RGB24, MERGED, False, border=(114, 128, 128), only=only, what=f"n={n}", dev_maps=dev_maps, key=lambda k: ("split", k))


GUARD = 256


@pytest.mark.parametrize("dst", [(64, 64), (70, 66), (30, 34)])
@pytest.mark.parametrize("fcc,planes,norm,off", [(BGR24, PLANAR, True, 0), (BGR24, PLANAR, True, 4), (RGB24, MERGED, True, 4), (RGB24, MERGED, False, 0),
                                                 (RGB24, MERGED, False, 1), (BGR24, PLANAR, False, 1), (Y800, MERGED, False, 1), (RGB24, MERGED, True, 0)])
def test_unaligned_outputs_and_guard_bytes(vpp, oracle, frames, fcc, planes, norm, off, dst):
    """outputs 0 / 1 / 4 bytes past a 16-byte boundary (vector-store and element-wise kernels); the bytes before and after every output stay as they were"""
    import tensor_stream as ts
    host, dev = frames
    sets = [R.map_set(w, h, *dst) for (w, h, _) in GEO]
    maps = [(f"{nm}@{k}", sets[k][nm]) for k in range(len(GEO)) for nm in ("affine30", "garbage")]
    remaps = [(m // 2, m) for m in range(len(maps))]
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
    check(vpp, oracle, host, dev, GEO, maps, remaps, dst, fcc, planes, norm, border=(114, 128, 128), out=out, what=f"offset {off}")
    want = buf.clone()
    for s in starts:
        want[s:s + nbytes] = pat[s:s + nbytes]
    if not torch.equal(want, pat):
        bad = torch.nonzero(want != pat).flatten()[0].item()
        k = min(bad // stride, n - 1)
        raise AssertionError(f"guard byte damaged at {bad - starts[k]} relative to output {k} of {nbytes} bytes (offset {off}, dst {dst})")
    if not knob_run():
        d = ts.describe_remap(params(ts, dst, fcc, planes, norm), GEO, [(0, 0)] * len(maps), remaps=remaps, border=(114, 128, 128), aligned_outputs=(off == 0))
        assert d["kernel"].split(",")[1] == ("vec" if off == 0 and dst[0] >= 32 else "elem")
        assert d["tail"] == (2 if (off == 0 and dst[0] == 70) else 0)


@pytest.mark.parametrize("g_term,ct_bits", [(1, 0), (2, 2048)])
def test_colour_g_term_variants(oracle, frames, g_term, ct_bits):
    """TSVPP_OPT_COLOR_G_TERM against the oracle's matching contraction variant (bits as tests/test_gpu_parity.py sets them), border included, restored afterwards"""
    import tensor_stream as ts
    from tensor_stream import vpp as V
    CT_RESIZE, CT_INNER = 1 | 2 | 8 | 16 | 64, 256
    host, dev = frames
    dst = (64, 64)
    sets = [R.map_set(w, h, *dst) for (w, h, _) in GEO]
    maps = [(f"{nm}@{k}", sets[k][nm]) for k in range(len(GEO)) for nm in ("barrel", "split")]
    remaps = [(m // 2, m) for m in range(len(maps))]
    v = ts.VideoProcessor(device=0, max_consumers=1)
    try:
        v.set_option(V.OPT_COLOR_G_TERM, g_term)
        oracle.set_contract(CT_RESIZE | CT_INNER | ct_bits)
        try:
            check(v, oracle, host, dev, GEO, maps, remaps, dst, RGB24, PLANAR, False, border=(77, 201, 33))
            check(v, oracle, host, dev, GEO, maps, remaps, dst, BGR24, MERGED, True, border=(77, 201, 33))
        finally:
            oracle.set_contract(-1)
        v.set_option(V.OPT_COLOR_G_TERM, 0)
        check(v, oracle, host, dev, GEO, maps, remaps, dst, RGB24, PLANAR, False, border=(77, 201, 33))
    finally:
        oracle.set_contract(-1)
        v.Close()


def test_graph_capture_replays_frames_and_maps(vpp, oracle):
    """the records travel in the kernarg segment and hold the maps' ADDRESSES: the call allocates, copies and synchronises nothing, is legal during capture, and
    the graph replays the captured request on whatever the frames AND the maps hold at replay time, onto re-poisoned outputs"""
    import tensor_stream as ts
    geo = [GEO[0], GEO[1], GEO[2]]
    dst = (64, 64)
    a = [synth_nv12(w, h, seed=1510 + k, pitch=p) for k, (w, h, p) in enumerate(geo)]
    dev = [(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()) for y, uv in a]
    kinds = [("affine30", "barrel"), ("barrel", "garbage"), ("translate", "affine30")]  # the maps before capture, then what each replay overwrites them with
    sets = [R.map_set(w, h, *dst) for (w, h, _) in geo]
    dev_maps = [to_device(sets[k][kinds[0][0]]) for k in range(3)] + [to_device(sets[k][kinds[0][1]]) for k in range(3)]
    remaps = [(k, k) for k in range(3)] + [(k, 3 + k) for k in range(3)]
    fp = params(ts, dst, RGB24, MERGED, False)
    out = vpp._alloc(fp.parameters, 64, 64, len(remaps))
    kw = dict(remaps=remaps, width=[g[0] for g in geo], height=[g[1] for g in geo], out=out, border=(114, 128, 128))
    ys, uvs = [d[0] for d in dev], [d[1] for d in dev]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        vpp.convert_remap(ys, uvs, dev_maps, fp, **kw)  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        vpp.convert_remap(ys, uvs, dev_maps, fp, **kw)
    for step, seed in enumerate((1520, 1530), start=1):
        b = [synth_nv12(w, h, seed=seed + k, pitch=p) for k, (w, h, p) in enumerate(geo)]
        for k in range(len(geo)):
            dev[k][0].copy_(torch.from_numpy(b[k][0]).cuda())
            dev[k][1].copy_(torch.from_numpy(b[k][1]).cuda())
        now = [sets[k][kinds[step][0]] for k in range(3)] + [sets[k][kinds[step][1]] for k in range(3)]
        for t, xy in zip(dev_maps, now):
            t.copy_(torch.from_numpy(xy).cuda())
        out.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        for i, (k, m) in enumerate(remaps):
            ref = R.expected(oracle, b[k][0], b[k][1], geo[k][0], geo[k][1], now[m], RGB24, MERGED, False, (114, 128, 128))
            assert np.array_equal(bits(out[i]), ref), (seed, i)


def test_status_codes_with_a_live_context(vpp, frames):
    """the validation of tests/test_remap_cpu.py answers before any launch; a null or misaligned map, a null plane or output and a null context are TSVPP_ERROR;
    the Python surface refuses a wrong dtype, device or shape with ValueError before the C call"""
    import tensor_stream as ts
    from tensor_stream import _native as N
    host, dev = frames
    y, uv = dev[0]
    w, h, pitch = GEO[0]
    fp = params(ts, (64, 64), RGB24, MERGED, False)
    one = dict(width=w, height=h)
    xy = to_device(R.translation(64, 64, 4, 2))
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_remap(y, uv, xy, fp, remaps=[(1, 0)], **one)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_remap(y, uv, xy, fp, remaps=[(0, 1)], **one)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_remap(y, uv, xy, fp, border=(256, 128, 128), **one)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_remap(y, uv, (xy, -5), fp, **one)
    for rt in (0, 2, 3):  # NEAREST, BICUBIC, AREA: follow-ups
        with pytest.raises(RuntimeError, match="-2"):
            vpp.convert_remap(y, uv, xy, params(ts, (64, 64), RGB24, MERGED, False, rt=rt), **one)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_remap(y, uv, xy, fp, width=w - 1, height=h)
    for bad in (xy.cpu(), xy.double(), xy[:, :62], xy.permute(1, 0, 2), [xy, xy]):
        with pytest.raises(ValueError):
            vpp.convert_remap(y, uv, bad, fp, **one)
    fr = (N.NV12 * 1)(N.NV12(y.data_ptr(), uv.data_ptr(), pitch, pitch, w, h))
    ms = (N.Map * 1)(N.Map(None, 0, 0))
    rs = (N.Remap * 1)(N.Remap(0, 0))
    out = torch.empty(64 * 64 * 3, dtype=torch.uint8, device="cuda")
    outs = (ctypes.c_void_p * 1)(out.data_ptr())
    L = N.lib()
    p = ctypes.byref(fp.parameters)
    assert L.tsvpp_convert_remap(vpp._ctx, 1, fr, 1, ms, 1, rs, p, -1, -1, -1, outs, None) == -3       # a null map
    ms[0].xy = xy.data_ptr() + 4
    assert L.tsvpp_convert_remap(vpp._ctx, 1, fr, 1, ms, 1, rs, p, -1, -1, -1, outs, None) == -3       # ... one that is not 8-byte aligned
    ms[0].xy = xy.data_ptr()
    fr[0].uv = None
    assert L.tsvpp_convert_remap(vpp._ctx, 1, fr, 1, ms, 1, rs, p, -1, -1, -1, outs, None) == -3
    fr[0].uv = uv.data_ptr()
    outs[0] = None
    assert L.tsvpp_convert_remap(vpp._ctx, 1, fr, 1, ms, 1, rs, p, -1, -1, -1, outs, None) == -3
    assert L.tsvpp_convert_remap(vpp._ctx, 1, fr, 1, ms, 1, rs, p, -1, -1, -1, None, None) == -3
    outs[0] = out.data_ptr()
    assert L.tsvpp_convert_remap(None, 1, fr, 1, ms, 1, rs, p, -1, -1, -1, outs, None) == -3
    assert L.tsvpp_convert_remap(vpp._ctx, 1, fr, 1, ms, 1, rs, p, -1, -1, -1, outs, None) == 0
    torch.cuda.synchronize()
