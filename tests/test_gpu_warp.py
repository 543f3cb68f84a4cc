"""GPU: tsvpp_convert_warp -- rotated and affine-warped boxes, each sampled BILINEAR through its own 2 x 3 matrix into one output size, one launch per 32.

The contract (include/tsvpp.h): the output is, bit for bit, what the oracle's conversion WITHOUT a resize returns for the virtual NV12 frame that the stated
coordinate and blend arithmetic samples (tests/warp_util.py: a numpy restatement, checked on the CPU in tests/test_warp_cpu.py).  Every comparison is
np.array_equal on the raw bits (uint8 bytes; fp32 viewed as bytes)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import warp_util as W
from letterbox_util import BGR24, BILINEAR, FLAVOURS, MERGED, PLANAR, RGB24, Y800, bits
from util import frame_k, knob_run, synth_nv12

pytestmark = pytest.mark.gpu

LIMIT = 32  # TSVPP_MAX_WARPS
# (width, height, pitch): landscape, portrait, a frame several tiles' footprints large, one smaller than a tile
GEO = [(128, 72, 192), (72, 128, 96), (322, 182, 384), (32, 18, 48)]
# 70 x 66: 4 k + 2 columns (the shifted tile column); 30 x 34: narrower than a tile (element-wise stores)
DSTS = [(64, 64), (70, 66), (30, 34), (112, 112)]
BORDERS = [None, (114, 128, 128), (3, 250, 7)]


def params(ts, dst, fcc, planes, norm, rt=BILINEAR):
    return ts.FrameParameters(width=dst[0], height=dst[1], resize_type=rt, pixel_format=fcc, planes_pos=planes, normalization=norm)


def f32(m):
    return tuple(float(np.float32(v)) for v in m)


def matrices(w, h, dw, dh):
    """the matrix set of one frame: name -> m"""
    import tensor_stream as ts
    out = {
        "rot30": ts.warp_rotated_box(w / 2, h / 2, 1.7 * dw, 1.7 * dh, math.radians(30), dw, dh),
        "transpose": (0, 1, 0, 1, 0, 0),
        "mirror": (-1, 0, w, 0, 1, 0),
        "up_shear": (0.37, 0.1, 0.3 * w, 0.05, 0.37, 0.3 * h),
        "down4.6": (4.6, 0, w / 2 - 2.3 * dw, 0, 4.6, h / 2 - 2.3 * dh),
        "left": ts.warp_rotated_box(0, h / 2, w, h, 0.2, dw, dh),
        "right": ts.warp_rotated_box(w, h / 2, w, h, -0.3, dw, dh),
        "top": ts.warp_rotated_box(w / 2, 0, w, h, 2.0, dw, dh),
        "bottom": ts.warp_rotated_box(w / 2, h, w, h, -1.1, dw, dh),
        "far": (1, 0, 5000, 0, 1, -3000),
        "singular": (0, 0, w / 3, 0, 0, h / 3),
    }
    return {k: f32(m) for k, m in out.items()}


@pytest.fixture(scope="module")
def frames():
    """the frames of GEO: [(y, uv)] on the host, the same on the device"""
    host = [synth_nv12(w, h, seed=1300 + k, pitch=p) for k, (w, h, p) in enumerate(GEO)]
    dev = [(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()) for y, uv in host]
    return host, dev


_virtual = {}


def virtual(host, k, geo, m, dst, border, key=None):
    """the virtual frame of (frame k, m, dst, border), computed once per module"""
    kk = (key if key is not None else k, geo[k][:2], m, dst, border)
    if kk not in _virtual:
        _virtual[kk] = W.virtual_frame(host[k][0], host[k][1], geo[k][0], geo[k][1], m, dst[0], dst[1], border)
    return _virtual[kk]


def check(v, oracle, host, dev, geo, warps, dst, fcc, planes, norm, border=None, out=None, only=None, what="", key=None):
    """one convert_warp call for `warps` = [(frame, m)], outputs (all, or the indices `only`) compared with the expected ones; returns the output tensor"""
    import tensor_stream as ts
    got = v.convert_warp([d[0] for d in dev], [d[1] for d in dev], [(k,) + m for k, m in warps], params(ts, dst, fcc, planes, norm), border=border, out=out,
                         width=[g[0] for g in geo], height=[g[1] for g in geo])
    torch.cuda.synchronize()
    for i in (range(len(warps)) if only is None else only):
        k, m = warps[i]
        ref = W.expected(oracle, None, None, 0, 0, m, dst, fcc, planes, norm, border, virtual=virtual(host, k, geo, m, dst, border, key=None if key is None else key(k)))
        g = bits(got[i])
        assert g.size == ref.size, (what, i, g.size, ref.size)
        bad = np.flatnonzero(g != ref)
        assert bad.size == 0, (f"{what} warp {i}: frame {k} {geo[k]} m={m} -> {dst} fcc={fcc} planes={planes} norm={norm} border={border}: {bad.size} bytes differ, "
                               f"first at {bad[:4]}")
    return got


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
    warps = [(k, m) for k, (w, h, _) in enumerate(GEO) for m in matrices(w, h, *dst).values()]
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
    """TSVPP_LDS_KB (read when a context is created): the default budget stages every tile, 0 gathers every tile, 3 KiB stages some tiles and gathers others in
    one launch -- the same bits, and the model's"""
    import tensor_stream as ts
    host, dev = frames
    w, h, pitch = GEO[2]
    dst = (112, 112)
    ms = matrices(w, h, *dst)
    warps = [(2, ms[k]) for k in ("rot30", "up_shear", "down4.6", "left", "far")]
    fp = params(ts, dst, BGR24, PLANAR, True)
    results = []
    for kb in (None, "0", "3"):
        if kb is not None:
            monkeypatch.setenv("TSVPP_LDS_KB", kb)
        v = ts.VideoProcessor(device=0, max_consumers=1)
        try:
            if not knob_run(("TSVPP_LDS_KB",)):
                d = ts.describe_warp(fp, [g for g in GEO], [(k,) + m for k, m in warps])
                if kb is None:
                    assert d["kernel"].endswith("staged,replicate>") and d["staged"] == len(warps) and d["lds"] > 3 * 1024
                elif kb == "0":
                    assert d["kernel"].endswith("gather,replicate>") and d["staged"] == 0 and d["lds"] == 0
                else:  # "far" and "up_shear" tap little: they stage; the 30 degree warp at scale 1.7 does not fit 3 KiB
                    assert d["kernel"].endswith("staged,replicate>") and 0 < d["staged"] < len(warps) and 0 < d["lds"] <= 3 * 1024
            got = check(v, oracle, host, dev, GEO, warps, dst, BGR24, PLANAR, True, what=f"LDS_KB={kb}")
            results.append(bits(got))
            check(v, oracle, host, dev, GEO, warps, dst, RGB24, MERGED, False, border=(114, 128, 128), what=f"LDS_KB={kb}")
        finally:
            v.Close()
    assert np.array_equal(results[0], results[1]) and np.array_equal(results[0], results[2]), "staged, gathering and mixed launches differ"


@pytest.mark.parametrize("n", [1, LIMIT, LIMIT + 1, 2 * LIMIT + 6])
def test_splitting_over_launches(vpp, oracle, frames, n):
    """one call, a frame of its own per output -- different sizes and pitches, distinct content (every byte + 37 k) --: the first and the last output of every
    launch are right"""
    host, dev = frames
    geo = [GEO[k % 3] for k in range(n)]
    h = [(frame_k(host[k % 3][0], k), frame_k(host[k % 3][1], k)) for k in range(n)]
    d = [(dev[k % 3][0] + (37 * k) % 256, dev[k % 3][1] + (37 * k) % 256) for k in range(n)]
    dst = (64, 64)
    names = ["rot30", "up_shear", "left", "bottom"]
    warps = [(k, matrices(geo[k][0], geo[k][1], *dst)[names[k % 4]]) for k in range(n)]
    only = sorted({0, n - 1} | {k for k in (LIMIT - 1, LIMIT, 2 * LIMIT - 1, 2 * LIMIT) if k < n})
    check(vpp, oracle, h, d, geo, warps, dst, BGR24, PLANAR, True, only=only, what=f"n={n}", key=lambda k: ("split", k))
    check(vpp, oracle, h, d, geo, warps, dst, RGB24, MERGED, False, border=(114, 128, 128), only=only, what=f"n={n}", key=lambda k: ("split", k))


GUARD = 256


@pytest.mark.parametrize("dst", [(64, 64), (70, 66), (30, 34)])
@pytest.mark.parametrize("fcc,planes,norm,off", [(BGR24, PLANAR, True, 0), (BGR24, PLANAR, True, 4), (RGB24, MERGED, True, 4), (RGB24, MERGED, False, 0),
                                                 (RGB24, MERGED, False, 1), (BGR24, PLANAR, False, 1), (Y800, MERGED, False, 1), (RGB24, MERGED, True, 0)])
def test_unaligned_outputs_and_guard_bytes(vpp, oracle, frames, fcc, planes, norm, off, dst):
    """outputs 0 / 1 / 4 bytes past a 16-byte boundary (vector-store and element-wise kernels); the bytes before and after every output stay as they were"""
    import tensor_stream as ts
    host, dev = frames
    warps = [(k, matrices(w, h, *dst)[name]) for k, (w, h, _) in enumerate(GEO) for name in ("rot30", "right")]
    n = len(warps)
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
    check(vpp, oracle, host, dev, GEO, warps, dst, fcc, planes, norm, border=(114, 128, 128), out=out, what=f"offset {off}")
    want = buf.clone()
    for s in starts:
        want[s:s + nbytes] = pat[s:s + nbytes]
    if not torch.equal(want, pat):
        bad = torch.nonzero(want != pat).flatten()[0].item()
        k = min(bad // stride, n - 1)
        raise AssertionError(f"guard byte damaged at {bad - starts[k]} relative to output {k} of {nbytes} bytes (offset {off}, dst {dst})")
    if not knob_run():
        d = ts.describe_warp(params(ts, dst, fcc, planes, norm), GEO, [(k,) + m for k, m in warps], border=(114, 128, 128), aligned_outputs=(off == 0))
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
    warps = [(k, matrices(w, h, *dst)[name]) for k, (w, h, _) in enumerate(GEO) for name in ("rot30", "top")]
    v = ts.VideoProcessor(device=0, max_consumers=1)
    try:
        v.set_option(V.OPT_COLOR_G_TERM, g_term)
        oracle.set_contract(CT_RESIZE | CT_INNER | ct_bits)
        try:
            check(v, oracle, host, dev, GEO, warps, dst, RGB24, PLANAR, False, border=(77, 201, 33))
            check(v, oracle, host, dev, GEO, warps, dst, BGR24, MERGED, True, border=(77, 201, 33))
        finally:
            oracle.set_contract(-1)
        v.set_option(V.OPT_COLOR_G_TERM, 0)
        check(v, oracle, host, dev, GEO, warps, dst, RGB24, PLANAR, False, border=(77, 201, 33))
    finally:
        oracle.set_contract(-1)
        v.Close()


def test_graph_capture_replays_bit_exact(vpp, oracle):
    """the records travel in the kernarg segment: the call allocates, copies and synchronises nothing, is legal during capture (one kernel node), and the graph
    replays the captured request on whatever the frames hold at replay time, onto re-poisoned outputs"""
    import tensor_stream as ts
    geo = [GEO[0], GEO[1], GEO[2]]
    dst = (64, 64)
    a = [synth_nv12(w, h, seed=1310 + k, pitch=p) for k, (w, h, p) in enumerate(geo)]
    dev = [(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()) for y, uv in a]
    warps = [(k, matrices(w, h, *dst)[name]) for k, (w, h, _) in enumerate(geo) for name in ("rot30", "left")]
    fp = params(ts, dst, RGB24, MERGED, False)
    out = vpp._alloc(fp.parameters, 64, 64, len(warps))
    kw = dict(width=[g[0] for g in geo], height=[g[1] for g in geo], out=out, border=(114, 128, 128))
    ys, uvs, ws = [d[0] for d in dev], [d[1] for d in dev], [(k,) + m for k, m in warps]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        vpp.convert_warp(ys, uvs, ws, fp, **kw)  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        vpp.convert_warp(ys, uvs, ws, fp, **kw)
    for seed in (1320, 1330):
        b = [synth_nv12(w, h, seed=seed + k, pitch=p) for k, (w, h, p) in enumerate(geo)]
        for k in range(len(geo)):
            dev[k][0].copy_(torch.from_numpy(b[k][0]).cuda())
            dev[k][1].copy_(torch.from_numpy(b[k][1]).cuda())
        out.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        for i, (k, m) in enumerate(warps):
            ref = W.expected(oracle, b[k][0], b[k][1], geo[k][0], geo[k][1], m, dst, RGB24, MERGED, False, (114, 128, 128))
            assert np.array_equal(bits(out[i]), ref), (seed, i)


def test_status_codes_with_a_live_context(vpp, frames):
    """the validation of tests/test_warp_cpu.py answers before any launch; a null plane or output is TSVPP_ERROR"""
    import tensor_stream as ts
    from tensor_stream import _native as N
    host, dev = frames
    y, uv = dev[0]
    w, h, pitch = GEO[0]
    fp = params(ts, (64, 64), RGB24, MERGED, False)
    one = dict(width=w, height=h)
    m = W.scale_only(w, h, 64, 64)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_warp(y, uv, [(1,) + m], fp, **one)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_warp(y, uv, [m], fp, border=(256, 128, 128), **one)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_warp(y, uv, [m], fp, border=(114, -1, 128), **one)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_warp(y, uv, [(float("nan"),) + m[1:]], fp, **one)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_warp(y, uv, [], fp, **one)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_warp(y, uv, [(2.0 ** 25,) + m[1:]], fp, **one)
    for rt in (0, 2, 3):  # NEAREST, BICUBIC, AREA: follow-ups
        with pytest.raises(RuntimeError, match="-2"):
            vpp.convert_warp(y, uv, [m], params(ts, (64, 64), RGB24, MERGED, False, rt=rt), **one)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_warp(y, uv, [m], params(ts, (64, 64), RGB24, MERGED, False), width=w - 1, height=h)
    fr = (N.NV12 * 1)(N.NV12(y.data_ptr(), None, pitch, pitch, w, h))
    ws = (N.Warp * 1)(N.Warp(0, (ctypes.c_float * 6)(*m)))
    out = torch.empty(64 * 64 * 3, dtype=torch.uint8, device="cuda")
    outs = (ctypes.c_void_p * 1)(out.data_ptr())
    L = N.lib()
    p = ctypes.byref(fp.parameters)
    assert L.tsvpp_convert_warp(vpp._ctx, 1, fr, 1, ws, p, -1, -1, -1, outs, None) == -3
    fr[0].uv = uv.data_ptr()
    outs[0] = None
    assert L.tsvpp_convert_warp(vpp._ctx, 1, fr, 1, ws, p, -1, -1, -1, outs, None) == -3
    assert L.tsvpp_convert_warp(vpp._ctx, 1, fr, 1, ws, p, -1, -1, -1, None, None) == -3
    outs[0] = out.data_ptr()
    assert L.tsvpp_convert_warp(None, 1, fr, 1, ws, p, -1, -1, -1, outs, None) == -3
    assert L.tsvpp_convert_warp(vpp._ctx, 1, fr, 1, ws, p, -1, -1, -1, outs, None) == 0
    torch.cuda.synchronize()
