"""GPU: tsvpp_convert_perspective -- homography-warped outputs, each sampled BILINEAR through its own 3 x 3 map into one output size, one launch per 32.

The contract (include/tsvpp.h): the output is, bit for bit, what the oracle's conversion WITHOUT a resize returns for the virtual NV12 frame that the stated
coordinate -- three fused multiply-add pairs, one correctly rounded reciprocal, two products -- and the affine call's blend sample (tests/persp_util.py: a numpy
restatement, checked on the CPU in tests/test_persp_cpu.py).  Every comparison is np.array_equal on the raw bits (uint8 bytes; fp32 viewed as bytes)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import persp_util as P
import warp_util as W
from letterbox_util import BGR24, BILINEAR, FLAVOURS, MERGED, PLANAR, RGB24, Y800, bits
from test_gpu_warp import BORDERS, DSTS, GEO, frames, matrices, params  # noqa: F401  (frames: that module's fixture -- the same frames and output sizes)
from util import frame_k, knob_run, synth_nv12

pytestmark = pytest.mark.gpu

LIMIT = 32  # TSVPP_MAX_PERSP


def f32(h):
    return tuple(float(np.float32(v)) for v in h)


def homographies(w, h, dw, dh):
    """the homography set of one frame: name -> h.  Every one is in the domain (asserted): the horizon stays off the output"""
    def quad(pts, dx=0.0, dy=0.0):
        return P.from_quad([(x * w + dx, y * h + dy) for x, y in pts], dw, dh)
    mild = [(0.1, 0.1), (0.9, 0.15), (0.85, 0.9), (0.12, 0.85)]
    strong = [(0.42, 0.2), (0.58, 0.2), (0.98, 0.9), (0.02, 0.9)]  # the far edge is 6 x shorter than the near one
    c, s = math.cos(math.radians(30)), math.sin(math.radians(30))
    keyrot = [(0.5 + (x - 0.5) * c - (y - 0.5) * s * h / w, 0.5 + (x - 0.5) * s * w / h + (y - 0.5) * c) for x, y in [(0.3, 0.25), (0.7, 0.25), (0.85, 0.75), (0.15, 0.75)]]
    out = {
        "mild": quad(mild),
        "strong": quad(strong),
        "keyrot": quad(keyrot),
        "left": quad(mild, dx=-0.5 * w),
        "right": quad(mild, dx=0.5 * w),
        "top": quad(strong, dy=-0.5 * h),
        "bottom": quad(strong, dy=0.5 * h),
        "far": quad(mild, dx=5000, dy=-3000),
        "x4": tuple(4.0 * v for v in quad(mild)),
        "x3": tuple(3.0 * v for v in quad(keyrot)),  # h8 = 3: a scaling that rounds
        "affine": P.affine(matrices(w, h, dw, dh)["rot30"]),
    }
    out = {k: f32(v) for k, v in out.items()}
    for k, v in out.items():
        assert P.in_domain(v, dw, dh), (k, v)
    return out


_virtual = {}


def virtual(host, k, geo, h, dst, border, key=None):
    """the virtual frame of (frame k, h, dst, border), computed once per module"""
    kk = (key if key is not None else k, geo[k][:2], h, dst, border)
    if kk not in _virtual:
        _virtual[kk] = P.virtual_frame(host[k][0], host[k][1], geo[k][0], geo[k][1], h, dst[0], dst[1], border)
    return _virtual[kk]


def check(v, oracle, host, dev, geo, persps, dst, fcc, planes, norm, border=None, out=None, only=None, what="", key=None):
    """one convert_perspective call for `persps` = [(frame, h)], outputs (all, or the indices `only`) compared with the expected ones; returns the output tensor"""
    import tensor_stream as ts
    got = v.convert_perspective([d[0] for d in dev], [d[1] for d in dev], [(k,) + h for k, h in persps], params(ts, dst, fcc, planes, norm), border=border, out=out,
                                width=[g[0] for g in geo], height=[g[1] for g in geo])
    torch.cuda.synchronize()
    for i in (range(len(persps)) if only is None else only):
        k, h = persps[i]
        ref = P.expected(oracle, None, None, 0, 0, h, dst, fcc, planes, norm, border, virtual=virtual(host, k, geo, h, dst, border, key=None if key is None else key(k)))
        g = bits(got[i])
        assert g.size == ref.size, (what, i, g.size, ref.size)
        bad = np.flatnonzero(g != ref)
        assert bad.size == 0, (f"{what} output {i}: frame {k} {geo[k]} h={h} -> {dst} fcc={fcc} planes={planes} norm={norm} border={border}: {bad.size} bytes differ, "
                               f"first at {bad[:4]}")
    return got


def full_set(dst):
    return [(k, h) for k, (w, hh, _) in enumerate(GEO) for h in homographies(w, hh, *dst).values()]


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
    ms = [(k, m) for k, (w, h, _) in enumerate(GEO) for m in matrices(w, h, *dst).values()]
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
    """TSVPP_LDS_KB (read when a context is created): the default budget stages, 0 gathers every tile, 3 KiB stages some tiles and gathers others in one launch
    -- the same bits, and the model's"""
    import tensor_stream as ts
    host, dev = frames
    w, h, pitch = GEO[2]
    dst = (112, 112)
    hs = homographies(w, h, *dst)
    persps = [(2, hs[k]) for k in ("mild", "strong", "keyrot", "left", "far", "affine")]
    fp = params(ts, dst, BGR24, PLANAR, True)
    results = []
    for kb in (None, "0", "3"):
        if kb is not None:
            monkeypatch.setenv("TSVPP_LDS_KB", kb)
        v = ts.VideoProcessor(device=0, max_consumers=1)
        try:
            if not knob_run(("TSVPP_LDS_KB",)):
                d = ts.describe_perspective(fp, [g for g in GEO], [(k,) + q for k, q in persps])
                if kb is None:
                    assert d["kernel"].endswith("staged,replicate>") and d["staged"] >= 4 and d["lds"] > 3 * 1024
                elif kb == "0":
                    assert d["kernel"].endswith("gather,replicate>") and d["staged"] == 0 and d["lds"] == 0
                else:  # "far" taps one pixel: it stages; the keystones do not fit 3 KiB
                    assert d["kernel"].endswith("staged,replicate>") and 0 < d["staged"] < len(persps) and 0 < d["lds"] <= 3 * 1024
            got = check(v, oracle, host, dev, GEO, persps, dst, BGR24, PLANAR, True, what=f"LDS_KB={kb}")
            results.append(bits(got))
            check(v, oracle, host, dev, GEO, persps, dst, RGB24, MERGED, False, border=(114, 128, 128), what=f"LDS_KB={kb}")
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
    names = ["mild", "strong", "left", "keyrot"]
    persps = [(k, homographies(geo[k][0], geo[k][1], *dst)[names[k % 4]]) for k in range(n)]
    only = sorted({0, n - 1} | {k for k in (LIMIT - 1, LIMIT, 2 * LIMIT - 1, 2 * LIMIT) if k < n})
    check(vpp, oracle, h, d, geo, persps, dst, BGR24, PLANAR, True, only=only, what=f"n={n}", key=lambda k: ("split", k))
    check(vpp, oracle, h, d, geo, persps, dst, RGB24, MERGED, False, border=(114, 128, 128), only=only, what=f"n={n}", key=lambda k: ("split", k))


GUARD = 256


@pytest.mark.parametrize("dst", [(64, 64), (70, 66), (30, 34)])
@pytest.mark.parametrize("fcc,planes,norm,off", [(BGR24, PLANAR, True, 0), (BGR24, PLANAR, True, 4), (RGB24, MERGED, True, 4), (RGB24, MERGED, False, 0),
                                                 (RGB24, MERGED, False, 1), (BGR24, PLANAR, False, 1), (Y800, MERGED, False, 1), (RGB24, MERGED, True, 0)])
def test_unaligned_outputs_and_guard_bytes(vpp, oracle, frames, fcc, planes, norm, off, dst):
    """outputs 0 / 1 / 4 bytes past a 16-byte boundary (vector-store and element-wise kernels); the bytes before and after every output stay as they were"""
    import tensor_stream as ts
    host, dev = frames
    persps = [(k, homographies(w, h, *dst)[name]) for k, (w, h, _) in enumerate(GEO) for name in ("keyrot", "right")]
    n = len(persps)
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
    check(vpp, oracle, host, dev, GEO, persps, dst, fcc, planes, norm, border=(114, 128, 128), out=out, what=f"offset {off}")
    want = buf.clone()
    for s in starts:
        want[s:s + nbytes] = pat[s:s + nbytes]
    if not torch.equal(want, pat):
        bad = torch.nonzero(want != pat).flatten()[0].item()
        k = min(bad // stride, n - 1)
        raise AssertionError(f"guard byte damaged at {bad - starts[k]} relative to output {k} of {nbytes} bytes (offset {off}, dst {dst})")
    if not knob_run():
        d = ts.describe_perspective(params(ts, dst, fcc, planes, norm), GEO, [(k,) + h for k, h in persps], border=(114, 128, 128), aligned_outputs=(off == 0))
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
    persps = [(k, homographies(w, h, *dst)[name]) for k, (w, h, _) in enumerate(GEO) for name in ("strong", "top")]
    v = ts.VideoProcessor(device=0, max_consumers=1)
    try:
        v.set_option(V.OPT_COLOR_G_TERM, g_term)
        oracle.set_contract(CT_RESIZE | CT_INNER | ct_bits)
        try:
            check(v, oracle, host, dev, GEO, persps, dst, RGB24, PLANAR, False, border=(77, 201, 33))
            check(v, oracle, host, dev, GEO, persps, dst, BGR24, MERGED, True, border=(77, 201, 33))
        finally:
            oracle.set_contract(-1)
        v.set_option(V.OPT_COLOR_G_TERM, 0)
        check(v, oracle, host, dev, GEO, persps, dst, RGB24, PLANAR, False, border=(77, 201, 33))
    finally:
        oracle.set_contract(-1)
        v.Close()


def test_graph_capture_replays_bit_exact(vpp, oracle):
    """the records travel in the kernarg segment: the call allocates, copies and synchronises nothing, is legal during capture (one kernel node), and the graph
    replays the captured request on whatever the frames hold at replay time, onto re-poisoned outputs"""
    import tensor_stream as ts
    geo = [GEO[0], GEO[1], GEO[2]]
    dst = (64, 64)
    a = [synth_nv12(w, h, seed=1510 + k, pitch=p) for k, (w, h, p) in enumerate(geo)]
    dev = [(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()) for y, uv in a]
    persps = [(k, homographies(w, h, *dst)[name]) for k, (w, h, _) in enumerate(geo) for name in ("strong", "left")]
    fp = params(ts, dst, RGB24, MERGED, False)
    out = vpp._alloc(fp.parameters, 64, 64, len(persps))
    kw = dict(width=[g[0] for g in geo], height=[g[1] for g in geo], out=out, border=(114, 128, 128))
    ys, uvs, qs = [d[0] for d in dev], [d[1] for d in dev], [(k,) + h for k, h in persps]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        vpp.convert_perspective(ys, uvs, qs, fp, **kw)  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        vpp.convert_perspective(ys, uvs, qs, fp, **kw)
    for seed in (1520, 1530):
        b = [synth_nv12(w, h, seed=seed + k, pitch=p) for k, (w, h, p) in enumerate(geo)]
        for k in range(len(geo)):
            dev[k][0].copy_(torch.from_numpy(b[k][0]).cuda())
            dev[k][1].copy_(torch.from_numpy(b[k][1]).cuda())
        out.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        for i, (k, h) in enumerate(persps):
            ref = P.expected(oracle, b[k][0], b[k][1], geo[k][0], geo[k][1], h, dst, RGB24, MERGED, False, (114, 128, 128))
            assert np.array_equal(bits(out[i]), ref), (seed, i)


def test_status_codes_with_a_live_context(vpp, frames):
    """the validation of tests/test_persp_cpu.py answers before any launch; a null plane or output is TSVPP_ERROR"""
    import tensor_stream as ts
    from tensor_stream import _native as N
    host, dev = frames
    y, uv = dev[0]
    w, h, pitch = GEO[0]
    fp = params(ts, (64, 64), RGB24, MERGED, False)
    one = dict(width=w, height=h)
    q = P.affine(W.scale_only(w, h, 64, 64))
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_perspective(y, uv, [(1,) + q], fp, **one)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_perspective(y, uv, [q], fp, border=(256, 128, 128), **one)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_perspective(y, uv, [q], fp, border=(114, -1, 128), **one)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_perspective(y, uv, [q[:7] + (float("nan"),) + q[8:]], fp, **one)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_perspective(y, uv, [], fp, **one)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_perspective(y, uv, [(2.0 ** 25,) + q[1:]], fp, **one)
    with pytest.raises(RuntimeError, match="-2"):  # the horizon crosses the output
        vpp.convert_perspective(y, uv, [q[:6] + (-1 / 32, 0.0, 1.0)], fp, **one)
    for rt in (0, 2, 3):  # NEAREST, BICUBIC, AREA: out of scope
        with pytest.raises(RuntimeError, match="-2"):
            vpp.convert_perspective(y, uv, [q], params(ts, (64, 64), RGB24, MERGED, False, rt=rt), **one)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_perspective(y, uv, [q], params(ts, (64, 64), RGB24, MERGED, False), width=w - 1, height=h)
    fr = (N.NV12 * 1)(N.NV12(y.data_ptr(), None, pitch, pitch, w, h))
    qs = (N.Persp * 1)(N.Persp(0, (ctypes.c_float * 9)(*q)))
    out = torch.empty(64 * 64 * 3, dtype=torch.uint8, device="cuda")
    outs = (ctypes.c_void_p * 1)(out.data_ptr())
    L = N.lib()
    p = ctypes.byref(fp.parameters)
    assert L.tsvpp_convert_perspective(vpp._ctx, 1, fr, 1, qs, p, -1, -1, -1, outs, None) == -3
    fr[0].uv = uv.data_ptr()
    outs[0] = None
    assert L.tsvpp_convert_perspective(vpp._ctx, 1, fr, 1, qs, p, -1, -1, -1, outs, None) == -3
    assert L.tsvpp_convert_perspective(vpp._ctx, 1, fr, 1, qs, p, -1, -1, -1, None, None) == -3
    outs[0] = out.data_ptr()
    assert L.tsvpp_convert_perspective(None, 1, fr, 1, qs, p, -1, -1, -1, outs, None) == -3
    assert L.tsvpp_convert_perspective(vpp._ctx, 1, fr, 1, qs, p, -1, -1, -1, outs, None) == 0
    torch.cuda.synchronize()
