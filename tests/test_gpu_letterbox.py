"""GPU: tsvpp_convert_letterbox -- n NV12 frames, each resized with its aspect kept into an inner rectangle of one canvas size, the rest pad, one launch per 32.

The contract (include/tsvpp.h): the inner rectangle holds, bit for bit, what the oracle returns for the frame resized to the rectangle's size; every other pixel
holds what the oracle's conversion without a resize returns for a frame of the constant pad sample.  Every comparison is np.array_equal on the raw bits (uint8
bytes; fp32 viewed as bytes) against a canvas built from the existing oracle only (tests/letterbox_util.py)."""
import ctypes

import numpy as np
import pytest
import torch

from guard_util import arena
from letterbox_util import BGR24, BICUBIC, BILINEAR, CANVASES, FLAVOURS, GEO, MERGED, NEAREST, PLANAR, RGB24, Y800, AREA, bits, default_rect, expected_canvas
from util import frame_k, knob_run, synth_nv12

pytestmark = pytest.mark.gpu

LIMIT = 32  # TSVPP_MAX_LETTERBOX
GRAY = (114, 128, 128)


def params(ts, canvas, rt, fcc, planes, norm):
    return ts.FrameParameters(width=canvas[0], height=canvas[1], resize_type=rt, pixel_format=fcc, planes_pos=planes, normalization=norm)


@pytest.fixture(scope="module")
def frames():
    """the frames of GEO: [(y, uv)] on the host, the same on the device"""
    host = [synth_nv12(w, h, seed=700 + k, pitch=p) for k, (w, h, p) in enumerate(GEO)]
    dev = [(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()) for y, uv in host]
    return host, dev


def check(v, oracle, host, dev, geo, canvas, rt, fcc, planes, norm, pad=GRAY, rects=None, out=None, only=None, what=""):
    """letterbox the frames in one call, compare canvases (all, or the indices `only`) with the expected ones; returns (out, rects)"""
    import tensor_stream as ts
    fp = params(ts, canvas, rt, fcc, planes, norm)
    got, used = v.convert_letterbox([d[0] for d in dev], [d[1] for d in dev], fp, pad=pad, rects=rects, out=out, width=[g[0] for g in geo], height=[g[1] for g in geo])
    torch.cuda.synchronize()
    assert len(used) == len(geo)
    for k in (range(len(geo)) if only is None else only):
        w, h = geo[k][0], geo[k][1]
        want_rect = tuple(rects[k]) if rects is not None else default_rect(w, h, *canvas)
        assert tuple(used[k]) == want_rect, (what, k, used[k], want_rect)
        ref = expected_canvas(oracle, host[k][0], host[k][1], w, h, want_rect, canvas, rt, fcc, planes, norm, pad)
        g = bits(got[k])
        assert g.size == ref.size, (what, k, g.size, ref.size)
        bad = np.flatnonzero(g != ref)
        assert bad.size == 0, (f"{what} frame {k} {geo[k]} -> canvas {canvas} rect {want_rect} rt={rt} fcc={fcc} planes={planes} norm={norm} pad={pad}: "
                               f"{bad.size} bytes differ, first at {bad[:4]}")
    return got, used


@pytest.mark.parametrize("canvas", CANVASES)
@pytest.mark.parametrize("rt", [NEAREST, BILINEAR, BICUBIC])
def test_geometry_against_the_oracle(vpp, oracle, frames, rt, canvas):
    """every frame of GEO into every canvas, every flavour: pad above / below and left / right, no pad, up-scale, the shifted tile column, element-wise stores"""
    host, dev = frames
    assert default_rect(72, 128, 64, 64) == (14, 0, 36, 64) and default_rect(64, 64, 64, 64) == (0, 0, 64, 64)
    for fcc, planes, norm in FLAVOURS:
        check(vpp, oracle, host, dev, GEO, canvas, rt, fcc, planes, norm)
    if rt == BILINEAR:  # a pad that runs into the colour back end's clamps
        for fcc, planes, norm in FLAVOURS:
            check(vpp, oracle, host, dev, GEO, canvas, rt, fcc, planes, norm, pad=(3, 250, 7))


@pytest.mark.parametrize("rt", [NEAREST, BILINEAR, BICUBIC])
def test_rectangles_of_the_caller(vpp, oracle, frames, rt):
    """a small rectangle off every tile boundary, one that fills the canvas (no pad at all, aspect not kept), one in the last rows and columns"""
    host, dev = frames
    rects = [(6, 2, 20, 10), (0, 0, 64, 64), (34, 50, 30, 14), (2, 2, 60, 60), (62, 0, 2, 64)]
    for fcc, planes, norm in [(RGB24, MERGED, False), (BGR24, PLANAR, True), (RGB24, MERGED, True), (Y800, MERGED, False)]:
        check(vpp, oracle, host, dev, GEO, (64, 64), rt, fcc, planes, norm, rects=rects)
    check(vpp, oracle, host[:2], dev[:2], GEO[:2], (70, 66), rt, BGR24, PLANAR, False, rects=[(40, 2, 30, 64), (0, 0, 70, 66)])


@pytest.mark.parametrize("n", [1, LIMIT, LIMIT + 1, 2 * LIMIT + 6])
def test_mixed_batch_and_splitting_over_launches(vpp, oracle, frames, n):
    """one call, frames of different size and pitch, distinct content per frame (every byte + 37 k): the first and the last canvas of every launch are right"""
    host, dev = frames
    geo = [GEO[k % 3] for k in range(n)]
    h = [(frame_k(host[k % 3][0], k), frame_k(host[k % 3][1], k)) for k in range(n)]
    d = [(dev[k % 3][0] + (37 * k) % 256, dev[k % 3][1] + (37 * k) % 256) for k in range(n)]
    only = sorted({0, n - 1} | {k for k in (LIMIT - 1, LIMIT, 2 * LIMIT - 1, 2 * LIMIT) if k < n})
    check(vpp, oracle, h, d, geo, (64, 64), BILINEAR, BGR24, PLANAR, True, only=only, what=f"n={n}")
    check(vpp, oracle, h, d, geo, (70, 66), BICUBIC, RGB24, MERGED, False, only=only, what=f"n={n}")


@pytest.mark.parametrize("canvas", [(64, 64), (70, 66), (30, 34)])
@pytest.mark.parametrize("rt,fcc,planes,norm,off", [(BILINEAR, BGR24, PLANAR, True, 0), (BILINEAR, BGR24, PLANAR, True, 4), (BICUBIC, RGB24, MERGED, True, 4),
                                                    (BICUBIC, RGB24, MERGED, False, 0), (BICUBIC, RGB24, MERGED, False, 1), (NEAREST, BGR24, PLANAR, False, 1),
                                                    (NEAREST, BGR24, PLANAR, False, 4), (BILINEAR, Y800, MERGED, False, 1), (BILINEAR, RGB24, MERGED, True, 0)])
def test_unaligned_outputs_and_guard_bytes(vpp, oracle, frames, rt, fcc, planes, norm, off, canvas):
    """canvases 0 / 1 / 4 bytes past a 16-byte boundary (vector-store and element-wise kernels); the bytes before and after every canvas stay as they were"""
    import tensor_stream as ts
    host, dev = frames
    n = len(GEO)
    nbytes = (1 if fcc == Y800 else 3) * canvas[0] * canvas[1] * (4 if norm else 1)
    _, slots, verify = arena([nbytes] * n, off, what="canvas", where=f"canvas {canvas}")
    out = [s.view(torch.float32) if norm else s for s in slots]
    check(vpp, oracle, host, dev, GEO, canvas, rt, fcc, planes, norm, out=out, what=f"offset {off}")
    verify()
    if not knob_run():
        d = ts.describe_letterbox(params(ts, canvas, rt, fcc, planes, norm), GEO, aligned_outputs=(off == 0))
        # element-wise stores: canvases off the 16-byte alignment, and widths 4 k + 2 narrower than a tile (no tile column to shift)
        assert d["kernel"].split(",")[2] == ("vec" if off == 0 and canvas[0] >= 32 else "elem")
        assert d["tail"] == (2 if (off == 0 and canvas[0] == 70) else 0)


@pytest.mark.parametrize("rt", [BILINEAR, BICUBIC])
def test_staged_and_gather_paths(oracle, monkeypatch, rt):
    """the one larger case, 1920 x 1080 -> 640 x 640: with no LDS budget (TSVPP_LDS_KB=0, read when a context is created) every tile gathers from global memory --
    the same bits as the staged launch, and the oracle's"""
    import tensor_stream as ts
    W, H, PITCH = 1920, 1080, 2048
    y, uv = synth_nv12(W, H, seed=2025, pitch=PITCH)
    dev = [(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda())]
    results = []
    for kb in (None, "0"):
        if kb is not None:
            monkeypatch.setenv("TSVPP_LDS_KB", kb)
        v = ts.VideoProcessor(device=0, max_consumers=1)
        try:
            if not knob_run(("TSVPP_LDS_KB",)):
                d = ts.describe_letterbox(params(ts, (640, 640), rt, BGR24, PLANAR, True), (W, H, PITCH))
                if kb is None:
                    assert d["kernel"].endswith("staged>") and d["staged"] == 1 and d["lds"] > 0
                else:
                    assert d["kernel"].endswith("gather>") and d["staged"] == 0
            fp = params(ts, (640, 640), rt, BGR24, PLANAR, True)
            got, used = v.convert_letterbox([dev[0][0]], [dev[0][1]], fp, width=W, height=H)
            torch.cuda.synchronize()
            assert used == [(0, 140, 640, 360)]
            results.append(bits(got[0]))
        finally:
            v.Close()
    assert np.array_equal(results[0], results[1]), "staged and gathering launches differ"
    inner, _, _ = oracle.convert(y[:, :W], uv[:, :W], dst=(640, 360), resize_type=rt, fourcc=BGR24, planes=PLANAR, normalization=True, nthreads=8)
    ref = expected_canvas(oracle, y, uv, W, H, (0, 140, 640, 360), (640, 640), rt, BGR24, PLANAR, True, GRAY, inner=inner)
    assert np.array_equal(results[0], ref)


@pytest.mark.parametrize("rt", [NEAREST, BILINEAR, BICUBIC])
def test_the_inner_block_is_what_convert_returns(vpp, frames, rt):
    """the two paths of the library agree: the rectangle holds tsvpp_convert's output for dst = the rectangle's size"""
    import tensor_stream as ts
    host, dev = frames
    for fcc, planes, norm in [(RGB24, MERGED, False), (BGR24, PLANAR, True)]:
        got, used = vpp.convert_letterbox([d[0] for d in dev], [d[1] for d in dev], params(ts, (96, 64), rt, fcc, planes, norm), width=[g[0] for g in GEO],
                                          height=[g[1] for g in GEO])
        for k, (w, h, _) in enumerate(GEO):
            left, top, iw, ih = used[k]
            one = vpp.Convert(dev[k][0], dev[k][1], params(ts, (iw, ih), rt, fcc, planes, norm), width=w, height=h)
            torch.cuda.synchronize()
            block = got[k][:, top:top + ih, left:left + iw] if planes == PLANAR else got[k][top:top + ih, left:left + iw, :]
            assert np.array_equal(bits(block), bits(one)), (k, used[k], rt, fcc, planes, norm)


@pytest.mark.parametrize("g_term,ct_bits", [(1, 0), (2, 2048)])
def test_colour_g_term_variants(oracle, frames, g_term, ct_bits):
    """TSVPP_OPT_COLOR_G_TERM against the oracle's matching contraction variant (bits as tests/test_gpu_parity.py sets them), pad included, restored afterwards"""
    import tensor_stream as ts
    from tensor_stream import vpp as V
    CT_RESIZE, CT_INNER = 1 | 2 | 8 | 16 | 64, 256
    host, dev = frames
    v = ts.VideoProcessor(device=0, max_consumers=1)
    try:
        v.set_option(V.OPT_COLOR_G_TERM, g_term)
        oracle.set_contract(CT_RESIZE | CT_INNER | ct_bits)
        try:
            check(v, oracle, host, dev, GEO, (64, 64), BILINEAR, RGB24, PLANAR, False, pad=(77, 201, 33))
            check(v, oracle, host, dev, GEO, (70, 66), BICUBIC, BGR24, MERGED, True, pad=(77, 201, 33))
        finally:
            oracle.set_contract(-1)
        v.set_option(V.OPT_COLOR_G_TERM, 0)
        check(v, oracle, host, dev, GEO, (64, 64), BILINEAR, RGB24, PLANAR, False, pad=(77, 201, 33))
    finally:
        oracle.set_contract(-1)
        v.Close()


def test_graph_capture_replays_bit_exact(vpp, oracle):
    """the per-frame records travel in the kernarg segment: the call allocates, copies and synchronises nothing, is legal during capture, and the graph replays the
    captured request on whatever the frames hold at replay time"""
    import tensor_stream as ts
    geo = [GEO[0], GEO[1], GEO[4]]
    a = [synth_nv12(w, h, seed=310 + k, pitch=p) for k, (w, h, p) in enumerate(geo)]
    dev = [(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()) for y, uv in a]
    fp = params(ts, (64, 64), BICUBIC, RGB24, MERGED, False)
    out = vpp._alloc(fp.parameters, 64, 64, len(geo))
    kw = dict(width=[g[0] for g in geo], height=[g[1] for g in geo], out=out)
    ys, uvs = [d[0] for d in dev], [d[1] for d in dev]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        vpp.convert_letterbox(ys, uvs, fp, **kw)  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        vpp.convert_letterbox(ys, uvs, fp, **kw)
    for seed in (320, 330):
        b = [synth_nv12(w, h, seed=seed + k, pitch=p) for k, (w, h, p) in enumerate(geo)]
        for k in range(len(geo)):
            dev[k][0].copy_(torch.from_numpy(b[k][0]).cuda())
            dev[k][1].copy_(torch.from_numpy(b[k][1]).cuda())
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k, (w, h, _) in enumerate(geo):
            ref = expected_canvas(oracle, b[k][0], b[k][1], w, h, default_rect(w, h, 64, 64), (64, 64), BICUBIC, RGB24, MERGED, False, GRAY)
            assert np.array_equal(bits(out[k]), ref), (seed, k)


def test_status_codes_with_a_live_context(vpp, frames):
    """the validation of tests/test_letterbox_cpu.py answers before any launch; a null plane or output is TSVPP_ERROR"""
    import tensor_stream as ts
    from tensor_stream import _native as N
    host, dev = frames
    y, uv = dev[0]
    w, h, pitch = GEO[0]
    fp = params(ts, (64, 64), BILINEAR, RGB24, MERGED, False)
    one = dict(width=w, height=h)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_letterbox([y], [uv], fp, rects=[(0, 0, 66, 64)], **one)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_letterbox([y], [uv], fp, pad=(256, 128, 128), **one)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_letterbox([y], [uv], fp, rects=[(1, 0, 62, 64)], **one)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_letterbox([y], [uv], params(ts, (64, 64), AREA, RGB24, MERGED, False), **one)
    fr = (N.NV12 * 1)(N.NV12(y.data_ptr(), None, pitch, pitch, w, h))
    out = torch.empty(64 * 64 * 3, dtype=torch.uint8, device="cuda")
    outs = (ctypes.c_void_p * 1)(out.data_ptr())
    L = N.lib()
    assert L.tsvpp_convert_letterbox(vpp._ctx, 1, fr, ctypes.byref(fp.parameters), None, 114, 128, 128, outs, None) == -3
    fr[0].uv = uv.data_ptr()
    outs[0] = None
    assert L.tsvpp_convert_letterbox(vpp._ctx, 1, fr, ctypes.byref(fp.parameters), None, 114, 128, 128, outs, None) == -3
    outs[0] = out.data_ptr()
    assert L.tsvpp_convert_letterbox(vpp._ctx, 1, fr, ctypes.byref(fp.parameters), None, 114, 128, 128, outs, None) == 0
    torch.cuda.synchronize()
