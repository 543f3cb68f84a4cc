"""GPU: tsvpp_convert_letterbox_area -- the letterbox call with AREA: n NV12 frames, each resized by the AREA rules into an inner rectangle of one canvas size, the
rest pad, one launch per 32, the weight rows generated inside the kernel from a jump start.

The contract (include/tsvpp.h): the inner rectangle holds, bit for bit, what the oracle returns for the frame resized with AREA to the rectangle's size; every
other pixel holds what the oracle's conversion without a resize returns for a frame of the constant pad sample.  Every comparison is np.array_equal on the raw
bits against a canvas built from the existing oracle only (tests/letterbox_util.py; tensors: tests/tensor_util.py).  No case is skipped."""
import numpy as np
import pytest
import torch

import tensor_util as T
from letterbox_util import AREA, BGR24, CANVASES, FLAVOURS, GEO, MERGED, PLANAR, RGB24, Y800, bits, default_rect, expected_canvas
from util import frame_k, knob_run, synth_nv12

pytestmark = pytest.mark.gpu

LIMIT = 32  # TSVPP_MAX_LETTERBOX
GRAY = (114, 128, 128)
TWO = [(RGB24, MERGED, False), (BGR24, PLANAR, True)]  # uint8 merged and fp32 planar


def params(ts, canvas, fcc, planes, norm):
    return ts.FrameParameters(width=canvas[0], height=canvas[1], resize_type=AREA, pixel_format=fcc, planes_pos=planes, normalization=norm)


@pytest.fixture(scope="module")
def frames():
    """the frames of GEO (those of tests/test_gpu_letterbox.py): [(y, uv)] on the host, the same on the device"""
    host = [synth_nv12(w, h, seed=700 + k, pitch=p) for k, (w, h, p) in enumerate(GEO)]
    dev = [(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()) for y, uv in host]
    return host, dev


_INNER = {}


def inner_of(oracle, key, y, uv, w, h, size, fcc, planes, norm):
    """the oracle's AREA resize of a frame to the rectangle's size, computed once per (frame, size, flavour) and never modified"""
    k = (key, w, h, size, fcc, planes, norm)
    if k not in _INNER:
        inner, _, _ = oracle.convert(y[:h, :w], uv[:h // 2, :w], dst=size, resize_type=AREA, fourcc=fcc, planes=planes, normalization=norm)
        inner.setflags(write=False)
        _INNER[k] = inner
    return _INNER[k]


def check(v, oracle, host, dev, geo, canvas, fcc, planes, norm, pad=GRAY, rects=None, out=None, only=None, key="geo", what=""):
    """letterbox the frames in one call, compare canvases (all, or the indices `only`) with the expected ones; returns (out, rects)"""
    import tensor_stream as ts
    fp = params(ts, canvas, fcc, planes, norm)
    got, used = v.convert_letterbox_area([d[0] for d in dev], [d[1] for d in dev], fp, pad=pad, rects=rects, out=out, width=[g[0] for g in geo],
                                         height=[g[1] for g in geo])
    torch.cuda.synchronize()
    assert len(used) == len(geo)
    for k in (range(len(geo)) if only is None else only):
        w, h = geo[k][0], geo[k][1]
        want_rect = tuple(rects[k]) if rects is not None else default_rect(w, h, *canvas)
        assert tuple(used[k]) == want_rect, (what, k, used[k], want_rect)
        inner = inner_of(oracle, (key, k), host[k][0], host[k][1], w, h, want_rect[2:], fcc, planes, norm)
        ref = expected_canvas(oracle, host[k][0], host[k][1], w, h, want_rect, canvas, AREA, fcc, planes, norm, pad, inner=inner)
        g = bits(got[k])
        assert g.size == ref.size, (what, k, g.size, ref.size)
        bad = np.flatnonzero(g != ref)
        assert bad.size == 0, (f"{what} frame {k} {geo[k]} -> canvas {canvas} rect {want_rect} fcc={fcc} planes={planes} norm={norm} pad={pad}: "
                               f"{bad.size} bytes differ, first at {bad[:4]}")
    return got, used


@pytest.mark.parametrize("canvas", CANVASES)
def test_geometry_against_the_oracle(vpp, oracle, frames, canvas):
    """every frame of GEO into every canvas, all ten flavours, one launch per canvas: down-scale frames and the 32 x 18 up-scale frame side by side, pad above /
    below and left / right, no pad, the shifted tile column of 4 k + 2 columns, a canvas narrower than a tile (element-wise stores)"""
    import tensor_stream as ts
    host, dev = frames
    assert len(FLAVOURS) == 10
    if not knob_run():
        d = ts.describe_letterbox_area(params(ts, canvas, RGB24, MERGED, False), GEO)
        rects = [default_rect(w, h, *canvas) for w, h, _ in GEO]
        down = sum(1 for (w, h, _), r in zip(GEO, rects) if np.float32(w) / np.float32(r[2]) > 1 and np.float32(h) / np.float32(r[3]) > 1)
        assert d["launches"] == 1 and d["down"] == down
        assert canvas != (64, 64) or 0 < down < len(GEO)  # one launch mixes both rules
    for fcc, planes, norm in FLAVOURS:
        check(vpp, oracle, host, dev, GEO, canvas, fcc, planes, norm)
    for fcc, planes, norm in TWO:  # a pad that runs into the colour back end's clamps
        check(vpp, oracle, host, dev, GEO, canvas, fcc, planes, norm, pad=(3, 250, 7))


# (frame w, h, pitch), canvas, rectangle: the period classes of the jump start (P_x / P_y worked out in tests/test_letterbox_area_cpu.py's restatement)
PERIODS = [
    ((192, 108, 192), (64, 64), (0, 14, 64, 36)),      # 1 / 1
    ((240, 180, 256), (100, 100), (0, 12, 100, 76)),   # 5 / 19: tile columns start at 32, 64, 96 -- first % 5 = 2, 4, 1
    ((200, 150, 208), (96, 64), (10, 4, 76, 58)),      # 19 / 29
    ((214, 182, 224), (70, 66), (0, 0, 70, 66)),       # 105 / 33: x never closes inside the output; the shifted last tile column
    ((322, 182, 384), (64, 64), (0, 14, 64, 36)),      # 32 / 18: a tile starts exactly on a reset (column 32; canvas row 32 is inner row 18)
]


@pytest.mark.parametrize("case", range(len(PERIODS)))
def test_period_classes(vpp, oracle, case):
    (w, h, pitch), canvas, rect = PERIODS[case]
    y, uv = synth_nv12(w, h, seed=4100 + case, pitch=pitch)
    dev = [(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda())]
    for fcc, planes, norm in TWO:
        check(vpp, oracle, [(y, uv)], dev, [(w, h, pitch)], canvas, fcc, planes, norm, rects=[rect], key=("period", case))


def test_rectangles_of_the_caller(vpp, oracle, frames):
    """rectangles off every tile boundary: left = 14 (an odd multiple of 2: the edge splits 4-column thread tiles), one that fills the canvas, one in the last rows
    and columns, a ten-column one (322 -> 10 columns: 33 taps)"""
    host, dev = frames
    rects = [(14, 2, 20, 10), (0, 0, 64, 64), (34, 50, 30, 14), (2, 2, 60, 60), (54, 0, 10, 64)]
    for fcc, planes, norm in TWO + [(RGB24, MERGED, True), (Y800, MERGED, False)]:
        check(vpp, oracle, host, dev, GEO, (64, 64), fcc, planes, norm, rects=rects, key="rects")
    check(vpp, oracle, host[:2], dev[:2], GEO[:2], (70, 66), BGR24, PLANAR, False, rects=[(42, 2, 26, 64), (0, 0, 70, 66)], key="rects70")


def test_canvas_equal_to_the_rectangle_is_convert_batch(vpp, frames):
    """the two paths of the library agree byte for byte: a rectangle that is the whole canvas holds the GPU's own convert_batch(AREA)"""
    import tensor_stream as ts
    host, dev = frames
    for k in (0, 3, 4):  # down-scale, up-scale, a ratio above 5
        w, h, _ = GEO[k]
        for canvas in [(64, 36), (70, 66)]:
            for fcc, planes, norm in TWO:
                fp = params(ts, canvas, fcc, planes, norm)
                got, _ = vpp.convert_letterbox_area([dev[k][0]], [dev[k][1]], fp, rects=[(0, 0) + canvas], width=w, height=h)
                one = vpp.convert_batch([dev[k][0]], [dev[k][1]], fp, width=w, height=h)
                torch.cuda.synchronize()
                assert np.array_equal(bits(got[0]), bits(one[0])), (k, canvas, fcc, planes, norm)


def test_33_frames_are_two_launches(vpp, oracle, frames):
    """one call, frames of different size and pitch, distinct content per frame (every byte + 37 k): the first and the last canvas of every launch are right"""
    import tensor_stream as ts
    host, dev = frames
    n = LIMIT + 1
    geo = [GEO[k % 3] for k in range(n)]
    h = [(frame_k(host[k % 3][0], k), frame_k(host[k % 3][1], k)) for k in range(n)]
    d = [(dev[k % 3][0] + (37 * k) % 256, dev[k % 3][1] + (37 * k) % 256) for k in range(n)]
    desc = ts.describe_letterbox_area(params(ts, (64, 64), BGR24, PLANAR, True), geo)
    assert desc["launches"] == 2 and desc["frames"] == n and desc["limit"] == LIMIT
    only = [0, LIMIT - 1, LIMIT]
    check(vpp, oracle, h, d, geo, (64, 64), BGR24, PLANAR, True, only=only, key="33")
    check(vpp, oracle, h, d, geo, (70, 66), RGB24, MERGED, False, only=only, key="33")


def test_staged_and_gathering_tiles(oracle, frames, monkeypatch):
    """TSVPP_LDS_KB (read when a context is created) sized so that, in ONE launch, the tiles of the 128 x 72 frame stage their footprint behind the weight rows and
    those of the 322 x 182 frame gather from global memory; then no budget at all: every tile gathers, the rows still live in LDS.  The same bits, the oracle's."""
    import tensor_stream as ts
    host, dev = frames
    pick = [0, 4]
    geo, h, d = [GEO[k] for k in pick], [host[k] for k in pick], [dev[k] for k in pick]
    for kb, staged in (("12", 1), ("0", 0)):
        monkeypatch.setenv("TSVPP_LDS_KB", kb)
        v = ts.VideoProcessor(device=0, max_consumers=1)
        try:
            if not knob_run(("TSVPP_LDS_KB",)):
                desc = ts.describe_letterbox_area(params(ts, (64, 64), BGR24, PLANAR, True), geo)
                assert desc["staged"] == staged and desc["kernel"].endswith("staged>" if staged else "gather>") and desc["lds"] > 0
            for fcc, planes, norm in TWO:
                check(v, oracle, h, d, geo, (64, 64), fcc, planes, norm, key="mix")
        finally:
            v.Close()


FORMATS = [(RGB24, PLANAR), (BGR24, PLANAR), (Y800, MERGED)]


@pytest.mark.parametrize("canvas", [(64, 64), (70, 66), (30, 34)])
def test_tensors_with_mean_and_scale(vpp, oracle, frames, canvas):
    """fp16 / bf16 / fp32 elements of (q - mean[c]) * scale[c], the pad included: q is the fp32 planar canvas above, then tensor_util's two float32 operations and
    one conversion"""
    import tensor_stream as ts
    host, dev = frames
    kw = dict(width=[g[0] for g in GEO], height=[g[1] for g in GEO])
    for fcc, planes in FORMATS:
        c = 1 if fcc == Y800 else 3
        qs = []
        for k, (w, h, _) in enumerate(GEO):
            rect = default_rect(w, h, *canvas)
            inner = inner_of(oracle, ("geo", k), host[k][0], host[k][1], w, h, rect[2:], fcc, PLANAR if fcc != Y800 else MERGED, True)
            qs.append(expected_canvas(oracle, host[k][0], host[k][1], w, h, rect, canvas, AREA, fcc, PLANAR, True, GRAY, inner=inner).view(np.float32))
        for dtype in T.DTYPES:
            for name, spec in (("imagenet", T.IMAGENET), ("corner", T.CORNER)):
                got, used = vpp.convert_letterbox_area([d[0] for d in dev], [d[1] for d in dev], params(ts, canvas, fcc, planes, True), dtype=T.TORCH[dtype],
                                                       mean=spec[0], std=spec[1], **kw)
                torch.cuda.synchronize()
                for k in range(len(GEO)):
                    assert got[k].dtype == T.TORCH[dtype]
                    ref = T.expected(qs[k], c, spec, dtype)
                    g = T.bits(got[k])
                    assert g.size == ref.size == c * canvas[0] * canvas[1] * T.ESIZE[dtype]
                    bad = np.flatnonzero(g != ref)
                    assert bad.size == 0, f"{name} {dtype} frame {k} canvas {canvas} fcc={fcc}: {bad.size} bytes differ, first at {bad[:4]}"
        # dtype = fp32, mean 0, scale 1: the bits of the call without a spec
        old, _ = vpp.convert_letterbox_area([d[0] for d in dev], [d[1] for d in dev], params(ts, canvas, fcc, planes, True), **kw)
        new, _ = vpp.convert_letterbox_area([d[0] for d in dev], [d[1] for d in dev], params(ts, canvas, fcc, planes, True), dtype=torch.float32, **kw)
        torch.cuda.synchronize()
        for k in range(len(GEO)):
            assert np.array_equal(T.bits(old[k]), T.bits(new[k])), (canvas, fcc, k)


def test_graph_capture_in_a_fresh_context(vpp, oracle, frames):
    """a context that has never seen the scale: the call allocates, copies and synchronises nothing, so its FIRST run may be the captured one (the kernel itself has
    run before, in another context at other scales: loading code is the runtime's business, not the call's); the graph replays the captured request on whatever the
    frames hold at replay time"""
    import tensor_stream as ts
    from tensor_stream import _native as N
    geo = [(250, 140, 256), (72, 128, 96), (322, 182, 384)]  # 250 -> 64: a ratio no other test uses
    a = [synth_nv12(w, h, seed=5310 + k, pitch=p) for k, (w, h, p) in enumerate(geo)]
    dev = [(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()) for y, uv in a]
    fp = params(ts, (64, 64), RGB24, MERGED, False)
    vpp.convert_letterbox_area([d[0] for d in frames[1]], [d[1] for d in frames[1]], fp, width=[g[0] for g in GEO], height=[g[1] for g in GEO])
    torch.cuda.synchronize()
    v = ts.VideoProcessor(device=0, max_consumers=1)
    try:
        out = v._alloc(fp.parameters, 64, 64, len(geo))
        kw = dict(width=[g[0] for g in geo], height=[g[1] for g in geo], out=out)
        ys, uvs = [d[0] for d in dev], [d[1] for d in dev]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            v.convert_letterbox_area(ys, uvs, fp, **kw)  # no warm-up: the first call of this context
        assert N.lib().tsvpp_debug_area_tables(v._ctx) == 0  # nothing cached
        for seed in (5320, 5330):
            b = [synth_nv12(w, h, seed=seed + k, pitch=p) for k, (w, h, p) in enumerate(geo)]
            for k in range(len(geo)):
                dev[k][0].copy_(torch.from_numpy(b[k][0]).cuda())
                dev[k][1].copy_(torch.from_numpy(b[k][1]).cuda())
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            for k, (w, h, _) in enumerate(geo):
                ref = expected_canvas(oracle, b[k][0], b[k][1], w, h, default_rect(w, h, 64, 64), (64, 64), AREA, RGB24, MERGED, False, GRAY)
                assert np.array_equal(bits(out[k]), ref), (seed, k)
    finally:
        v.Close()


def test_status_codes_with_a_live_context(vpp, frames):
    """the validation of tests/test_letterbox_area_cpu.py answers before any launch; the existing call keeps refusing AREA"""
    import tensor_stream as ts
    host, dev = frames
    y, uv = dev[0]
    one = dict(width=GEO[0][0], height=GEO[0][1])
    fp = params(ts, (64, 64), RGB24, MERGED, False)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_letterbox_area([y], [uv], fp, rects=[(0, 0, 66, 64)], **one)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_letterbox_area([y], [uv], fp, rects=[(0, 0, 2, 64)], **one)  # 128 -> 2 columns: 64 taps
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_letterbox_area([y], [uv], ts.FrameParameters(width=64, height=64, resize_type=1, pixel_format=RGB24, planes_pos=MERGED, normalization=False), **one)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_letterbox([y], [uv], fp, **one)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_letterbox_area([y], [uv], fp, dtype=torch.float16, **one)  # a spec needs normalization
