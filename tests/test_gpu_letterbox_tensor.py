"""GPU: tsvpp_convert_letterbox_tensor -- letterboxed canvases as what a network takes: fp32 / fp16 / bf16 elements of (q - mean[c]) * scale[c], planar RGB24 /
BGR24 and Y800; the pad pixel goes through the same expression as every sample.

The expected bits come from the existing oracle alone: letterbox_util.expected_canvas (the fp32 planar canvas q of tsvpp_convert_letterbox), then tensor_util's
float32 subtraction and multiplication and numpy's / torch's round-to-nearest-even conversion.  Every comparison is np.array_equal on raw bytes.  A canvas q is
computed once and shared by every dtype and spec."""
import numpy as np
import pytest
import torch

import tensor_util as T
from letterbox_util import BGR24, BICUBIC, BILINEAR, CANVASES, GEO, MERGED, NEAREST, PLANAR, RGB24, Y800, default_rect, expected_canvas
from util import frame_k, knob_run, synth_nv12

pytestmark = pytest.mark.gpu

LIMIT = 32  # TSVPP_MAX_LETTERBOX
GRAY = (114, 128, 128)
FORMATS = [(RGB24, PLANAR), (BGR24, PLANAR), (Y800, MERGED)]
SPECS = [("imagenet", T.IMAGENET), ("corner", T.CORNER)]


def params(ts, canvas, rt, fcc, planes, norm=True):
    return ts.FrameParameters(width=canvas[0], height=canvas[1], resize_type=rt, pixel_format=fcc, planes_pos=planes, normalization=norm)


@pytest.fixture(scope="module")
def frames():
    """the frames of GEO (those of tests/test_gpu_letterbox.py): [(y, uv)] on the host, the same on the device"""
    host = [synth_nv12(w, h, seed=700 + k, pitch=p) for k, (w, h, p) in enumerate(GEO)]
    dev = [(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()) for y, uv in host]
    return host, dev


_Q = {}


def q_of(oracle, key, y, uv, w, h, rect, canvas, rt, fcc, pad):
    """the fp32 planar canvas of the existing entry point, cached (never modified)"""
    k = (key, w, h, rect, canvas, rt, fcc, pad)
    if k not in _Q:
        q = expected_canvas(oracle, y, uv, w, h, rect, canvas, rt, fcc, PLANAR, True, pad).view(np.float32)
        q.setflags(write=False)
        _Q[k] = q
    return _Q[k]


def check(v, oracle, host, dev, geo, canvas, rt, fcc, planes, dtype, spec, pad=GRAY, rects=None, out=None, only=None, key="geo", what=""):
    import tensor_stream as ts
    fp = params(ts, canvas, rt, fcc, planes)
    got, used = v.convert_letterbox([d[0] for d in dev], [d[1] for d in dev], fp, pad=pad, rects=rects, out=out, width=[g[0] for g in geo], height=[g[1] for g in geo],
                                    dtype=T.TORCH[dtype], mean=spec[0], std=spec[1])
    torch.cuda.synchronize()
    c = 1 if fcc == Y800 else 3
    for k in (range(len(geo)) if only is None else only):
        w, h = geo[k][0], geo[k][1]
        want_rect = tuple(rects[k]) if rects is not None else default_rect(w, h, *canvas)
        assert tuple(used[k]) == want_rect and got[k].dtype == T.TORCH[dtype]
        ref = T.expected(q_of(oracle, (key, k), host[k][0], host[k][1], w, h, want_rect, canvas, rt, fcc, pad), c, spec, dtype)
        g = T.bits(got[k])
        assert g.size == ref.size == c * canvas[0] * canvas[1] * T.ESIZE[dtype], (what, k, g.size, ref.size)
        bad = np.flatnonzero(g != ref)
        assert bad.size == 0, f"{what} frame {k} {geo[k]} -> canvas {canvas} rect {want_rect} rt={rt} fcc={fcc} {dtype} pad={pad}: {bad.size} bytes differ, first at {bad[:4]}"
    return got, used


@pytest.mark.parametrize("canvas", CANVASES)
@pytest.mark.parametrize("rt", [NEAREST, BILINEAR, BICUBIC])
def test_geometry_against_the_oracle(vpp, oracle, frames, rt, canvas):
    """every frame of GEO into every canvas: formats x dtypes x specs, and both pads -- the pad goes through the affine step"""
    host, dev = frames
    for fcc, planes in FORMATS:
        for dtype in T.DTYPES:
            for name, spec in SPECS:
                check(vpp, oracle, host, dev, GEO, canvas, rt, fcc, planes, dtype, spec, what=name)
                if rt == BILINEAR:  # a pad that runs into the colour back end's clamps
                    check(vpp, oracle, host, dev, GEO, canvas, rt, fcc, planes, dtype, spec, pad=(3, 250, 7), what=name)


def test_the_pad_goes_through_the_affine_step(vpp, oracle, frames):
    """stated on its own: a canvas pixel outside the rectangle is cvt((q_pad - mean[c]) * scale[c]), not q_pad and not zero"""
    import tensor_stream as ts
    from letterbox_util import pad_pixel
    host, dev = frames
    fp = params(ts, (64, 64), BILINEAR, RGB24, PLANAR)
    got, used = vpp.convert_letterbox([dev[0][0]], [dev[0][1]], fp, pad=GRAY, width=[GEO[0][0]], height=[GEO[0][1]], dtype=torch.float16, mean=T.IMAGENET[0],
                                      std=T.IMAGENET[1])
    torch.cuda.synchronize()
    assert used[0][1] > 0  # pad rows above the rectangle
    px = pad_pixel(oracle, GRAY, RGB24, PLANAR, True)
    want = T.expected(px.reshape(3, 1), 3, T.IMAGENET, T.F16).view(np.float16)
    corner = got[0][:, 0, 0].cpu().numpy()
    assert np.array_equal(corner.view(np.uint16), want.view(np.uint16)) and not np.array_equal(corner, px.astype(np.float16))


@pytest.mark.parametrize("rt", [NEAREST, BILINEAR, BICUBIC])
def test_rectangles_of_the_caller(vpp, oracle, frames, rt):
    """the rectangles of tests/test_gpu_letterbox.py: a small one off every tile boundary, one that fills the canvas, one in the last rows and columns"""
    host, dev = frames
    rects = [(6, 2, 20, 10), (0, 0, 64, 64), (34, 50, 30, 14), (2, 2, 60, 60), (62, 0, 2, 64)]
    for (fcc, planes), dtype, (name, spec) in [((RGB24, PLANAR), T.F16, SPECS[0]), ((BGR24, PLANAR), T.BF16, SPECS[1]), ((Y800, MERGED), T.F16, SPECS[1]),
                                               ((BGR24, PLANAR), T.F32, SPECS[0])]:
        check(vpp, oracle, host, dev, GEO, (64, 64), rt, fcc, planes, dtype, spec, rects=rects, what=name)
    check(vpp, oracle, host[:2], dev[:2], GEO[:2], (70, 66), rt, BGR24, PLANAR, T.F16, T.IMAGENET, rects=[(40, 2, 30, 64), (0, 0, 70, 66)])


def test_33_frames_are_two_launches(vpp, oracle, frames):
    """one call, frames of different size and pitch, distinct content per frame (every byte + 37 k): the first and the last canvas of every launch are right"""
    import tensor_stream as ts
    host, dev = frames
    n = LIMIT + 1
    geo = [GEO[k % 3] for k in range(n)]
    h = [(frame_k(host[k % 3][0], k), frame_k(host[k % 3][1], k)) for k in range(n)]
    d = [(dev[k % 3][0] + (37 * k) % 256, dev[k % 3][1] + (37 * k) % 256) for k in range(n)]
    desc = ts.describe_letterbox(params(ts, (64, 64), BILINEAR, BGR24, PLANAR), geo, dtype=torch.float16)
    assert desc["launches"] == 2 and desc["frames"] == n
    only = [0, LIMIT - 1, LIMIT]
    check(vpp, oracle, h, d, geo, (64, 64), BILINEAR, BGR24, PLANAR, T.F16, T.IMAGENET, only=only, key="33")
    check(vpp, oracle, h, d, geo, (70, 66), BICUBIC, RGB24, PLANAR, T.BF16, T.CORNER, only=only, key="33")


GUARD = 256


@pytest.mark.parametrize("canvas", [(64, 64), (70, 66), (30, 34)])
@pytest.mark.parametrize("rt,fcc,planes,dtype,off", [(BILINEAR, BGR24, PLANAR, T.F16, 0), (BILINEAR, BGR24, PLANAR, T.F16, 2), (BICUBIC, RGB24, PLANAR, T.BF16, 4),
                                                     (NEAREST, Y800, MERGED, T.F16, 2), (BILINEAR, RGB24, PLANAR, T.F32, 4), (BICUBIC, Y800, MERGED, T.BF16, 0)])
def test_unaligned_canvases_and_guard_bytes(vpp, oracle, frames, rt, fcc, planes, dtype, off, canvas):
    """canvases 0 / 2 / 4 bytes past a 16-byte boundary (vector-store and element-wise kernels); the 256 bytes before and after every canvas stay as written"""
    import tensor_stream as ts
    host, dev = frames
    n = len(GEO)
    nbytes = (1 if fcc == Y800 else 3) * canvas[0] * canvas[1] * T.ESIZE[dtype]
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
    out = [s.view(T.TORCH[dtype]) for s in slots]
    check(vpp, oracle, host, dev, GEO, canvas, rt, fcc, planes, dtype, T.IMAGENET, out=out, what=f"offset {off}")
    want = buf.clone()
    for s in starts:
        want[s:s + nbytes] = pat[s:s + nbytes]
    if not torch.equal(want, pat):
        bad = torch.nonzero(want != pat).flatten()[0].item()
        k = min(bad // stride, n - 1)
        raise AssertionError(f"guard byte damaged at {bad - starts[k]} relative to canvas {k} of {nbytes} bytes (offset {off}, canvas {canvas})")
    if not knob_run():
        d = ts.describe_letterbox(params(ts, canvas, rt, fcc, planes), GEO, aligned_outputs=(off == 0), dtype=T.TORCH[dtype])
        # element-wise stores: canvases off the 16-byte alignment, and widths 4 k + 2 narrower than a tile (no tile column to shift)
        assert d["kernel"].split(",")[-2] == ("vec" if off == 0 and not (canvas[0] % 4 != 0 and canvas[0] < 32) else "elem")
        assert d["tail"] == (2 if (off == 0 and canvas[0] == 70) else 0)


@pytest.mark.parametrize("rt", [NEAREST, BILINEAR, BICUBIC])
def test_identity_f32_is_the_existing_entry_point(vpp, frames, rt):
    import tensor_stream as ts
    host, dev = frames
    kw = dict(width=[g[0] for g in GEO], height=[g[1] for g in GEO])
    for canvas in CANVASES:
        for fcc, planes in FORMATS:
            for pad in (GRAY, (3, 250, 7)):
                fp = params(ts, canvas, rt, fcc, planes)
                old, r0 = vpp.convert_letterbox([d[0] for d in dev], [d[1] for d in dev], fp, pad=pad, **kw)
                new, r1 = vpp.convert_letterbox([d[0] for d in dev], [d[1] for d in dev], fp, pad=pad, dtype=torch.float32, **kw)
                torch.cuda.synchronize()
                assert r0 == r1 and old.dtype == new.dtype == torch.float32 and old.shape == new.shape
                for k in range(len(GEO)):
                    assert np.array_equal(T.bits(old[k]), T.bits(new[k])), (canvas, fcc, pad, k)
