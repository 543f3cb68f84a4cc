"""GPU: tsvpp_convert_rois_tensor -- boxes of NV12 frames as what a network takes: fp32 / fp16 / bf16 elements of (q - mean[c]) * scale[c], planar RGB24 / BGR24
and Y800, all four resize types behind one name.

The expected bits come from the existing oracle alone (tensor_util): the oracle's fp32 planar result q for the box's sliced planes, then the float32 subtraction
and multiplication, then numpy's / torch's round-to-nearest-even conversion.  Every comparison is np.array_equal on raw bytes.  The oracle's q of a
(resize type, format, size, box) is computed once and shared by every dtype and spec."""
import numpy as np
import pytest
import torch

import tensor_util as T
from util import knob_run, synth_nv12

pytestmark = pytest.mark.gpu

NEAREST, BILINEAR, BICUBIC, AREA = 0, 1, 2, 3
Y800, RGB24, BGR24 = 0, 1, 2
PLANAR, MERGED = 0, 1
LIMIT = 64  # TSVPP_MAX_ROIS
GEO = [(128, 72, 192), (322, 182, 384)]
# one tile; 2 x 2 tiles; 4 k + 2 columns (the shifted tile column); narrower than a tile (element-wise stores)
SIZES = [(32, 32), (64, 64), (70, 66), (30, 34)]
FORMATS = [(RGB24, PLANAR), (BGR24, PLANAR), (Y800, MERGED)]


def box_set(dw, dh):
    return [
        (1, 40, 30, 140, 100),            # a down-scale on both axes, 100 x 70
        (0, 10, 8, 30, 24),               # an up-scale, 20 x 16
        (1, 100, 60, 100 + dw, 60 + dh),  # exactly the output size: the plain colour conversion
        (1, 101, 20, 201, 90),            # an odd left (U and V swap)
        (1, 322 - 60, 182 - 50, 322, 182),  # touches the frame's right and bottom edges
        (0, 128 - 40, 72 - 30, 128, 72),
    ]


def params(ts, dst, rt, fcc, planes, norm=True):
    return ts.FrameParameters(width=dst[0], height=dst[1], resize_type=rt, pixel_format=fcc, planes_pos=planes, normalization=norm)


@pytest.fixture(scope="module")
def frames():
    host = [synth_nv12(w, h, seed=900 + k, pitch=p) for k, (w, h, p) in enumerate(GEO)]
    dev = [(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()) for y, uv in host]
    return host, dev


_Q = {}


def q_of(oracle, host, key, box, dst, rt, fcc):
    """the oracle's fp32 planar result of the box, cached (never modified)"""
    k = (key, box, dst, rt, fcc)
    if k not in _Q:
        f, l, t, r, b = box
        y, uv = host[f]
        ref, _, _ = oracle.convert(y[t:b, l:r], uv[t // 2:t // 2 + (b - t) // 2, l:r], dst=dst, resize_type=rt, fourcc=fcc, planes=PLANAR, normalization=True, nthreads=4)
        assert ref.dtype == np.float32
        ref.setflags(write=False)
        _Q[k] = ref
    return _Q[k]


def run(v, host, dev, boxes, dst, rt, fcc, planes, dtype, spec, out=None):
    import tensor_stream as ts
    fp = params(ts, dst, rt, fcc, planes)
    widths, heights = [g[0] for g in GEO[:len(dev)]], [g[1] for g in GEO[:len(dev)]]
    return v.convert_rois([d[0] for d in dev], [d[1] for d in dev], boxes, fp, out=out, width=widths, height=heights, dtype=T.TORCH[dtype], mean=spec[0], std=spec[1])


def check(v, oracle, host, dev, boxes, dst, rt, fcc, planes, dtype, spec, out=None, key="geo", only=None, what=""):
    got = run(v, host, dev, boxes, dst, rt, fcc, planes, dtype, spec, out=out)
    torch.cuda.synchronize()
    c = 1 if fcc == Y800 else 3
    for i in (range(len(boxes)) if only is None else only):
        assert got[i].dtype == T.TORCH[dtype]
        ref = T.expected(q_of(oracle, host, key, boxes[i], dst, rt, fcc), c, spec, dtype)
        g = T.bits(got[i])
        assert g.size == ref.size == c * dst[0] * dst[1] * T.ESIZE[dtype], (what, i, g.size, ref.size)
        bad = np.flatnonzero(g != ref)
        assert bad.size == 0, f"{what} box {i} {boxes[i]} -> {dst} rt={rt} fcc={fcc} {dtype}: {bad.size} bytes differ, first at {bad[:4]}"
    return got


@pytest.mark.parametrize("fcc,planes", FORMATS)
@pytest.mark.parametrize("rt", [NEAREST, BILINEAR, BICUBIC, AREA])
def test_grid_against_the_oracle(vpp, oracle, frames, rt, fcc, planes):
    """resize types x formats x dtypes x specs x sizes, every box of box_set"""
    host, dev = frames
    for dst in SIZES:
        for dtype in T.DTYPES:
            for name, spec in T.SPECS.items():
                check(vpp, oracle, host, dev, box_set(*dst), dst, rt, fcc, planes, dtype, spec, what=name)


@pytest.mark.parametrize("rt", [NEAREST, BILINEAR, BICUBIC, AREA])
def test_identity_f32_is_the_existing_entry_point(vpp, frames, rt):
    import tensor_stream as ts
    host, dev = frames
    widths, heights = [g[0] for g in GEO], [g[1] for g in GEO]
    for dst in SIZES:
        for fcc, planes in FORMATS:
            fp = params(ts, dst, rt, fcc, planes)
            old = (vpp.convert_rois_area if rt == AREA else vpp.convert_rois)([d[0] for d in dev], [d[1] for d in dev], box_set(*dst), fp, width=widths, height=heights)
            new = run(vpp, host, dev, box_set(*dst), dst, rt, fcc, planes, T.F32, T.IDENTITY)
            torch.cuda.synchronize()
            assert old.dtype == new.dtype == torch.float32 and old.shape == new.shape
            for i in range(len(old)):
                assert np.array_equal(T.bits(old[i]), T.bits(new[i])), (dst, fcc, i)


def test_overflow_is_infinity_in_fp16_alone(vpp, oracle, frames):
    host, dev = frames
    boxes = box_set(32, 32)[:3]
    spec = ((0.0, 0.0, 0.0), (1e-6, 1e-6, 1e-6))
    with np.errstate(over="ignore"):
        assert [float(s) for s in T.scales(spec[1])] == [1e6] * 3  # scale = 1e6
        seen = {}
        for dtype in T.DTYPES:
            got = check(vpp, oracle, host, dev, boxes, (32, 32), BILINEAR, RGB24, PLANAR, dtype, spec, what="overflow")
            seen[dtype] = got.float()
    assert bool(torch.isinf(seen[T.F16]).any()) and bool(torch.isfinite(seen[T.BF16]).all()) and bool(torch.isfinite(seen[T.F32]).all())


@pytest.mark.parametrize("fcc", [RGB24, BGR24])
@pytest.mark.parametrize("dtype", [T.F16, T.F32])
def test_colour_coverage_of_the_store(vpp, oracle, fcc, dtype):
    """one box of exactly 256 x 256 -- the plain colour conversion -- from a frame with Y = column, U = row, V = 255 - row: every luma value against 128 chroma pairs
    through the new store function's own copy of the colour arithmetic"""
    y = np.tile(np.arange(256, dtype=np.uint8), (256, 1))
    uv = np.empty((128, 256), np.uint8)
    uv[:, 0::2] = np.arange(128, dtype=np.uint8)[:, None]
    uv[:, 1::2] = 255 - np.arange(128, dtype=np.uint8)[:, None]
    host = [(y, uv)]
    dev = [(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda())]
    import tensor_stream as ts
    boxes = [(0, 0, 0, 256, 256)]
    for name, spec in (("imagenet", T.IMAGENET), ("corner", T.CORNER)):
        fp = params(ts, (256, 256), BILINEAR, fcc, PLANAR)
        got = vpp.convert_rois(dev[0][0], dev[0][1], boxes, fp, dtype=T.TORCH[dtype], mean=spec[0], std=spec[1])
        torch.cuda.synchronize()
        ref = T.expected(q_of(oracle, host, "ramp", boxes[0], (256, 256), BILINEAR, fcc), 3, spec, dtype)
        assert np.array_equal(T.bits(got[0]), ref), (name, fcc, dtype)


def test_65_boxes_are_two_launches(vpp, oracle, frames):
    import tensor_stream as ts
    host, dev = frames
    rng = np.random.default_rng(65)
    boxes = []
    for _ in range(LIMIT + 1):
        f = int(rng.integers(0, 2))
        fw, fh = GEO[f][0], GEO[f][1]
        bw, bh = 2 * int(rng.integers(4, fw // 2 + 1)), 2 * int(rng.integers(4, fh // 2 + 1))
        l, t = int(rng.integers(0, fw - bw + 1)), int(rng.integers(0, fh - bh + 1))
        boxes.append((f, l, t, l + bw, t + bh))
    d = ts.describe_rois(params(ts, (64, 64), BILINEAR, BGR24, PLANAR), [(g[0], g[1], g[2]) for g in GEO], boxes, dtype=torch.float16)
    assert d["launches"] == 2 and d["rois"] == LIMIT + 1
    only = [0, LIMIT - 1, LIMIT]  # the first and the last output of each launch (the second launch holds one)
    check(vpp, oracle, host, dev, boxes, (64, 64), BILINEAR, BGR24, PLANAR, T.F16, T.IMAGENET, key="65", only=only)
    check(vpp, oracle, host, dev, boxes, (64, 64), AREA, RGB24, PLANAR, T.BF16, T.CORNER, key="65", only=only)


GUARD = 256


@pytest.mark.parametrize("dst", [(64, 64), (70, 66), (30, 34)])
@pytest.mark.parametrize("rt,fcc,planes,dtype,off", [(BILINEAR, BGR24, PLANAR, T.F16, 0), (BILINEAR, BGR24, PLANAR, T.F16, 2), (BICUBIC, RGB24, PLANAR, T.BF16, 4),
                                                     (NEAREST, Y800, MERGED, T.F16, 2), (AREA, RGB24, PLANAR, T.F16, 2), (BILINEAR, RGB24, PLANAR, T.F32, 4),
                                                     (AREA, BGR24, PLANAR, T.F32, 0), (BICUBIC, Y800, MERGED, T.BF16, 4)])
def test_unaligned_outputs_and_guard_bytes(vpp, oracle, frames, rt, fcc, planes, dtype, off, dst):
    """outputs 0 / 2 / 4 bytes past a 16-byte boundary (vector-store and element-wise kernels); the 256 bytes before and after every output stay as written"""
    import tensor_stream as ts
    host, dev = frames
    boxes = box_set(*dst)
    n = len(boxes)
    nbytes = (1 if fcc == Y800 else 3) * dst[0] * dst[1] * T.ESIZE[dtype]
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
    check(vpp, oracle, host, dev, boxes, dst, rt, fcc, planes, dtype, T.IMAGENET, out=out, what=f"offset {off}")
    want = buf.clone()
    for s in starts:
        want[s:s + nbytes] = pat[s:s + nbytes]
    if not torch.equal(want, pat):
        bad = torch.nonzero(want != pat).flatten()[0].item()
        k = min(bad // stride, n - 1)
        raise AssertionError(f"guard byte damaged at {bad - starts[k]} relative to output {k} of {nbytes} bytes (offset {off}, dst {dst})")
    if not knob_run():
        d = ts.describe_rois(params(ts, dst, rt, fcc, planes), [(g[0], g[1], g[2]) for g in GEO], boxes, aligned_outputs=(off == 0), dtype=T.TORCH[dtype])
        # element-wise stores: outputs off the 16-byte alignment, and widths 4 k + 2 narrower than a tile (no tile column to shift)
        assert d["kernel"].split(",")[-2] == ("vec" if off == 0 and not (dst[0] % 4 != 0 and dst[0] < 32) else "elem")
        assert d["tail"] == (2 if (off == 0 and dst[0] == 70) else 0)


def test_an_output_off_its_element_alignment_is_refused(vpp, frames):
    """an output must be aligned to its element: TSVPP_ERROR before anything is launched"""
    import ctypes

    import tensor_stream as ts
    from tensor_stream import _native as N
    host, dev = frames
    buf = torch.zeros(3 * 32 * 32 * 4 + 64, dtype=torch.uint8, device="cuda")
    fp = params(ts, (32, 32), BILINEAR, RGB24, PLANAR)
    fr = (N.NV12 * 1)(N.NV12(dev[0][0].data_ptr(), dev[0][1].data_ptr(), GEO[0][2], GEO[0][2], GEO[0][0], GEO[0][1]))
    roi = (N.Roi * 1)(N.Roi(0, 0, 0, 64, 64))
    for dtype, off, want in ((torch.float16, 1, -3), (torch.bfloat16, 3, -3), (torch.float32, 2, -3), (torch.float16, 2, 0), (torch.float32, 4, 0)):
        spec = ts.tensor_spec(dtype=dtype)
        outs = (ctypes.c_void_p * 1)(buf.data_ptr() + off)
        sts = N.lib().tsvpp_convert_rois_tensor(vpp._ctx, 1, fr, 1, roi, ctypes.byref(fp.parameters), ctypes.byref(spec), outs, None)
        torch.cuda.synchronize()
        assert sts == want, (dtype, off, sts)
        if want != 0:
            assert int(buf.sum()) == 0  # nothing was launched
        buf.zero_()


def test_graph_capture_replays_bit_exact(vpp, oracle):
    """the twin of tests/test_gpu_rois.py's capture test for one fp16 call: a single stream, no parallel branches; the spec travels in the kernarg segment with
    the records, so the call allocates, copies and synchronises nothing"""
    import tensor_stream as ts
    a, b = synth_nv12(322, 182, seed=311, pitch=384), synth_nv12(322, 182, seed=312, pitch=384)
    dy, duv = torch.from_numpy(a[0]).cuda(), torch.from_numpy(a[1]).cuda()
    boxes = [bx for bx in box_set(64, 64) if bx[0] == 1]
    boxes = [(0,) + bx[1:] for bx in boxes]
    fp = params(ts, (64, 64), BICUBIC, RGB24, PLANAR)
    out = vpp._alloc(fp.parameters, 64, 64, len(boxes), torch.float16)
    kw = dict(out=out, width=322, height=182, dtype=torch.float16, mean=T.IMAGENET[0], std=T.IMAGENET[1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        vpp.convert_rois(dy, duv, boxes, fp, **kw)  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        vpp.convert_rois(dy, duv, boxes, fp, **kw)
    dy.copy_(torch.from_numpy(b[0]).cuda())
    duv.copy_(torch.from_numpy(b[1]).cuda())
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    for i, bx in enumerate(boxes):
        ref = T.expected(q_of(oracle, [b], "graph", bx, (64, 64), BICUBIC, RGB24), 3, T.IMAGENET, T.F16)
        assert np.array_equal(T.bits(out[i]), ref), (i, bx)
