"""GPU: tsvpp_convert_rois -- many boxes of one or several NV12 frames, each resized to one output size, in one launch per 64 boxes.

The contract (include/tsvpp.h): the output of box (left, top, right, bottom) is, bit for bit, what the oracle returns for the SLICED planes with no crop,

    ys  = y [top : bottom, left : right]                      luma
    uvs = uv[top // 2 : top // 2 + h // 2, left : right]      interleaved chroma, BYTE columns (an odd `left` swaps U and V, as the crop stage does)
    oracle.convert(ys, uvs, dst=(dw, dh), ...)

and, for a box Convert's crop stage accepts (strictly smaller than the frame in both dimensions), what tsvpp_convert(crop = box) returns.  Every comparison
is np.array_equal on the raw bits (uint8 bytes; fp32 viewed as bytes)."""
import os

import numpy as np
import pytest
import torch

from guard_util import arena
from util import knob_run, synth_nv12

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

NEAREST, BILINEAR, BICUBIC, AREA = 0, 1, 2, 3
Y800, RGB24, BGR24 = 0, 1, 2
PLANAR, MERGED = 0, 1
LIMIT = 64  # TSVPP_MAX_ROIS
W, H, PITCH = 1920, 1080, 2048

FLAVOURS = [(fcc, planes, norm) for fcc in (RGB24, BGR24) for planes in (PLANAR, MERGED) for norm in (False, True)] + [(Y800, MERGED, False), (Y800, MERGED, True)]


def box_set(dw, dh):
    """the boxes the issue names, over a 1920 x 1080 frame"""
    return [
        (100, 50, 700, 550),              # down-scale
        (300, 200, 364, 248),             # up-scale
        (400, 300, 400 + dw, 300 + dh),   # the output size itself: a plain colour conversion
        (101, 40, 401, 300),              # odd left (U and V swap)
        (200, 33, 480, 333),              # odd top
        (7, 9, 327, 249),                 # both odd
        (0, 0, 256, 256),                 # touches the left and the top edge
        (W - 310, 400, W, 700),           # the right edge
        (500, H - 200, 900, H),           # the bottom edge
        (0, 100, W, 324),                 # full width (Convert's crop stage would ignore it)
        (800, 0, 1000, H),                # full height
        (600, 300, 1000, 700),            # two overlapping boxes
        (700, 400, 1100, 800),
        (W - 2, H - 2, W, H),             # 2 x 2, in the corner
        (1000, 500, 1800, 600),           # down on x, up on y
        (50, 300, 130, 1000),             # up on x, down on y
    ]


def seeded_boxes(n, seed, frames):
    """n boxes (frame, l, t, r, b) with even sides 2..512 anywhere inside the frames [(w, h), ...]"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        f = int(rng.integers(0, len(frames)))
        fw, fh = frames[f]
        bw = 2 * int(rng.integers(1, min(512, fw) // 2 + 1))
        bh = 2 * int(rng.integers(1, min(512, fh) // 2 + 1))
        l, t = int(rng.integers(0, fw - bw + 1)), int(rng.integers(0, fh - bh + 1))
        out.append((f, l, t, l + bw, t + bh))
    return out


def expect(oracle, y, uv, box, dst, rt, fcc, planes, norm):
    l, t, r, b = box
    w, h = r - l, b - t
    ys = y[t:b, l:l + w]
    uvs = uv[t // 2:t // 2 + h // 2, l:l + w]
    ref, _, _ = oracle.convert(ys, uvs, dst=dst, resize_type=rt, fourcc=fcc, planes=planes, normalization=norm, nthreads=8)
    return ref.view(np.uint8).ravel()


def bits(t):
    return t.contiguous().cpu().numpy().ravel().view(np.uint8)


def params(ts, dst, rt, fcc, planes, norm, crop=(0, 0, 0, 0)):
    return ts.FrameParameters(width=dst[0], height=dst[1], crop_coords=crop, resize_type=rt, pixel_format=fcc, planes_pos=planes, normalization=norm)


def check_rois(v, oracle, frames_host, frames_dev, boxes, dst, rt, fcc, planes, norm, widths=None, out=None, what=""):
    """convert the boxes, compare every one with the oracle on its sliced planes; returns the output"""
    import tensor_stream as ts
    fp = params(ts, dst, rt, fcc, planes, norm)
    got = v.convert_rois([f[0] for f in frames_dev], [f[1] for f in frames_dev], boxes, fp, out=out, width=widths)
    torch.cuda.synchronize()
    for i, b in enumerate(boxes):
        b5 = b if len(b) == 5 else (0,) + tuple(b)
        y, uv = frames_host[b5[0]]
        ref = expect(oracle, y, uv, b5[1:], dst, rt, fcc, planes, norm)
        g = bits(got[i])
        assert g.size == ref.size, (what, i, b, g.size, ref.size)
        bad = np.flatnonzero(g != ref)
        assert bad.size == 0, f"{what} box {i} {b} -> {dst} rt={rt} fcc={fcc} planes={planes} norm={norm}: {bad.size} bytes differ, first at {bad[:4]}"
    return got


@pytest.fixture(scope="module")
def frame():
    y, uv = synth_nv12(W, H, seed=2024, pitch=PITCH)
    return (y, uv), (torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda())


@pytest.mark.parametrize("dst", [(224, 224), (112, 112), (250, 250)])
@pytest.mark.parametrize("fcc,planes,norm", FLAVOURS)
@pytest.mark.parametrize("rt", [NEAREST, BILINEAR, BICUBIC])
def test_box_set_matches_the_oracle_and_the_crop_path(vpp, oracle, frame, rt, fcc, planes, norm, dst):
    import tensor_stream as ts
    host, dev = frame
    boxes = box_set(*dst)
    got = check_rois(vpp, oracle, [host], [dev], boxes, dst, rt, fcc, planes, norm, widths=W)
    # the two paths of the library agree: every box Convert's crop stage accepts, through tsvpp_convert(crop = box)
    cropped = 0
    for i, (l, t, r, b) in enumerate(boxes):
        if r - l < W and b - t < H:
            one = vpp.Convert(dev[0], dev[1], params(ts, dst, rt, fcc, planes, norm, crop=(l, t, r, b)), width=W)
            torch.cuda.synchronize()
            assert np.array_equal(bits(one), bits(got[i])), f"box {i} {(l, t, r, b)}: tsvpp_convert(crop) and tsvpp_convert_rois differ"
            cropped += 1
    assert cropped == len(boxes) - 2  # all but the full-width and the full-height box


def test_a_box_of_the_output_size_is_the_plain_colour_conversion(vpp, oracle, frame):
    """every interpolation weight is zero: BILINEAR and BICUBIC return the bits of a conversion without a resize (which is what the oracle runs for dst == size)"""
    import tensor_stream as ts
    host, dev = frame
    boxes = [(400, 300, 624, 524), (401, 301, 625, 525)]
    outs = [check_rois(vpp, oracle, [host], [dev], boxes, (224, 224), rt, RGB24, MERGED, False, widths=W) for rt in (NEAREST, BILINEAR, BICUBIC)]
    assert np.array_equal(bits(outs[0]), bits(outs[1])) and np.array_equal(bits(outs[0]), bits(outs[2]))
    plain = vpp.Convert(dev[0], dev[1], params(ts, (0, 0), NEAREST, RGB24, MERGED, False, crop=boxes[0]), width=W)
    torch.cuda.synchronize()
    assert np.array_equal(bits(plain), bits(outs[1][0]))


@pytest.mark.parametrize("n", [1, LIMIT, LIMIT + 1, 3 * LIMIT + 5])
@pytest.mark.parametrize("rt,fcc,planes,norm,dst", [(BILINEAR, BGR24, PLANAR, True, (112, 112)), (BICUBIC, RGB24, MERGED, False, (112, 112)),
                                                    (NEAREST, Y800, MERGED, False, (96, 64))])
def test_splitting_over_launches(vpp, oracle, frame, n, rt, fcc, planes, norm, dst):
    host, dev = frame
    boxes = seeded_boxes(n, seed=1000 + n, frames=[(W, H)])
    check_rois(vpp, oracle, [host], [dev], boxes, dst, rt, fcc, planes, norm, widths=W, what=f"n={n}")


@pytest.mark.parametrize("n_frames", [2, 3])
def test_frames_of_different_size_and_pitch(vpp, oracle, n_frames):
    geo = [(1920, 1080, 2048, 2048), (1280, 720, 1280, 1280), (640, 360, 704, 768)][:n_frames]
    host, dev = [], []
    for k, (w, h, py, puv) in enumerate(geo):
        rng = np.random.default_rng(77 + k)
        y = rng.integers(0, 256, (h, py), dtype=np.uint8)
        uv = rng.integers(0, 256, (h // 2, puv), dtype=np.uint8)
        host.append((y, uv))
        dev.append((torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()))
    boxes = seeded_boxes(40, seed=5 + n_frames, frames=[(g[0], g[1]) for g in geo])
    boxes = sorted(boxes, key=lambda b: -b[0])  # frame indices out of order: the last frame's boxes first ...
    boxes = boxes[1::2] + boxes[0::2]           # ... and interleaved
    assert {b[0] for b in boxes} == set(range(n_frames)) and [b[0] for b in boxes] != sorted(b[0] for b in boxes)
    widths = [g[0] for g in geo]
    for rt, fcc, planes, norm in [(BILINEAR, RGB24, PLANAR, False), (BICUBIC, BGR24, MERGED, True), (NEAREST, RGB24, MERGED, False)]:
        check_rois(vpp, oracle, host, dev, boxes, (224, 224), rt, fcc, planes, norm, widths=widths, what=f"{n_frames} frames")


@pytest.mark.parametrize("dst", [(224, 224), (250, 250), (30, 30)])
@pytest.mark.parametrize("rt,fcc,planes,norm,off", [(BILINEAR, BGR24, PLANAR, True, 0), (BILINEAR, BGR24, PLANAR, True, 4), (BICUBIC, RGB24, MERGED, True, 4),
                                                    (BICUBIC, RGB24, MERGED, False, 0), (BICUBIC, RGB24, MERGED, False, 1), (BILINEAR, RGB24, MERGED, False, 4),
                                                    (NEAREST, BGR24, PLANAR, False, 1), (NEAREST, BGR24, PLANAR, False, 4), (BILINEAR, Y800, MERGED, False, 1),
                                                    (NEAREST, Y800, MERGED, True, 4), (BILINEAR, RGB24, MERGED, True, 0), (NEAREST, BGR24, PLANAR, False, 0)])
def test_unaligned_outputs_and_guard_bytes(vpp, oracle, frame, rt, fcc, planes, norm, off, dst):
    """outputs 0 / 1 / 4 bytes past a 16-byte boundary (vector-store and element-wise kernels); the bytes before and after every output stay as they were"""
    import tensor_stream as ts
    host, dev = frame
    boxes = box_set(*dst)[:8] + seeded_boxes(3, seed=dst[0] + off, frames=[(W, H)])
    boxes = [b if len(b) == 4 else b[1:] for b in boxes]
    n = len(boxes)
    nbytes = (1 if fcc == Y800 else 3) * dst[0] * dst[1] * (4 if norm else 1)
    _, slots, verify = arena([nbytes] * n, off, what="output", where=f"dst {dst}")
    out = [s.view(torch.float32) if norm else s for s in slots]
    check_rois(vpp, oracle, [host], [dev], boxes, dst, rt, fcc, planes, norm, widths=W, out=out, what=f"offset {off}")
    verify()
    if not knob_run():
        d = ts.describe_rois(params(ts, dst, rt, fcc, planes, norm), (W, H, PITCH), boxes, aligned_outputs=(off == 0))
        # element-wise stores: outputs off the 16-byte alignment, and widths 4 k + 2 narrower than a tile (no tile column to shift)
        assert d["kernel"].split(",")[2] == ("vec" if off == 0 and not (dst[0] % 4 != 0 and dst[0] < 32) else "elem")
        assert d["tail"] == (2 if (off == 0 and dst[0] == 250) else 0)


def test_staged_and_gather_paths(oracle, frame, monkeypatch):
    """the LDS budget decides per box: with none (TSVPP_LDS_KB=0, read when a context is created) every box gathers from global memory -- same bits"""
    import tensor_stream as ts
    host, dev = frame
    boxes = box_set(224, 224)
    cases = [(BILINEAR, BGR24, PLANAR, True), (BICUBIC, RGB24, MERGED, False), (NEAREST, Y800, MERGED, False)]
    for kb in (None, "0"):
        if kb is not None:
            monkeypatch.setenv("TSVPP_LDS_KB", kb)
        v = ts.VideoProcessor(device=0, max_consumers=1)
        try:
            for rt, fcc, planes, norm in cases:
                if not knob_run(("TSVPP_LDS_KB",)):
                    d = ts.describe_rois(params(ts, (224, 224), rt, fcc, planes, norm), (W, H, PITCH), boxes)
                    if kb is None:  # most boxes stage; the full-width box (a 32-column tile taps 275 x 34 luma bytes: fine) too, the full-height one as well
                        assert d["kernel"].endswith("staged>") and d["staged"] >= len(boxes) - 2 and d["lds"] > 0
                    else:
                        assert d["kernel"].endswith("gather>") and d["staged"] == 0
                check_rois(v, oracle, [host], [dev], boxes, (224, 224), rt, fcc, planes, norm, widths=W, what=f"TSVPP_LDS_KB={kb}")
        finally:
            v.Close()


def test_a_launch_mixes_staged_and_gathering_boxes(vpp, oracle, frame):
    """a box whose tiles outgrow the LDS budget (1920 x 1080 -> 112 x 112: a tile taps 566 x 318 luma bytes) beside small ones, in one launch"""
    import tensor_stream as ts
    host, dev = frame
    boxes = [(0, 0, W, H), (100, 100, 300, 300), (0, 0, W, 540), (7, 9, 71, 73)]
    if not knob_run():
        d = ts.describe_rois(params(ts, (112, 112), BICUBIC, RGB24, PLANAR, True), (W, H, PITCH), boxes)
        assert d["kernel"].endswith("staged>") and 0 < d["staged"] < len(boxes)
    for rt in (NEAREST, BILINEAR, BICUBIC):
        check_rois(vpp, oracle, [host], [dev], boxes, (112, 112), rt, RGB24, PLANAR, True, widths=W)
        check_rois(vpp, oracle, [host], [dev], boxes, (112, 112), rt, BGR24, MERGED, False, widths=W)


@pytest.mark.parametrize("g_term,ct_bits", [(1, 0), (2, 2048)])
def test_colour_g_term_variants(oracle, frame, g_term, ct_bits):
    """TSVPP_OPT_COLOR_G_TERM against the oracle's matching contraction variant (bits as tests/test_gpu_parity.py sets them), restored afterwards"""
    import tensor_stream as ts
    from tensor_stream import vpp as V
    CT_RESIZE, CT_INNER = 1 | 2 | 8 | 16 | 64, 256
    host, dev = frame
    boxes = box_set(224, 224)[:6]
    v = ts.VideoProcessor(device=0, max_consumers=1)
    try:
        v.set_option(V.OPT_COLOR_G_TERM, g_term)
        oracle.set_contract(CT_RESIZE | CT_INNER | ct_bits)
        try:
            check_rois(v, oracle, [host], [dev], boxes, (224, 224), BILINEAR, RGB24, PLANAR, False, widths=W)
            check_rois(v, oracle, [host], [dev], boxes, (224, 224), BICUBIC, BGR24, MERGED, True, widths=W)
        finally:
            oracle.set_contract(-1)
        v.set_option(V.OPT_COLOR_G_TERM, 0)
        check_rois(v, oracle, [host], [dev], boxes, (224, 224), BILINEAR, RGB24, PLANAR, False, widths=W)
    finally:
        oracle.set_contract(-1)
        v.Close()


def test_stream_order_after_an_asynchronous_upload(vpp, oracle):
    """a conversion enqueued after an asynchronous upload of the frame on the same stream sees the uploaded data (an ordinary in-order launch)"""
    import tensor_stream as ts
    y, uv = synth_nv12(1280, 720, seed=91)
    py, puv = torch.from_numpy(y).pin_memory(), torch.from_numpy(uv).pin_memory()
    dy, duv = torch.zeros((720, 1280), dtype=torch.uint8, device="cuda"), torch.zeros((360, 1280), dtype=torch.uint8, device="cuda")
    boxes = seeded_boxes(24, seed=8, frames=[(1280, 720)])
    fp = params(ts, (224, 224), BILINEAR, BGR24, PLANAR, True)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        dy.copy_(py, non_blocking=True)
        duv.copy_(puv, non_blocking=True)
        got = vpp.convert_rois(dy, duv, boxes, fp)
    s.synchronize()
    for i, b in enumerate(boxes):
        assert np.array_equal(bits(got[i]), expect(oracle, y, uv, b[1:], (224, 224), BILINEAR, BGR24, PLANAR, True)), (i, b)


def test_graph_capture_replays_bit_exact(vpp, oracle):
    """the per-box records travel in the kernarg segment: the call allocates, copies and synchronises nothing, is legal during capture, and the graph replays the
    captured boxes on whatever the frame holds at replay time"""
    import tensor_stream as ts
    a, b = synth_nv12(1280, 720, seed=301), synth_nv12(1280, 720, seed=302)
    dy, duv = torch.from_numpy(a[0]).cuda(), torch.from_numpy(a[1]).cuda()
    boxes = seeded_boxes(LIMIT + 6, seed=12, frames=[(1280, 720)])  # two launches
    fp = params(ts, (112, 112), BICUBIC, RGB24, MERGED, False)
    out = vpp._alloc(fp.parameters, 112, 112, len(boxes))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        vpp.convert_rois(dy, duv, boxes, fp, out=out)  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        vpp.convert_rois(dy, duv, boxes, fp, out=out)
    dy.copy_(torch.from_numpy(b[0]).cuda())
    duv.copy_(torch.from_numpy(b[1]).cuda())
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    for i, bx in enumerate(boxes):
        assert np.array_equal(bits(out[i]), expect(oracle, b[0], b[1], bx[1:], (112, 112), BICUBIC, RGB24, MERGED, False)), (i, bx)


def test_bunny_boxes(vpp, oracle):
    """picture content, not only noise, through BICUBIC's tie test (flat sky: sums AT half-integers) and the other samplers"""
    z = np.load(os.path.join(HERE, "golden", "bunny_idr129_1280x720.npz"))
    y, uv = np.ascontiguousarray(z["y"]), np.ascontiguousarray(z["uv"])
    dev = (torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda())
    boxes = [(0, 0, 320, 200), (480, 200, 800, 520), (321, 91, 1121, 631), (1000, 500, 1280, 720), (600, 333, 664, 397), (0, 0, 1280, 720), (200, 0, 424, 224)]
    for rt in (NEAREST, BILINEAR, BICUBIC):
        for fcc, planes, norm in [(RGB24, MERGED, False), (BGR24, PLANAR, True), (Y800, MERGED, False)]:
            check_rois(vpp, oracle, [(y, uv)], [dev], boxes, (224, 224), rt, fcc, planes, norm, widths=1280, what="bunny")
    check_rois(vpp, oracle, [(y, uv)], [dev], boxes, (256, 256), BICUBIC, RGB24, PLANAR, False, widths=1280, what="bunny")


def test_status_codes_with_a_live_context(vpp, frame):
    """the validation of tests/test_rois_cpu.py answers before any launch; a null plane or output is TSVPP_ERROR"""
    import ctypes

    import tensor_stream as ts
    from tensor_stream import _native as N
    host, dev = frame
    fp = params(ts, (224, 224), BILINEAR, RGB24, MERGED, False)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_rois(dev[0], dev[1], [(0, 0, 2000, 100)], fp, width=W)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_rois(dev[0], dev[1], [(0, 0, 101, 100)], fp, width=W)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_rois(dev[0], dev[1], [(0, 0, 100, 100)], params(ts, (224, 224), AREA, RGB24, MERGED, False), width=W)
    fr = (N.NV12 * 1)(N.NV12(dev[0].data_ptr(), None, PITCH, PITCH, W, H))
    roi = (N.Roi * 1)(N.Roi(0, 0, 0, 64, 64))
    out = torch.empty(224 * 224 * 3, dtype=torch.uint8, device="cuda")
    outs = (ctypes.c_void_p * 1)(out.data_ptr())
    assert N.lib().tsvpp_convert_rois(vpp._ctx, 1, fr, 1, roi, ctypes.byref(fp.parameters), outs, None) == -3
    fr[0].uv = dev[1].data_ptr()
    outs[0] = None
    assert N.lib().tsvpp_convert_rois(vpp._ctx, 1, fr, 1, roi, ctypes.byref(fp.parameters), outs, None) == -3
