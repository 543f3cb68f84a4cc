"""GPU: tsvpp_convert_rois_area -- AREA resize of many boxes of one or several NV12 frames to one output size, in one launch per 64 boxes.

The contract is tsvpp_convert_rois's (include/tsvpp.h): the output of box (left, top, right, bottom) is, bit for bit, what the oracle returns for the SLICED planes

    ys  = y [top : bottom, left : right]
    uvs = uv[top // 2 : top // 2 + h // 2, left : right]      BYTE columns (an odd `left` swaps U and V, as the crop stage does)
    oracle.convert(ys, uvs, dst=(dw, dh), resize_type=AREA, ...)

and, for a box Convert's crop stage accepts, what tsvpp_convert(crop = box, AREA) returns.  A box with both ratios above 1 runs the AREA down-scale with weight rows
the kernel generates per tile, any other box the AREA up-scale rule.  Every comparison is np.array_equal on the raw bits."""
import ctypes
import math

import numpy as np
import pytest
import torch

from guard_util import arena
from util import knob_run, synth_nv12

pytestmark = pytest.mark.gpu

NEAREST, BILINEAR, BICUBIC, AREA = 0, 1, 2, 3
Y800, RGB24, BGR24 = 0, 1, 2
PLANAR, MERGED = 0, 1
LIMIT = 64     # TSVPP_MAX_ROIS_AREA
MAX_TAPS = 40  # ROI_AREA_MAX_TAPS
W, H, PITCH = 1920, 1080, 2048

FLAVOURS = [(fcc, planes, norm) for fcc in (RGB24, BGR24) for planes in (PLANAR, MERGED) for norm in (False, True)] + [(Y800, MERGED, False), (Y800, MERGED, True)]


def box_set(dw, dh):
    """tests/test_gpu_rois.py's boxes ..."""
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
    ] + [
        # ... plus the boxes behind the generator's scales: 448 (one row at 224), 336 (period 2), 300 (period 56: wraps inside the output and across a tile
        # boundary), 226 (two taps, the longest chain), 302, 500 (to 112: five taps), the full width and the full height (to 112: 18 and 10 taps)
        (10, 20, 458, 468),               # even corner
        (11, 21, 347, 357),               # odd corner
        (100, 31, 400, 331),              # odd top
        (501, 400, 727, 626),             # odd left
        (W - 302, 300, W, 602),           # at the right edge
        (700, H - 500, 1200, H),          # at the bottom edge
        (301, 111, 801, 611),             # 500, both odd
        (0, 200, W, 648),                 # full width
        (600, 0, 1100, H),                # full height
        (0, 0, W, H),                     # the frame
    ]


def is_down(box, dst):
    xr, yr = np.float32(box[2] - box[0]) / np.float32(dst[0]), np.float32(box[3] - box[1]) / np.float32(dst[1])
    return bool(xr > 1 and yr > 1), int(math.ceil(float(xr))), int(math.ceil(float(yr)))


def within_the_cap(boxes, dst):
    """the boxes the entry point accepts for this output size: a down-scale box above ROI_AREA_MAX_TAPS taps is refused (tests/test_rois_area_cpu.py)"""
    keep = []
    for b in boxes:
        down, tx, ty = is_down(b[-4:], dst)
        if not (down and max(tx, ty) > MAX_TAPS):
            keep.append(b)
    return keep


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


def expect(oracle, y, uv, box, dst, fcc, planes, norm):
    l, t, r, b = box
    w, h = r - l, b - t
    ys = y[t:b, l:l + w]
    uvs = uv[t // 2:t // 2 + h // 2, l:l + w]
    ref, _, _ = oracle.convert(ys, uvs, dst=dst, resize_type=AREA, fourcc=fcc, planes=planes, normalization=norm, nthreads=8)
    return ref.view(np.uint8).ravel()


def bits(t):
    return t.contiguous().cpu().numpy().ravel().view(np.uint8)


def params(ts, dst, fcc, planes, norm, crop=(0, 0, 0, 0), rt=AREA):
    return ts.FrameParameters(width=dst[0], height=dst[1], crop_coords=crop, resize_type=rt, pixel_format=fcc, planes_pos=planes, normalization=norm)


def check_rois(v, oracle, frames_host, frames_dev, boxes, dst, fcc, planes, norm, widths=None, out=None, what=""):
    """convert the boxes, compare every one with the oracle on its sliced planes; returns the output"""
    import tensor_stream as ts
    fp = params(ts, dst, fcc, planes, norm)
    got = v.convert_rois_area([f[0] for f in frames_dev], [f[1] for f in frames_dev], boxes, fp, out=out, width=widths)
    torch.cuda.synchronize()
    for i, b in enumerate(boxes):
        b5 = b if len(b) == 5 else (0,) + tuple(b)
        y, uv = frames_host[b5[0]]
        ref = expect(oracle, y, uv, b5[1:], dst, fcc, planes, norm)
        g = bits(got[i])
        assert g.size == ref.size, (what, i, b, g.size, ref.size)
        bad = np.flatnonzero(g != ref)
        assert bad.size == 0, f"{what} box {i} {b} -> {dst} fcc={fcc} planes={planes} norm={norm}: {bad.size} bytes differ, first at {bad[:4]}"
    return got


@pytest.fixture(scope="module")
def frame():
    y, uv = synth_nv12(W, H, seed=2024, pitch=PITCH)
    return (y, uv), (torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda())


@pytest.mark.parametrize("dst", [(224, 224), (112, 112), (250, 250), (30, 30)])
@pytest.mark.parametrize("fcc,planes,norm", FLAVOURS)
def test_box_set_matches_the_oracle_and_the_crop_path(vpp, oracle, frame, fcc, planes, norm, dst):
    import tensor_stream as ts
    host, dev = frame
    boxes = within_the_cap(box_set(*dst), dst)
    assert len(boxes) >= len(box_set(*dst)) - (4 if dst == (30, 30) else 0)  # 30 columns: the four boxes 1920 wide with yr > 1 need 64 taps
    d = ts.describe_rois_area(params(ts, dst, fcc, planes, norm), (W, H, PITCH), boxes)
    assert d["down"] == sum(is_down(b, dst)[0] for b in boxes) and 0 < d["down"] < len(boxes)  # both rules in one launch
    got = check_rois(vpp, oracle, [host], [dev], boxes, dst, fcc, planes, norm, widths=W)
    # the two paths of the library agree: every box Convert's crop stage accepts, through tsvpp_convert(crop = box, AREA)
    cropped = 0
    for i, (l, t, r, b) in enumerate(boxes):
        if r - l < W and b - t < H:
            one = vpp.Convert(dev[0], dev[1], params(ts, dst, fcc, planes, norm, crop=(l, t, r, b)), width=W)
            torch.cuda.synchronize()
            assert np.array_equal(bits(one), bits(got[i])), f"box {i} {(l, t, r, b)}: tsvpp_convert(crop, AREA) and tsvpp_convert_rois_area differ"
            cropped += 1
    assert cropped == sum(1 for (l, t, r, b) in boxes if r - l < W and b - t < H) >= len(boxes) - 5


def test_a_box_of_the_output_size_is_the_plain_colour_conversion(vpp, oracle, frame):
    """the AREA up-scale rule at ratio 1: every weight is zero"""
    import tensor_stream as ts
    host, dev = frame
    boxes = [(400, 300, 624, 524), (401, 301, 625, 525)]
    out = check_rois(vpp, oracle, [host], [dev], boxes, (224, 224), RGB24, MERGED, False, widths=W)
    plain = vpp.Convert(dev[0], dev[1], params(ts, (0, 0), RGB24, MERGED, False, crop=boxes[0], rt=NEAREST), width=W)
    torch.cuda.synchronize()
    assert np.array_equal(bits(plain), bits(out[0]))


@pytest.mark.parametrize("n", [1, LIMIT, LIMIT + 1, 3 * LIMIT + 5])
@pytest.mark.parametrize("fcc,planes,norm", [(BGR24, PLANAR, True), (RGB24, MERGED, False)])
def test_splitting_over_launches(vpp, oracle, frame, n, fcc, planes, norm):
    import tensor_stream as ts
    host, dev = frame
    boxes = seeded_boxes(n, seed=1000 + n, frames=[(W, H)])
    d = ts.describe_rois_area(params(ts, (112, 112), fcc, planes, norm), (W, H, PITCH), boxes)
    assert d["launches"] == math.ceil(n / LIMIT) and d["limit"] == LIMIT
    check_rois(vpp, oracle, [host], [dev], boxes, (112, 112), fcc, planes, norm, widths=W, what=f"n={n}")


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
    for fcc, planes, norm, dst in [(RGB24, PLANAR, False, (112, 112)), (BGR24, MERGED, True, (224, 224)), (Y800, MERGED, False, (112, 112))]:
        check_rois(vpp, oracle, host, dev, boxes, dst, fcc, planes, norm, widths=widths, what=f"{n_frames} frames")


@pytest.mark.parametrize("dst", [(250, 250), (30, 30)])
@pytest.mark.parametrize("fcc,planes,norm", [(BGR24, PLANAR, True), (RGB24, MERGED, True), (RGB24, MERGED, False), (BGR24, PLANAR, False), (Y800, MERGED, False)])
@pytest.mark.parametrize("off", [0, 4])
def test_unaligned_outputs_and_guard_bytes(vpp, oracle, frame, fcc, planes, norm, off, dst):
    """outputs 0 / 4 bytes past a 16-byte boundary (vector-store and element-wise kernels); the bytes before and after every output stay as they were"""
    import tensor_stream as ts
    host, dev = frame
    boxes = within_the_cap(box_set(*dst), dst)[:8] + within_the_cap(box_set(*dst), dst)[16:20] + [b[1:] for b in seeded_boxes(3, seed=dst[0] + off, frames=[(W, H)])]
    n = len(boxes)
    nbytes = (1 if fcc == Y800 else 3) * dst[0] * dst[1] * (4 if norm else 1)
    _, slots, verify = arena([nbytes] * n, off, what="output", where=f"dst {dst}")
    out = [s.view(torch.float32) if norm else s for s in slots]
    check_rois(vpp, oracle, [host], [dev], boxes, dst, fcc, planes, norm, widths=W, out=out, what=f"offset {off}")
    verify()
    if not knob_run():
        d = ts.describe_rois_area(params(ts, dst, fcc, planes, norm), (W, H, PITCH), boxes, aligned_outputs=(off == 0))
        assert d["kernel"].split(",")[1] == ("vec" if off == 0 and not (dst[0] % 4 != 0 and dst[0] < 32) else "elem")
        assert d["tail"] == (2 if (off == 0 and dst[0] == 250) else 0)


def test_staged_and_gather_paths(oracle, frame, monkeypatch):
    """the LDS budget decides per box: with none (TSVPP_LDS_KB=0, read when a context is created) every box gathers from global memory -- same bits; the weight
    rows stay in LDS either way"""
    import tensor_stream as ts
    host, dev = frame
    boxes = box_set(224, 224)
    cases = [(BGR24, PLANAR, True), (RGB24, MERGED, False), (Y800, MERGED, False)]
    for kb in (None, "0"):
        if kb is not None:
            monkeypatch.setenv("TSVPP_LDS_KB", kb)
        v = ts.VideoProcessor(device=0, max_consumers=1)
        try:
            for fcc, planes, norm in cases:
                if not knob_run(("TSVPP_LDS_KB",)):
                    d = ts.describe_rois_area(params(ts, (224, 224), fcc, planes, norm), (W, H, PITCH), boxes)
                    if kb is None:
                        assert d["kernel"].endswith("staged>") and d["staged"] >= len(boxes) - 3 and d["lds"] > 0
                    else:
                        assert d["kernel"].endswith("gather>") and d["staged"] == 0 and d["lds"] > 0
                check_rois(v, oracle, [host], [dev], boxes, (224, 224), fcc, planes, norm, widths=W, what=f"TSVPP_LDS_KB={kb}")
        finally:
            v.Close()


def test_a_launch_mixes_staged_and_gathering_boxes(vpp, oracle, frame):
    """a box whose tiles outgrow the LDS budget (1920 x 1080 -> 112 x 112: a tile taps 566 x 318 luma bytes) beside small ones, in one launch"""
    import tensor_stream as ts
    host, dev = frame
    boxes = [(0, 0, W, H), (100, 100, 300, 300), (0, 0, W, 540), (7, 9, 71, 73)]
    if not knob_run():
        d = ts.describe_rois_area(params(ts, (112, 112), RGB24, PLANAR, True), (W, H, PITCH), boxes)
        assert d["kernel"].endswith("staged>") and 0 < d["staged"] < len(boxes) and d["taps"] == "18x10"
    check_rois(vpp, oracle, [host], [dev], boxes, (112, 112), RGB24, PLANAR, True, widths=W)
    check_rois(vpp, oracle, [host], [dev], boxes, (112, 112), BGR24, MERGED, False, widths=W)


def test_graph_capture_replays_bit_exact_and_nothing_is_cached(vpp, oracle):
    """records in the kernarg segment, weight rows generated in the kernel: the call allocates, copies and synchronises nothing, so it is legal during capture even
    with scales its context has never seen, and leaves no table behind -- where the same boxes through Convert(crop, AREA) leave their tables in the context"""
    import tensor_stream as ts
    from tensor_stream import _native as N
    a, b = synth_nv12(1280, 720, seed=301), synth_nv12(1280, 720, seed=302)
    dy, duv = torch.from_numpy(a[0]).cuda(), torch.from_numpy(a[1]).cuda()
    boxes = seeded_boxes(LIMIT + 6, seed=12, frames=[(1280, 720)])  # two launches
    fp = params(ts, (112, 112), RGB24, MERGED, False)
    out = vpp._alloc(fp.parameters, 112, 112, len(boxes))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        vpp.convert_rois_area(dy, duv, boxes, fp, out=out)  # warm-up outside capture, through ANOTHER context (the kernel's code object is loaded once per process)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    v = ts.VideoProcessor(device=0, max_consumers=1)  # a fresh context: no scale has been seen
    try:
        assert N.lib().tsvpp_debug_area_tables(v._ctx) == 0 and v.trim() == 0
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            v.convert_rois_area(dy, duv, boxes, fp, out=out)
        for src in (a, b):  # replayed twice, on whatever the frame holds at replay time
            dy.copy_(torch.from_numpy(src[0]).cuda())
            duv.copy_(torch.from_numpy(src[1]).cuda())
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            for i, bx in enumerate(boxes):
                assert np.array_equal(bits(out[i]), expect(oracle, src[0], src[1], bx[1:], (112, 112), RGB24, MERGED, False)), (i, bx)
        assert N.lib().tsvpp_debug_area_tables(v._ctx) == 0 and v.trim() == 0
        # the same conversion, one Convert per box: its tables stay in the context
        down = [bx for bx in boxes if is_down(bx[1:], (112, 112))[0] and bx[3] - bx[1] < 1280 and bx[4] - bx[2] < 720][:3]
        assert len(down) == 3
        for bx in down:
            one = v.Convert(dy, duv, params(ts, (112, 112), RGB24, MERGED, False, crop=bx[1:]))
            torch.cuda.synchronize()
            assert np.array_equal(bits(one), bits(out[boxes.index(bx)]))
        assert N.lib().tsvpp_debug_area_tables(v._ctx) >= 2
    finally:
        v.Close()


def test_status_codes_with_a_live_context(vpp, frame):
    """the validation of tests/test_rois_area_cpu.py answers before any launch"""
    import tensor_stream as ts
    from tensor_stream import _native as N
    host, dev = frame
    fp = params(ts, (224, 224), RGB24, MERGED, False)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_rois_area(dev[0], dev[1], [(0, 0, 2000, 100)], fp, width=W)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_rois_area(dev[0], dev[1], [(0, 0, 101, 100)], fp, width=W)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_rois_area(dev[0], dev[1], [(0, 0, 100, 100)], params(ts, (224, 224), RGB24, MERGED, False, rt=BILINEAR), width=W)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_rois_area(dev[0], dev[1], [(0, 0, W, H)], params(ts, (30, 30), RGB24, MERGED, False), width=W)  # 64 taps
    fr = (N.NV12 * 1)(N.NV12(dev[0].data_ptr(), None, PITCH, PITCH, W, H))
    roi = (N.Roi * 1)(N.Roi(0, 0, 0, 64, 64))
    out = torch.empty(224 * 224 * 3, dtype=torch.uint8, device="cuda")
    outs = (ctypes.c_void_p * 1)(out.data_ptr())
    assert N.lib().tsvpp_convert_rois_area(vpp._ctx, 1, fr, 1, roi, ctypes.byref(fp.parameters), outs, None) == -3
