"""GPU: tsvpp_convert_rois_sized -- many boxes, each resized to ITS OWN output size, in one launch per 48 boxes of a store class.

The contract (include/tsvpp.h): output i is, bit for bit, what tsvpp_convert_rois returns for box i alone at box i's size, i.e. oracle.convert on the box's sliced
planes with dst = that size (tests/test_gpu_rois.py: expect).  Every comparison is np.array_equal on raw bytes against the oracle; the library itself is the
yardstick only where a test says so.  Every call writes into the slots of one poisoned buffer with 64 guard bytes around each output (rois_sized_util.run), and
every byte outside the slots must be unchanged.  The shapes are the smallest at which the kernel's per-box output side can go wrong: 2 x 2, narrow tails, exactly a
tile, 4 k + 2 above a tile, tails on either axis, strips -- in ONE launch (rois_sized_util.SIZES)."""
import numpy as np
import pytest
import torch

import rois_sized_util as U
from rois_sized_util import BGR24, BICUBIC, BILINEAR, BOXES, FLAVOURS, FRAMES, LIMIT, MERGED, NEAREST, PLANAR, RGB24, SIZES
from util import knob_run, synth_nv12

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def frames():
    host = U.host_frames()
    return host, U.device_frames(host)


def refs(oracle, host, boxes, sizes, rt, fcc, planes, norm, key="fixed"):
    return [U.expect(oracle, host, b, s, rt, fcc, planes, norm, key=key) for b, s in zip(boxes, sizes)]


def esz(norm):
    return 4 if norm else 1


@pytest.mark.parametrize("fcc,planes,norm", FLAVOURS)
@pytest.mark.parametrize("rt", [NEAREST, BILINEAR, BICUBIC])
def test_twelve_sizes_in_one_launch_match_the_oracle_and_convert_rois(vpp, oracle, frames, rt, fcc, planes, norm):
    import tensor_stream as ts
    host, dev = frames
    fp = U.frame_parameters(ts, rt, fcc, planes, norm)
    outs = U.run(vpp, dev, BOXES, SIZES, fp, fcc, esz(norm), what=f"rt={rt} {fcc, planes, norm}")
    U.compare(outs, refs(oracle, host, BOXES, SIZES, rt, fcc, planes, norm), BOXES, SIZES, f"rt={rt} flavour {fcc, planes, norm}")
    # library against library: convert_rois, called once per distinct size, returns the same bytes
    for i, (b, s) in enumerate(zip(BOXES, SIZES)):
        one = vpp.convert_rois([d[0] for d in dev], [d[1] for d in dev], [b], U.frame_parameters(ts, rt, fcc, planes, norm, dst=s), width=[f[0] for f in FRAMES],
                               height=[f[1] for f in FRAMES])
        torch.cuda.synchronize()
        assert np.array_equal(one[0].cpu().numpy().ravel().view(np.uint8), outs[i]), f"box {i} {b} -> {s}: convert_rois and convert_rois_sized differ"
    if not knob_run():
        d = ts.describe_rois_sized(fp, FRAMES, BOXES, SIZES)
        assert d["launches"] == 2 and d["vec"] == 9 and d["grid"] == sum(U.tiles(w, h) for w, h in SIZES if not U.narrow_tail(w))


@pytest.mark.parametrize("order", ["reversed", "rotated"])
@pytest.mark.parametrize("rt,fcc,planes,norm", [(BILINEAR, RGB24, MERGED, False), (BICUBIC, BGR24, PLANAR, True), (NEAREST, U.Y800, MERGED, False)])
def test_the_order_of_the_boxes_does_not_change_an_output(vpp, oracle, frames, order, rt, fcc, planes, norm):
    """the box list reversed, and rotated by 5: every output has the bytes it had in its first place -- a wrong prefix sum or a record read at the wrong index shows"""
    import tensor_stream as ts
    host, dev = frames
    idx = list(range(len(BOXES)))[::-1] if order == "reversed" else [(i + 5) % len(BOXES) for i in range(len(BOXES))]
    boxes, sizes = [BOXES[i] for i in idx], [SIZES[i] for i in idx]
    outs = U.run(vpp, dev, boxes, sizes, U.frame_parameters(ts, rt, fcc, planes, norm), fcc, esz(norm), what=order)
    U.compare(outs, refs(oracle, host, boxes, sizes, rt, fcc, planes, norm), boxes, sizes, order)


@pytest.mark.parametrize("n", [LIMIT - 1, LIMIT, LIMIT + 1, 2 * LIMIT + 1])
@pytest.mark.parametrize("fcc,planes,norm", [(RGB24, MERGED, False), (BGR24, PLANAR, True)])
def test_chunk_boundaries(vpp, oracle, frames, n, fcc, planes, norm):
    """47, 48, 49 and 97 boxes from both frames with even sizes 2 .. 34: the launches of each store class end where they should"""
    import tensor_stream as ts
    host, dev = frames
    _, rois = U.seeded_request(7000 + n, n=n, max_side=34, frames=FRAMES)
    boxes, sizes = [r[:5] for r in rois], [r[5:] for r in rois]
    assert {b[0] for b in boxes} == {0, 1} and min(min(s) for s in sizes) == 2 and max(max(s) for s in sizes) == 34
    fp = U.frame_parameters(ts, BILINEAR, fcc, planes, norm)
    outs = U.run(vpp, dev, boxes, sizes, fp, fcc, esz(norm), what=f"n={n}")
    U.compare(outs, refs(oracle, host, boxes, sizes, BILINEAR, fcc, planes, norm, key=None), boxes, sizes, f"n={n}")
    if not knob_run():
        n_vec = sum(not U.narrow_tail(s[0]) for s in sizes)
        d = ts.describe_rois_sized(fp, FRAMES, boxes, sizes)
        assert d["vec"] == n_vec and d["launches"] == (n_vec + LIMIT - 1) // LIMIT + (n - n_vec + LIMIT - 1) // LIMIT


@pytest.mark.parametrize("placement", ["aligned", "unaligned", "alternating"])
@pytest.mark.parametrize("rt,fcc,planes,norm", [(BILINEAR, RGB24, MERGED, False), (BICUBIC, BGR24, PLANAR, True), (BILINEAR, RGB24, MERGED, True),
                                                (NEAREST, BGR24, PLANAR, False), (BILINEAR, U.Y800, MERGED, True)])
def test_output_placement_splits_the_call_by_store_class(vpp, oracle, frames, placement, rt, fcc, planes, norm):
    """all outputs 16-byte aligned; all one element past a boundary (+ 4 bytes fp32, + 1 uint8); alternating -- the two-class split inside one call.  Same bits,
    guards intact"""
    import tensor_stream as ts
    host, dev = frames
    aligned = {"aligned": [True] * 12, "unaligned": [False] * 12, "alternating": [i % 2 == 0 for i in range(12)]}[placement]
    outs = U.run(vpp, dev, BOXES, SIZES, U.frame_parameters(ts, rt, fcc, planes, norm), fcc, esz(norm), aligned=aligned, what=placement)
    U.compare(outs, refs(oracle, host, BOXES, SIZES, rt, fcc, planes, norm), BOXES, SIZES, placement)


@pytest.mark.parametrize("kb", ["0", "3"])
def test_lds_budgets_give_the_same_bits(vpp, oracle, frames, monkeypatch, kb):
    """TSVPP_LDS_KB (read when a context is created) = 0: every tile gathers from global memory; = 3: launches mix staged and gathering tiles.  The same bits as
    under the default budget, and the oracle's"""
    import tensor_stream as ts
    host, dev = frames
    monkeypatch.setenv("TSVPP_LDS_KB", kb)
    v = ts.VideoProcessor(device=0, max_consumers=1)
    try:
        for rt, fcc, planes, norm in [(BILINEAR, BGR24, PLANAR, True), (BICUBIC, RGB24, MERGED, False), (NEAREST, U.Y800, MERGED, False), (BICUBIC, RGB24, MERGED, True)]:
            fp = U.frame_parameters(ts, rt, fcc, planes, norm)
            want = refs(oracle, host, BOXES, SIZES, rt, fcc, planes, norm)
            for aligned in (True, False):
                a = U.run(vpp, dev, BOXES, SIZES, fp, fcc, esz(norm), aligned=aligned, what="default budget")
                b = U.run(v, dev, BOXES, SIZES, fp, fcc, esz(norm), aligned=aligned, what=f"TSVPP_LDS_KB={kb}")
                U.compare(a, want, BOXES, SIZES, "default budget")
                U.compare(b, want, BOXES, SIZES, f"TSVPP_LDS_KB={kb}")
            if not knob_run(("TSVPP_LDS_KB",)):
                d = ts.describe_rois_sized(fp, FRAMES, BOXES, SIZES)
                if kb == "0":
                    assert d["kernel"].endswith("gather>") and d["staged"] == 0
                else:  # (3 KiB less the merged flavours' static LDS leaves the first launch nothing: its boxes gather, the narrow tails' launch stages)
                    assert 0 < d["staged"] < 12
    finally:
        v.Close()


W, H, PITCH = 1920, 1080, 2048


@pytest.mark.parametrize("rt,fcc,planes,norm", [(BILINEAR, BGR24, PLANAR, True), (NEAREST, RGB24, MERGED, False)])
def test_a_pyramid_of_a_1080p_frame(vpp, oracle, rt, fcc, planes, norm):
    """the full-size case: one frame to 960 x 540, 480 x 270, 240 x 134 and 120 x 66 in one call.  Every level equals convert_rois of the whole frame at that
    size; the two smallest levels are also checked against the oracle"""
    import tensor_stream as ts
    y, uv = synth_nv12(W, H, seed=2024, pitch=PITCH)
    dy, duv = torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()
    sizes = ts.pyramid_sizes(W, H, 5)[1:]
    assert sizes == [(960, 540), (480, 270), (240, 134), (120, 66)]
    boxes = [(0, 0, 0, W, H)] * len(sizes)
    fp = U.frame_parameters(ts, rt, fcc, planes, norm)
    outs = U.run(vpp, [(dy, duv)], boxes, sizes, fp, fcc, esz(norm), frames=[(W, H, PITCH)], what="pyramid")
    for i, s in enumerate(sizes):
        one = vpp.convert_rois(dy, duv, [boxes[i][1:]], U.frame_parameters(ts, rt, fcc, planes, norm, dst=s), width=W, height=H)
        torch.cuda.synchronize()
        assert np.array_equal(one[0].cpu().numpy().ravel().view(np.uint8), outs[i]), f"level {i + 1} {s}: convert_rois and convert_rois_sized differ"
    U.compare(outs[2:], [U.expect(oracle, [(y, uv)], boxes[i], sizes[i], rt, fcc, planes, norm) for i in (2, 3)], boxes[2:], sizes[2:], "pyramid")
    # without `out`: views into one allocation, each at a multiple of 256 bytes, of output_shape
    got = vpp.convert_rois_sized(dy, duv, [b[1:] for b in boxes], fp, sizes, width=W, height=H)
    torch.cuda.synchronize()
    assert isinstance(got, list) and len(got) == len(sizes)
    for i, (g, s) in enumerate(zip(got, sizes)):
        assert tuple(g.shape) == tuple(ts.output_shape(fp.parameters, *s)) and g.data_ptr() % 256 == 0 and g.is_contiguous()
        assert np.array_equal(g.cpu().numpy().ravel().view(np.uint8), outs[i])


def test_graph_capture_replays_on_the_new_frame(vpp, oracle):
    """the records travel in the kernarg segment: the call allocates, copies and synchronises nothing, is legal during capture (both store classes: two launches),
    and the graph replays the captured boxes on whatever the planes hold at replay time"""
    import tensor_stream as ts
    a, b = U.host_frames(seed=4300), U.host_frames(seed=4400)
    dev = U.device_frames(a)
    fcc, planes, norm, rt = RGB24, MERGED, False, BICUBIC
    fp = U.frame_parameters(ts, rt, fcc, planes, norm)
    nbytes = [3 * w * h for w, h in SIZES]
    starts, total = U.slot_starts(nbytes, [True] * 12, 1)
    buf = torch.zeros(total, dtype=torch.uint8, device="cuda")
    out = [buf[s:s + nb] for s, nb in zip(starts, nbytes)]
    args = ([d[0] for d in dev], [d[1] for d in dev], BOXES, fp, SIZES)
    kw = dict(out=out, width=[f[0] for f in FRAMES], height=[f[1] for f in FRAMES])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        vpp.convert_rois_sized(*args, **kw)  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        vpp.convert_rois_sized(*args, **kw)
    for (dy, duv), (y, uv) in zip(dev, b):
        dy.copy_(torch.from_numpy(y).cuda())
        duv.copy_(torch.from_numpy(uv).cuda())
    buf.zero_()
    g.replay()
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    U.compare([got[s:s + nb] for s, nb in zip(starts, nbytes)], [U.expect(oracle, b, bx, sz, rt, fcc, planes, norm) for bx, sz in zip(BOXES, SIZES)], BOXES, SIZES,
              "graph replay")


def test_status_codes_with_a_live_context(vpp, frames):
    """the validation of tests/test_rois_sized_cpu.py answers before any launch; a null plane or output is TSVPP_ERROR"""
    import ctypes

    import tensor_stream as ts
    from tensor_stream import _native as N
    host, dev = frames
    ys, uvs = [d[0] for d in dev], [d[1] for d in dev]
    kw = dict(width=[f[0] for f in FRAMES], height=[f[1] for f in FRAMES])
    fp = U.frame_parameters(ts, BILINEAR, RGB24, MERGED, False)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_rois_sized(ys, uvs, [(0, 0, 0, 400, 100)], fp, [(32, 32)], **kw)
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_rois_sized(ys, uvs, [(0, 0, 0, 64, 64)], U.frame_parameters(ts, BILINEAR, RGB24, MERGED, False, dst=(32, 32)), [(32, 32)], **kw)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_rois_sized(ys, uvs, [(0, 0, 0, 64, 64)], fp, [(33, 32)], **kw)
    with pytest.raises(RuntimeError, match="-2"):
        vpp.convert_rois_sized(ys, uvs, [(0, 0, 0, 64, 64)], U.frame_parameters(ts, U.AREA, RGB24, MERGED, False), [(32, 32)], **kw)
    fr = (N.NV12 * 1)(N.NV12(ys[0].data_ptr(), None, 328, 328, 320, 180))
    roi = (N.RoiSized * 1)(N.RoiSized(0, 0, 0, 64, 64, 32, 32))
    out = torch.empty(32 * 32 * 3, dtype=torch.uint8, device="cuda")
    outs = (ctypes.c_void_p * 1)(out.data_ptr())
    assert N.lib().tsvpp_convert_rois_sized(vpp._ctx, 1, fr, 1, roi, ctypes.byref(fp.parameters), outs, None) == -3
    fr[0].uv = uvs[0].data_ptr()
    outs[0] = None
    assert N.lib().tsvpp_convert_rois_sized(vpp._ctx, 1, fr, 1, roi, ctypes.byref(fp.parameters), outs, None) == -3
