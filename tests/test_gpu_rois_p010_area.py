"""GPU: tsvpp_convert_rois_p010_area against tests/p010_area_util.box, the int64 restatement of the box filter, on the numpy slice of each box.  Raw bits
throughout, no tolerance; FOUR = uint8 merged, fp32 planar, an fp16 ImageNet tensor, Y800 fp32."""
import numpy as np
import pytest
import torch

import p010_util as M
import tensor_util as T
from p010_area_util import AREA, box
from p010_cases import FLAVOURS, FOUR, dev, frame, params, same, stored

pytestmark = pytest.mark.gpu
INTERIOR = (6, 8, 42, 32)  # 36 x 24 at left = 6: 2 mod 4, so the chroma pair's dword alignment within a 16-byte chunk changes
TWO = ["f32_planar", "u8_merged"]


def cut(fr, bx):
    l, t, r, b = bx
    return fr[0][t:b, l:r], fr[1][t // 2:b // 2, l:r]


def want(box_planes, dst, flavour):
    """the raw bytes of one box's output in a flavour of p010_cases.FLAVOURS"""
    Ys, UVs = M.samples(box_planes[0]), M.samples(box_planes[1])
    U, V = (box(UVs[:, c::2], dst[0] // 2, dst[1] // 2) for c in (0, 1))
    return stored(M.channels(box(Ys, *dst), U, V, FLAVOURS[flavour][0]), flavour)


def rois(vpp, frames, boxes, dst, flavour, planes_dev=None):  # boxes: (frame, left, top, right, bottom)
    fp, kw = params(dst, AREA, flavour)
    ys, uvs = planes_dev or ([dev(f[0]) for f in frames], [dev(f[1]) for f in frames])
    return vpp.convert_rois_p010_area(ys, uvs, boxes, fp, **kw)


def check(got, frames, boxes, dst, flavour):
    torch.cuda.synchronize()
    for i, (k, *bx) in enumerate(boxes):
        same(got[i], want(cut(frames[k], bx), dst, flavour), f"box {i} {(k, *bx)} -> {dst} {flavour}")
    return got


def model_boxes(dst):  # the whole frame; 2 x 2 at the bottom-right corner (16-fold up: one tap); the interior box; a box of the output's size (the identity)
    return [(0, 0, 0, 72, 56), (0, 70, 54, 72, 56), (0, *INTERIOR), (0, 4, 10, 4 + dst[0], 10 + dst[1])]


def checkerboard(h, pitch):
    """0 / 1023 in blocks of 3 samples (chroma: of 3 pairs, V the inverse of U), random low six bits: saturated sums"""
    y, x = np.mgrid[0:h, 0:pitch]
    low = np.random.default_rng(7).integers(0, 64, (h + h // 2, pitch), dtype=np.uint16)
    luma = ((((x // 3 + y // 3) & 1) * 1023) << 6).astype(np.uint16) | low[:h]
    y, x = np.mgrid[0:h // 2, 0:pitch]
    chroma = ((((x // 6 + y // 3 + x) & 1) * 1023) << 6).astype(np.uint16) | low[h:]
    return luma, chroma


@pytest.mark.parametrize("boxes,dst,flavour", [(model_boxes(d), d, f) for d in [(32, 32), (66, 34)] for f in FOUR]
                         + [([(0, 0, 0, 72, 56)], d, f) for d in [(64, 48), (30, 34)] for f in sorted(FLAVOURS)])
def test_boxes_against_the_model(vpp, boxes, dst, flavour):
    """one 72 x 56 frame at a pitch of 80 words.  The model's boxes to one tile and to three tile columns of which the last is the shifted one, four flavours;
    then every store with the whole frame: to 64 x 48 (vector stores) and to 30 x 34, 4 k + 2 columns narrower than a tile (element-wise)"""
    fr = [frame(72, 56, 20, pitch=80)]
    check(rois(vpp, fr, boxes, dst, flavour), fr, boxes, dst, flavour)


# exact 2; exact 3; 3 : 2 (weights 2, 1 / 1, 2); down in x and up in y; 16 aligned taps; 17 taps on both planes ((16 - 2 + 253) / 16 + 1, (8 - 1 + 126) / 8 + 1)
RATIOS = [((64, 48), (32, 24)), ((96, 72), (32, 24)), ((48, 36), (32, 24)), ((96, 20), (32, 40)), ((512, 512), (32, 32)), ((254, 254), (16, 16))]


@pytest.mark.parametrize("flavour", TWO)
@pytest.mark.parametrize("src,dst,board", [(*r, False) for r in RATIOS] + [(*RATIOS[1], True), (*RATIOS[2], True)])
def test_ratios(vpp, src, dst, board, flavour):
    """seeded words in a box inset at (4, 2), and through two of the ratios the checkerboard: saturated sums on the device"""
    import tensor_stream as ts
    w, h = src[0] + 8, src[1] + 4
    fr, boxes = [checkerboard(h, w + 8) if board else frame(w, h, 31, pitch=w + 8)], [(0, 4, 2, 4 + src[0], 2 + src[1])]
    if src == (254, 254):  # the walk must wrap its two buffers: at least three bands
        fp, kw = params(dst, AREA, flavour)
        d = ts.describe_rois_p010_area(fp, [(w, h, 2 * (w + 8))], boxes, **kw)
        assert d["staged"] == 1 and d["taps"] == "17x17" and 3 * int(d["band"]) <= 254, d
    check(rois(vpp, fr, boxes, dst, flavour), fr, boxes, dst, flavour)


@pytest.mark.parametrize("flavour", TWO)
def test_frames_of_two_sizes_in_one_launch(vpp, flavour):
    """a 16 x 12 box and the interior box of the small frame beside 254 x 254 out of a 262 x 258 frame, all to 16 x 16: footprints 12 to 254 words wide walk
    through band buffers sized for the widest"""
    fr = [frame(72, 56, 41, pitch=80), frame(262, 258, 42, pitch=270)]
    boxes = [(0, 2, 4, 18, 16), (0, *INTERIOR), (1, 4, 2, 258, 256)]
    check(rois(vpp, fr, boxes, (16, 16), flavour), fr, boxes, (16, 16), flavour)


@pytest.mark.parametrize("flavour", FOUR)
def test_nothing_outside_the_box_matters(vpp, flavour):
    """per box a frame that is 0xFFFF outside the box and in the pitch padding, with random low six bits: what a wrong origin or a clamp to the frame fails"""
    dst, clean, rng, dirty = (66, 34), frame(72, 56, 22, pitch=80), np.random.default_rng(23), []
    boxes = model_boxes(dst)
    for _, l, t, r, b in boxes:
        y, uv = np.full((56, 80), 0xFFFF, np.uint16), np.full((28, 80), 0xFFFF, np.uint16)
        y[t:b, l:r] = (clean[0][t:b, l:r] & 0xFFC0) | rng.integers(0, 64, (b - t, r - l), dtype=np.uint16)
        uv[t // 2:b // 2, l:r] = (clean[1][t // 2:b // 2, l:r] & 0xFFC0) | rng.integers(0, 64, ((b - t) // 2, r - l), dtype=np.uint16)
        dirty.append((y, uv))
    a = check(rois(vpp, [clean], boxes, dst, flavour), [clean], boxes, dst, flavour)
    b = rois(vpp, dirty, [(k, *bx[1:]) for k, bx in enumerate(boxes)], dst, flavour)
    torch.cuda.synchronize()
    assert np.array_equal(T.bits(a), T.bits(b))


@pytest.mark.parametrize("flavour", TWO)
def test_unaligned_chroma_pairs(vpp, flavour):
    """a chroma plane at an address 2 mod 4 (a view one word into an allocation) under an even pitch and an even left: the two-halfword path"""
    fr, boxes = frame(72, 56, 61, pitch=80), [(0, *INTERIOR), (0, 0, 0, 72, 56)]
    uv = dev(np.concatenate([np.full(1, 0xFFFF, np.uint16), fr[1].ravel()])).as_strided((28, 72), (80, 1), 1)
    assert uv.data_ptr() % 4 == 2
    check(rois(vpp, [fr], boxes, (34, 18), flavour, planes_dev=([dev(fr[0])], [uv])), [fr], boxes, (34, 18), flavour)


def test_capture_replay_and_the_split_at_64_boxes(vpp):
    """65 boxes of 12 x 10 out of three 16 x 12 frames (two launches) captured into a graph and replayed twice after the source planes changed"""
    first, second = [frame(16, 12, 50 + k) for k in range(3)], [frame(16, 12, 150 + k) for k in range(3)]
    boxes = [(k % 3, 2 * (k % 3), 2 * (k % 2), 2 * (k % 3) + 12, 2 * (k % 2) + 10) for k in range(65)]
    planes = ([dev(f[0]) for f in first], [dev(f[1]) for f in first])
    rois(vpp, first, boxes, (8, 8), "f32_planar", planes)  # (a first call outside the capture; torch.cuda.graph synchronises on entry)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = rois(vpp, first, boxes, (8, 8), "f32_planar", planes)
    for k, f in enumerate(second):
        planes[0][k].copy_(dev(f[0])), planes[1][k].copy_(dev(f[1]))
    for _ in range(2):  # (a second replay finds what only the first one after the capture gets right)
        got.zero_()
        g.replay()
        check(got, second, boxes, (8, 8), "f32_planar")
