"""GPU: tsvpp_convert_rois_p010 against tests/p010_util.py on the numpy slice of each box (the contract: output i is what the P010 letterbox call returns for a frame
that consists of box i alone, the rectangle equal to the canvas).  Raw bits throughout; FOUR = uint8 merged, fp32 planar, an fp16 ImageNet tensor, Y800 fp32."""
import os
import zlib

import numpy as np
import pytest
import torch

import p010_util as M
import tensor_util as T
from cpp_check import run_check, write_nv12
from p010_cases import BLACK, FLAVOURS, FOUR, convert, dev, frame, params, same, want

pytestmark = pytest.mark.gpu
INTERIOR = (6, 8, 42, 32)  # 36 x 24 at left = 6: 2 mod 4, so the chroma pair's dword alignment within a 16-byte chunk changes


def cut(fr, box):
    l, t, r, b = box
    return fr[0][t:b, l:r], fr[1][t // 2:b // 2, l:r]


def rois(vpp, frames, boxes, dst, mode, flavour, planes_dev=None):  # boxes: (frame, left, top, right, bottom)
    fp, kw = params(dst, mode, flavour)
    ys, uvs = planes_dev or ([dev(f[0]) for f in frames], [dev(f[1]) for f in frames])
    return vpp.convert_rois_p010(ys, uvs, boxes, fp, **kw)


def check(got, frames, boxes, dst, mode, flavour):
    torch.cuda.synchronize()
    for i, (k, l, t, r, b) in enumerate(boxes):
        same(got[i], want(cut(frames[k], (l, t, r, b)), (r - l, b - t), (0, 0, *dst), dst, mode, flavour, BLACK), f"box {i} {(k, l, t, r, b)} -> {dst} mode={mode} {flavour}")
    return got


def model_boxes(dst):  # the whole frame; 2 x 2 at the bottom-right corner (every tap clamps); the interior box; a box of the output's size (every weight is zero)
    return [(0, 0, 0, 72, 56), (0, 70, 54, 72, 56), (0, *INTERIOR), (0, 4, 10, 4 + dst[0], 10 + dst[1])]


@pytest.mark.parametrize("boxes,dst,mode,flavour", [(model_boxes(d), d, m, f) for d in [(32, 32), (66, 34)] for m in (M.NEAREST, M.BILINEAR) for f in FOUR]
                         + [([(0, *INTERIOR)], d, M.BILINEAR, f) for d in [(64, 64), (30, 34)] for f in sorted(FLAVOURS)])
def test_boxes_against_the_model(vpp, boxes, dst, mode, flavour):
    """one 72 x 56 frame at a pitch of 80 words.  The model's boxes to one tile and to three tile columns of which the last is the shifted one, four flavours;
    then every store with one box: to 64 x 64 (vector stores) and to 30 x 34, 4 k + 2 columns narrower than a tile (element-wise)"""
    fr = [frame(72, 56, 20, pitch=80)]
    check(rois(vpp, fr, boxes, dst, mode, flavour), fr, boxes, dst, mode, flavour)


@pytest.mark.parametrize("flavour", FOUR)
def test_equals_the_letterbox_call_on_the_box_alone(vpp, flavour):
    fr, dst = frame(72, 56, 21, pitch=80), (48, 40)
    a = rois(vpp, [fr], [(0, *INTERIOR)], dst, M.BILINEAR, flavour)
    b, _ = convert(vpp, [tuple(np.ascontiguousarray(p) for p in cut(fr, INTERIOR))], [(36, 24)], dst, M.BILINEAR, flavour, rects=[(0, 0, *dst)])
    torch.cuda.synchronize()
    assert np.array_equal(T.bits(a[0]), T.bits(b[0]))


@pytest.mark.parametrize("flavour", FOUR)
@pytest.mark.parametrize("mode", [M.NEAREST, M.BILINEAR])
def test_nothing_outside_the_box_matters(vpp, mode, flavour):
    """per box a frame that is 0xFFFF outside the box and in the pitch padding, with random low six bits: what a wrong origin or a clamp to the frame fails"""
    dst, clean, rng, dirty = (66, 34), frame(72, 56, 22, pitch=80), np.random.default_rng(23), []
    boxes = model_boxes(dst)
    for _, l, t, r, b in boxes:
        y, uv = np.full((56, 80), 0xFFFF, np.uint16), np.full((28, 80), 0xFFFF, np.uint16)
        y[t:b, l:r] = (clean[0][t:b, l:r] & 0xFFC0) | rng.integers(0, 64, (b - t, r - l), dtype=np.uint16)
        uv[t // 2:b // 2, l:r] = (clean[1][t // 2:b // 2, l:r] & 0xFFC0) | rng.integers(0, 64, ((b - t) // 2, r - l), dtype=np.uint16)
        dirty.append((y, uv))
    a = check(rois(vpp, [clean], boxes, dst, mode, flavour), [clean], boxes, dst, mode, flavour)
    b = rois(vpp, dirty, [(k, *bx[1:]) for k, bx in enumerate(boxes)], dst, mode, flavour)
    torch.cuda.synchronize()
    assert np.array_equal(T.bits(a), T.bits(b))


@pytest.mark.parametrize("flavour", FOUR)
def test_staged_and_gathered_tiles_in_one_launch(vpp, flavour):
    """48 x 48 and 64 x 96 stage; 416 x 416 to the same 32 x 32 exceeds the launch's LDS and gathers"""
    import tensor_stream as ts
    fr, boxes = [frame(416, 416, 30)], [(0, 8, 16, 56, 64), (0, 100, 40, 164, 136), (0, 0, 0, 416, 416)]
    fp, kw = params((32, 32), M.BILINEAR, flavour)
    d = ts.describe_rois_p010(fp, [(416, 416)], boxes, **kw)
    assert d["staged"] == 2 and d["src"] == "p010" and "staged" in d["kernel"], d
    check(rois(vpp, fr, boxes, (32, 32), M.BILINEAR, flavour), fr, boxes, (32, 32), M.BILINEAR, flavour)


@pytest.mark.parametrize("flavour", ["f32_planar", "u8_merged"])
def test_unaligned_chroma_pairs(vpp, flavour):
    """a chroma plane at an address 2 mod 4 (a view one word into an allocation) under an even pitch and an even left: the two-halfword path"""
    fr, boxes = frame(72, 56, 61, pitch=80), [(0, *INTERIOR), (0, 0, 0, 72, 56)]
    uv = dev(np.concatenate([np.full(1, 0xFFFF, np.uint16), fr[1].ravel()])).as_strided((28, 72), (80, 1), 1)
    assert uv.data_ptr() % 4 == 2
    check(rois(vpp, [fr], boxes, (66, 34), M.BILINEAR, flavour, planes_dev=([dev(fr[0])], [uv])), [fr], boxes, (66, 34), M.BILINEAR, flavour)


def test_capture_replay_and_the_split_at_64_boxes(vpp):
    """65 boxes of 4 x 4 out of three frames (two launches) captured into a graph and replayed after the source planes changed"""
    first, second = [frame(16, 12, 50 + k) for k in range(3)], [frame(16, 12, 150 + k) for k in range(3)]
    boxes = [(k % 3, 2 * (k % 7), 2 * (k % 5), 2 * (k % 7) + 4, 2 * (k % 5) + 4) for k in range(65)]
    planes = ([dev(f[0]) for f in first], [dev(f[1]) for f in first])
    rois(vpp, first, boxes, (8, 8), M.BILINEAR, "f32_planar", planes)  # (a first call outside the capture; torch.cuda.graph synchronises on entry)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = rois(vpp, first, boxes, (8, 8), M.BILINEAR, "f32_planar", planes)
    for k, f in enumerate(second):
        planes[0][k].copy_(dev(f[0])), planes[1][k].copy_(dev(f[1]))
    for _ in range(2):  # (a second replay finds what only the first one after the capture gets right)
        got.zero_()
        g.replay()
        check(got, second, boxes, (8, 8), M.BILINEAR, "f32_planar")


def test_check_program_crcs(tmp_path):
    """VideoProcessor::ConvertRoisP010 through its check program: the CRC-32 it prints per box is the model's"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tensor-stream_amd", "lib", "vpp_rois_p010")
    fr, dst, boxes = frame(128, 72, 70, pitch=192), (70, 66), [(0, 0, 128, 72), (6, 8, 42, 32), (126, 70, 128, 72)]
    write_nv12(tmp_path / "in.p010", *fr)
    for fcc, planes, norm in [(M.BGR24, M.PLANAR, True), (M.RGB24, M.MERGED, False)]:
        rc, lines, tails = run_check([exe, tmp_path / "in.p010", 128, 72, 2 * 192, *dst, M.BILINEAR, fcc, planes, int(norm), *[v for b in boxes for v in b]])
        assert rc == 0 and len(lines) == len(boxes), (rc, *tails)
        for (idx, crc, nbytes), (l, t, r, b) in zip(lines, boxes):
            ref = M.expected(*cut(fr, (l, t, r, b)), r - l, b - t, (0, 0, *dst), dst, M.BILINEAR, fcc, planes, norm, BLACK)
            assert int(nbytes) == ref.size and int(crc) == zlib.crc32(ref.tobytes()), f"box {idx} {(l, t, r, b)} -> {dst}"
