"""GPU: tsvpp_convert_letterbox_p010 -- 10-bit P010 frames into letterboxed canvases in one launch -- against tests/p010_util.py, the numpy restatement of the
contract of include/tsvpp.h.  Every comparison is on raw bits.  The flavours: uint8 merged, fp32 planar, an fp16 tensor with ImageNet mean / std, Y800 fp32."""
import os
import zlib

import numpy as np
import pytest
import torch

import p010_util as M
import tensor_util as T
from cpp_check import run_check, write_nv12
from letterbox_util import default_rect
from p010_cases import BLACK, FLAVOURS, FOUR, check, convert, dev, frame, want

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("flavour,chroma", [("y800_f32", 512), ("y800_u8", 512), ("y800_f16", 512)] + [(f, c) for f in FOUR[:3] for c in (512, 0, 1023)])
def test_all_1024_codes(vpp, flavour, chroma):
    """a 32 x 32 frame whose luma is the ramp 0..1023 with arbitrary low bits, no resize: every quotient k / 1023 and every byte; chroma 0 and 1023 reach the clamps"""
    y, uv = frame(32, 32, 1)
    y[:] = (np.arange(1024, dtype=np.uint16).reshape(32, 32) << 6) | (y & 63)
    uv[:] = (np.uint16(chroma) << 6) | (uv & 63)
    check(vpp, [(y, uv)], [(32, 32)], (32, 32), M.NEAREST, flavour)


@pytest.mark.parametrize("flavour", FOUR)
@pytest.mark.parametrize("mode", [M.NEAREST, M.BILINEAR])
def test_tiny_frames_into_a_canvas_with_a_shifted_tile_column(vpp, mode, flavour):
    """2 x 2 and 4 x 2 into 66 x 34: every tap clamps, three tile columns of which the last is the shifted one, gray pad"""
    sizes = [(2, 2), (4, 2)]
    check(vpp, [frame(*s, 10 + k) for k, s in enumerate(sizes)], sizes, (66, 34), mode, flavour, pad=(456, 512, 512))


@pytest.mark.parametrize("flavour", FOUR)
def test_rectangle_origin_splits_thread_tiles(vpp, flavour):
    """left = 6 (2 mod 4) and one tile row above the rectangle: thread tiles split between chroma pairs, pad and inner tiles mix; a pad that reaches the clamps"""
    check(vpp, [frame(72, 56, 20, pitch=80)], [(72, 56)], (96, 96), M.BILINEAR, flavour, pad=(30, 1000, 12), rects=[(6, 32, 52, 40)])


@pytest.mark.parametrize("flavour", FOUR)
def test_staged_and_gathered_tiles_in_one_launch(vpp, flavour):
    """48 x 48 and 64 x 96 (the exact ratios 2 and 3: every weight 0 or 1/2) stage; 416 x 416 into the same 32 x 32 exceeds the launch's LDS and gathers"""
    import tensor_stream as ts
    sizes = [(48, 48), (416, 416), (64, 96)]
    rects = [(0, 0, 32, 32)] * 3
    fcc, planes, norm, _ = FLAVOURS[flavour]
    d = ts.describe_letterbox_p010(ts.FrameParameters(width=32, height=32, resize_type=M.BILINEAR, pixel_format=fcc, planes_pos=planes, normalization=norm), sizes, rects=rects)
    assert d["staged"] == 2 and d["src"] == "p010" and "staged" in d["kernel"], d
    check(vpp, [frame(*s, 30 + k) for k, s in enumerate(sizes)], sizes, (32, 32), M.BILINEAR, flavour, rects=rects)


@pytest.mark.parametrize("flavour", FOUR)
def test_padding_words_and_low_bits_do_not_matter(vpp, flavour):
    """a padded pitch whose padding words are 0xFFFF and random low six bits in every sample: the outputs of the clean frame"""
    y, uv = frame(40, 24, 40, pitch=56, fill=0xFFFF)
    clean = (np.ascontiguousarray(y[:, :40] & 0xFFC0), np.ascontiguousarray(uv[:, :40] & 0xFFC0))
    a = check(vpp, [(y, uv)], [(40, 24)], (64, 64), M.BILINEAR, flavour)
    b, _ = convert(vpp, [clean], [(40, 24)], (64, 64), M.BILINEAR, flavour)
    assert np.array_equal(T.bits(a), T.bits(b))


@pytest.mark.parametrize("flavour", sorted(FLAVOURS))
@pytest.mark.parametrize("canvas", [(64, 64), (30, 34)])
def test_every_store_vector_and_element_wise(vpp, canvas, flavour):
    """every flavour's store, the merged exchanges included: into 64 x 64 (vector stores) and into 30 x 34, 4 k + 2 columns narrower than a tile (element-wise)"""
    check(vpp, [frame(72, 56, 60, pitch=80)], [(72, 56)], canvas, M.BILINEAR, flavour, pad=(456, 512, 512))


def test_check_program_crcs(tmp_path):
    """VideoProcessor::ConvertLetterboxP010 through its check program: the CRC-32 it prints per canvas is the model's"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tensor-stream_amd", "lib", "vpp_letterbox_p010")
    assert os.path.exists(exe), "vpp_letterbox_p010 not built (python -c 'import __graft_entry__ as g; g.build()')"
    geo, canvas = [(128, 72, 192), (72, 128, 96), (4, 2, 8)], (70, 66)
    for fcc, planes, norm in [(M.BGR24, M.PLANAR, True), (M.RGB24, M.MERGED, False)]:
        frames, args = [], [exe, *canvas, M.BILINEAR, fcc, planes, int(norm), 456, 512, 512]
        for k, (w, h, pitch) in enumerate(geo):
            y, uv = frame(w, h, 70 + k, pitch=pitch)
            write_nv12(tmp_path / f"in{k}.p010", y, uv)
            frames.append((y, uv))
            args += [tmp_path / f"in{k}.p010", w, h, 2 * pitch]
        rc, lines, tails = run_check(args)
        assert rc == 0 and len(lines) == len(geo), (rc, *tails)
        for (idx, crc, nbytes, *rect), (w, h, _), fr in zip(lines, geo, frames):
            want_rect = default_rect(w, h, *canvas)
            assert tuple(int(v) for v in rect) == want_rect
            ref = M.expected(fr[0], fr[1], w, h, want_rect, canvas, M.BILINEAR, fcc, planes, norm, (456, 512, 512))
            assert int(nbytes) == ref.size and int(crc) == zlib.crc32(ref.tobytes()), f"canvas {idx} {(w, h)} -> {canvas}"


def test_capture_replay_and_the_split_at_32_frames(vpp):
    """33 frames of 4 x 4 (two launches) captured into a graph; replayed twice after the source planes changed, against the model"""
    sizes = [(4, 4)] * 33
    first, second = [frame(4, 4, 50 + k) for k in range(33)], [frame(4, 4, 150 + k) for k in range(33)]
    planes = ([dev(f[0]) for f in first], [dev(f[1]) for f in first])
    convert(vpp, first, sizes, (8, 8), M.BILINEAR, "f32_planar", planes_dev=planes)  # (a first call outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got, _ = convert(vpp, first, sizes, (8, 8), M.BILINEAR, "f32_planar", planes_dev=planes)
    for k, f in enumerate(second):
        planes[0][k].copy_(dev(f[0]))
        planes[1][k].copy_(dev(f[1]))
    for _ in range(2):
        got.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k, f in enumerate(second):
            assert np.array_equal(T.bits(got[k]), want(f, (4, 4), (0, 0, 8, 8), (8, 8), M.BILINEAR, "f32_planar", BLACK)), k
