"""GPU: tsvpp_convert_letterbox_p010_area -- 10-bit P010 frames through an exact integer box filter into letterboxed canvases -- against tests/p010_area_util.py,
the numpy restatement of the contract of include/tsvpp.h.  Every comparison is on raw bits.  The flavours: uint8 merged, fp32 planar, an fp16 tensor with ImageNet
mean / std, Y800 fp32."""
import os
import zlib

import numpy as np
import pytest
import torch

import p010_area_util as A
import p010_cases as C
import p010_util as M
import tensor_util as T
from cpp_check import run_check, write_nv12
from letterbox_util import default_rect
from p010_cases import BLACK, FLAVOURS, FOUR, dev, frame

pytestmark = pytest.mark.gpu
GRAY = (456, 512, 512)


def convert(vpp, frames, sizes, canvas, flavour, pad=BLACK, rects=None, planes_dev=None):
    fp, kw = C.params(canvas, A.AREA, flavour)
    ys, uvs = planes_dev or ([dev(f[0]) for f in frames], [dev(f[1]) for f in frames])
    return vpp.convert_letterbox_p010_area(ys, uvs, fp, pad=pad, rects=rects, width=[s[0] for s in sizes], height=[s[1] for s in sizes], **kw)


def check(vpp, frames, sizes, canvas, flavour, pad=BLACK, rects=None, planes_dev=None):
    got, used = convert(vpp, frames, sizes, canvas, flavour, pad, rects, planes_dev)
    torch.cuda.synchronize()
    for k, (fr, size) in enumerate(zip(frames, sizes)):
        rect = tuple(rects[k]) if rects else default_rect(*size, *canvas)
        assert tuple(used[k]) == rect
        C.same(got[k], A.want(fr, size, rect, canvas, flavour, pad), f"frame {k} {size} -> {canvas} rect {rect} {flavour}")
    return got


@pytest.mark.parametrize("flavour", FOUR)
def test_equal_size_is_the_identity(vpp, flavour):
    """32 x 32 -> 32 x 32: one tap of weight N per axis, and byte-equal to the NEAREST call"""
    fr = frame(32, 32, 1)
    a = check(vpp, [fr], [(32, 32)], (32, 32), flavour)
    b, _ = C.convert(vpp, [fr], [(32, 32)], (32, 32), M.NEAREST, flavour)
    assert np.array_equal(T.bits(a), T.bits(b))


# ratio 2; 3; 3 : 2 (weights 2, 1 / 1, 2); just above 1; mixed; 6 (a footprint above the LDS budget: several bands); 16 x 2 (16 taps); 17 taps; one axis up, one down
ONE_TILE = [(64, 64), (96, 96), (48, 48), (34, 34), (50, 38), (192, 192), (512, 64), (514, 64), (24, 64)]


@pytest.mark.parametrize("flavour", FOUR)
@pytest.mark.parametrize("size", ONE_TILE)
def test_one_tile(vpp, size, flavour):
    check(vpp, [frame(*size, 10)], [size], (32, 32), flavour, rects=[(0, 0, 32, 32)])


@pytest.mark.parametrize("flavour", FOUR)
@pytest.mark.parametrize("sizes,canvas,rects", [
    ([(200, 120)], (96, 96), [(6, 32, 84, 50)]),  # split thread tiles, pad and inner tiles, sources shared across tile edges
    ([(100, 60)], (66, 34), None),                # the shifted last tile column
    ([(2, 2), (4, 2)], (66, 34), None)])          # an up-scale of tiny frames: one or two taps
def test_tile_seams_and_the_rectangle(vpp, sizes, canvas, rects, flavour):
    check(vpp, [frame(*s, 20 + k) for k, s in enumerate(sizes)], sizes, canvas, flavour, pad=(30, 1000, 12), rects=rects)


@pytest.mark.parametrize("flavour", ["y800_f32", "f32_planar"])
@pytest.mark.parametrize("size,canvas", [((16384, 2), (1024, 2)), ((2, 16384), (2, 1024)), ((32, 32), (32, 32))])
def test_integer_bounds(vpp, size, canvas, flavour):
    """flat 1023 at the longest side either way: the largest hx, v and first taps the limits allow; at equal size the luma ramp of all 1024 codes"""
    w, h = size
    y, uv = np.full((h, w), 1023 << 6, np.uint16), np.full((h // 2, w), 1023 << 6, np.uint16)
    if size == canvas:
        y[:] = np.arange(1024, dtype=np.uint16).reshape(32, 32) << 6
    check(vpp, [(y, uv)], [size], canvas, flavour, rects=[(0, 0, *canvas)])


@pytest.mark.parametrize("flavour", FOUR)
def test_padding_words_and_low_bits_do_not_matter(vpp, flavour):
    y, uv = frame(40, 24, 40, pitch=56, fill=0xFFFF)
    clean = (np.ascontiguousarray(y[:, :40] & 0xFFC0), np.ascontiguousarray(uv[:, :40] & 0xFFC0))
    a = check(vpp, [(y, uv)], [(40, 24)], (32, 32), flavour)
    b, _ = convert(vpp, [clean], [(40, 24)], (32, 32), flavour)
    assert np.array_equal(T.bits(a), T.bits(b))


@pytest.mark.parametrize("flavour", FOUR)
@pytest.mark.parametrize("layout", [C.LAYOUTS[k] for k in (1, 2, 4)])
def test_plane_layouts(vpp, layout, flavour):
    """odd pitch, odd offset, uv4 at 4 mod 16: 50 x 38 -> 32 x 30 from planes embedded in a buffer of 0xFFFF words"""
    fr = frame(50, 38, 50)
    ty, tuv, _ = C.embed(*fr, 50, 38, layout)
    check(vpp, [fr], [(50, 38)], (32, 30), flavour, rects=[(0, 0, 32, 30)], planes_dev=([ty], [tuv]))


@pytest.mark.parametrize("flavour", sorted(FLAVOURS))
@pytest.mark.parametrize("canvas", [(64, 64), (30, 34)])
def test_every_store_vector_and_element_wise(vpp, canvas, flavour):
    check(vpp, [frame(72, 56, 60, pitch=80)], [(72, 56)], canvas, flavour, pad=GRAY)


@pytest.mark.parametrize("flavour", FOUR)
def test_one_launch_mixes_ratios_1_3_and_6(vpp, flavour):
    sizes = [(32, 32), (96, 96), (192, 192)]
    check(vpp, [frame(*s, 30 + k) for k, s in enumerate(sizes)], sizes, (32, 32), flavour, rects=[(0, 0, 32, 32)] * 3)


def test_capture_replay_and_the_split_at_32_frames(vpp):
    """33 frames of 8 x 8 -> 4 x 4 (two launches) captured into a graph; replayed twice after the source planes changed, against the model"""
    sizes = [(8, 8)] * 33
    first, second = [frame(8, 8, 50 + k) for k in range(33)], [frame(8, 8, 150 + k) for k in range(33)]
    planes = ([dev(f[0]) for f in first], [dev(f[1]) for f in first])
    convert(vpp, first, sizes, (4, 4), "f32_planar", planes_dev=planes)  # (a first call outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got, _ = convert(vpp, first, sizes, (4, 4), "f32_planar", planes_dev=planes)
    for k, f in enumerate(second):
        planes[0][k].copy_(dev(f[0]))
        planes[1][k].copy_(dev(f[1]))
    for _ in range(2):
        got.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k, f in enumerate(second):
            assert np.array_equal(T.bits(got[k]), A.want(f, (8, 8), (0, 0, 4, 4), (4, 4), "f32_planar", BLACK)), k


def test_check_program_crcs(tmp_path):
    """VideoProcessor::ConvertLetterboxP010Area through the check program's --area: the CRC-32 it prints per canvas is the model's"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tensor-stream_amd", "lib", "vpp_letterbox_p010")
    assert os.path.exists(exe), "vpp_letterbox_p010 not built (python -c 'import __graft_entry__ as g; g.build()')"
    geo, canvas = [(128, 72, 192), (72, 128, 96), (4, 2, 8)], (70, 66)
    for flavour in ("f32_planar", "u8_merged"):
        fcc, planes, norm, _ = FLAVOURS[flavour]
        frames, args = [], [exe, "--area", *canvas, A.AREA, fcc, planes, int(norm), *GRAY]
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
            ref = A.want(fr, (w, h), want_rect, canvas, flavour, GRAY)
            assert int(nbytes) == ref.size and int(crc) == zlib.crc32(ref.tobytes()), f"canvas {idx} {(w, h)} -> {canvas}"
