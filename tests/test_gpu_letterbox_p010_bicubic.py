"""GPU: tsvpp_convert_letterbox_p010_bicubic -- 10-bit P010 frames through the separable integer cubic into letterboxed canvases -- against
tests/p010_cubic_util.py, the int64 restatement of the resize that include/tsvpp.h states.  Every comparison is on raw bits.  FOUR = uint8 merged, fp32 planar,
an fp16 tensor with ImageNet mean / std, Y800 fp32."""
import os
import zlib

import numpy as np
import pytest
import torch

import p010_cases as C
import p010_util as M
import tensor_util as T
from cpp_check import run_check, write_nv12
from letterbox_util import default_rect
from p010_cases import BLACK, FLAVOURS, FOUR, GRAY, dev, frame
from p010_cubic_util import BICUBIC, cubic

pytestmark = pytest.mark.gpu


def virtual_frame(y, uv, w, h, rect, canvas, pad):
    """p010_area_util.virtual_frame with the cubic: the canvas before the colour stage"""
    (cw, ch), (left, top, iw, ih) = canvas, rect
    Ys, UVs = M.samples(y)[:h, :w], M.samples(uv)[:h // 2, :w]
    Y, U, V = (np.full(s, p, np.int64) for s, p in zip(((ch, cw), (ch // 2, cw // 2), (ch // 2, cw // 2)), pad))
    Y[top:top + ih, left:left + iw] = cubic(Ys, iw, ih)
    for P, S in ((U, UVs[:, 0::2]), (V, UVs[:, 1::2])):
        P[top // 2:(top + ih) // 2, left // 2:(left + iw) // 2] = cubic(S, iw // 2, ih // 2)
    return Y, U, V


def want(fr, size, rect, canvas, flavour, pad):
    return C.stored(M.channels(*virtual_frame(fr[0], fr[1], *size, rect, canvas, pad), FLAVOURS[flavour][0]), flavour)


def convert(vpp, frames, sizes, canvas, flavour, pad=BLACK, rects=None, planes_dev=None):
    fp, kw = C.params(canvas, BICUBIC, flavour)
    ys, uvs = planes_dev or ([dev(f[0]) for f in frames], [dev(f[1]) for f in frames])
    return vpp.convert_letterbox_p010_bicubic(ys, uvs, fp, pad=pad, rects=rects, width=[s[0] for s in sizes], height=[s[1] for s in sizes], **kw)


def check(vpp, frames, sizes, canvas, flavour, pad=BLACK, rects=None, planes_dev=None):
    got, used = convert(vpp, frames, sizes, canvas, flavour, pad, rects, planes_dev)
    torch.cuda.synchronize()
    for k, (fr, size) in enumerate(zip(frames, sizes)):
        rect = tuple(rects[k]) if rects else default_rect(*size, *canvas)
        assert tuple(used[k]) == rect
        C.same(got[k], want(fr, size, rect, canvas, flavour, pad), f"frame {k} {size} -> {canvas} rect {rect} {flavour}")
    return got


# the identity; exact 2 x up; ratio 2; 3 : 2; the limit 8 over many bands; one axis up and one down; just above 1
ONE_TILE = [(32, 32), (16, 16), (64, 64), (48, 48), (256, 256), (24, 64), (34, 34)]


@pytest.mark.parametrize("flavour", FOUR)
@pytest.mark.parametrize("size", ONE_TILE)
def test_one_tile(vpp, size, flavour):
    fr = frame(*size, 10)
    a = check(vpp, [fr], [size], (32, 32), flavour, rects=[(0, 0, 32, 32)])
    if size == (32, 32):  # F = 0 on both axes: byte-equal to the NEAREST call
        b, _ = C.convert(vpp, [fr], [size], (32, 32), M.NEAREST, flavour)
        assert np.array_equal(T.bits(a), T.bits(b))


@pytest.mark.parametrize("flavour", FOUR)
@pytest.mark.parametrize("sizes,canvas,rects,pad", [
    ([(4, 4)], (40, 36), [(0, 0, 40, 36)], BLACK),                # every tap clamps at the frame
    ([(200, 120)], (96, 96), [(6, 32, 84, 50)], (30, 1000, 12)),  # thread tiles split by the rectangle's edge, Hbuf columns at 2 mod 4, pad, inner and mixed tiles
    ([(100, 60)], (66, 34), None, (30, 1000, 12)),                # the shifted last tile column
    ([(2, 2), (4, 2)], (66, 34), None, (30, 1000, 12)),           # tiny frames
    ([(32, 32), (16, 16), (256, 256)], (32, 32), [(0, 0, 32, 32)] * 3, BLACK)])  # hrows / band_cpr taken over the launch
def test_tile_seams_and_the_rectangle(vpp, sizes, canvas, rects, pad, flavour):
    check(vpp, [frame(*s, 20 + k) for k, s in enumerate(sizes)], sizes, canvas, flavour, pad=pad, rects=rects)


@pytest.mark.parametrize("flavour", FOUR)
def test_checkerboard_overshoots_into_both_clamps(vpp, flavour):
    """0 / 1023 in blocks of 3 samples, 24 x 24 -> 32 x 32: the unclamped h range, both clamps of k"""
    yy, xx = np.mgrid[0:24, 0:24]
    y = ((((xx // 3 + yy // 3) & 1) * 1023) << 6).astype(np.uint16)
    uv = np.ascontiguousarray(y[:12] ^ (np.arange(24, dtype=np.uint16) & 1) * np.uint16(1023 << 6))
    check(vpp, [(y, uv)], [(24, 24)], (32, 32), flavour, rects=[(0, 0, 32, 32)])


@pytest.mark.parametrize("flavour", FOUR)
def test_full_rectangle_equals_the_roi_call(vpp, flavour):
    """(50, 38) -> (32, 30): byte-equal to convert_rois_p010_bicubic of the box that is all of the frame"""
    fr = frame(50, 38, 40)
    a = check(vpp, [fr], [(50, 38)], (32, 30), flavour, rects=[(0, 0, 32, 30)])
    fp, kw = C.params((32, 30), BICUBIC, flavour)
    b = vpp.convert_rois_p010_bicubic([dev(fr[0])], [dev(fr[1])], [(0, 0, 0, 50, 38)], fp, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(T.bits(a), T.bits(b))


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


def test_capture_replay_and_the_split_at_32_frames(vpp):
    """33 frames of 8 x 8 -> 12 x 12 (two launches) captured into a graph; replayed twice after the source planes changed, against the model"""
    sizes = [(8, 8)] * 33
    first, second = [frame(8, 8, 50 + k) for k in range(33)], [frame(8, 8, 150 + k) for k in range(33)]
    planes = ([dev(f[0]) for f in first], [dev(f[1]) for f in first])
    convert(vpp, first, sizes, (12, 12), "f32_planar", planes_dev=planes)  # (a first call outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got, _ = convert(vpp, first, sizes, (12, 12), "f32_planar", planes_dev=planes)
    for k, f in enumerate(second):
        planes[0][k].copy_(dev(f[0]))
        planes[1][k].copy_(dev(f[1]))
    for _ in range(2):
        got.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k, f in enumerate(second):
            assert np.array_equal(T.bits(got[k]), want(f, (8, 8), (0, 0, 12, 12), (12, 12), "f32_planar", BLACK)), k


def test_check_program_crcs(tmp_path):
    """VideoProcessor::ConvertLetterboxP010Bicubic through the check program's --bicubic: the CRC-32 it prints per canvas is the model's"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tensor-stream_amd", "lib", "vpp_letterbox_p010")
    assert os.path.exists(exe), "vpp_letterbox_p010 not built (python -c 'import __graft_entry__ as g; g.build()')"
    geo, canvas, flavour = [(128, 72, 192), (72, 128, 96), (4, 2, 8)], (70, 66), "f32_planar"
    fcc, planes, norm, _ = FLAVOURS[flavour]
    frames, args = [], [exe, "--bicubic", *canvas, BICUBIC, fcc, planes, int(norm), *GRAY]
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
        ref = want(fr, (w, h), want_rect, canvas, flavour, GRAY)
        assert int(nbytes) == ref.size and int(crc) == zlib.crc32(ref.tobytes()), f"canvas {idx} {(w, h)} -> {canvas}"
