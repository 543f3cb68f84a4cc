"""GPU: VideoProcessor::ConvertLetterboxArea of the C++ class (tensor-stream_amd/cpp/VideoProcessor.h), plain and with a tensor spec, through `vpp_letterbox --area`:
the CRC-32 it prints per canvas (zlib's, over the device result) equals zlib.crc32 of the expected canvas (tests/letterbox_util.py with the oracle's AREA resize;
tensors: tests/tensor_util.py)."""
import os
import zlib

import numpy as np
import pytest

import tensor_util as T
from cpp_check import run_check, write_nv12
from letterbox_util import AREA, default_rect, expected_canvas
from util import synth_nv12

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tensor-stream_amd", "lib", "vpp_letterbox")

GEO = [(128, 72, 192), (72, 128, 96), (32, 18, 48), (322, 182, 384)]  # two down-scales, the up-scale rule, a ratio above 5
RGB24, BGR24, PLANAR, MERGED = 1, 2, 0, 1


def run(oracle, tmp_path, flags, canvas, fourcc, planes, norm, pad):
    assert os.path.exists(EXE), "vpp_letterbox not built (python -c 'import __graft_entry__ as g; g.build()')"
    frames, args = [], [EXE, "--area", *flags, *canvas, AREA, fourcc, planes, int(norm), *pad]
    for k, (w, h, pitch) in enumerate(GEO):
        y, uv = synth_nv12(w, h, seed=1900 + k + canvas[0], pitch=pitch)
        src = tmp_path / f"in{k}.nv12"
        write_nv12(src, y, uv)
        frames.append((y, uv))
        args += [src, w, h, pitch]
    rc, lines, tails = run_check(args)
    assert len(lines) == len(GEO), (rc, *tails)
    return rc, lines, tails, frames


@pytest.mark.parametrize("canvas,fourcc,planes,norm,pad", [
    ((64, 64), BGR24, PLANAR, True, (114, 128, 128)),  # BGR24 planar fp32: the detector's usual request
    ((70, 66), RGB24, MERGED, False, (16, 128, 128)),  # RGB24 merged uint8, a width of the form 4 k + 2, black pad
])
def test_crc_per_canvas(oracle, tmp_path, canvas, fourcc, planes, norm, pad):
    rc, lines, tails, frames = run(oracle, tmp_path, [], canvas, fourcc, planes, norm, pad)
    for (idx, crc, nbytes, *rect), (w, h, _), (y, uv) in zip(lines, GEO, frames):
        want = default_rect(w, h, *canvas)
        assert tuple(int(v) for v in rect) == want, (idx, rect, want)
        ref = expected_canvas(oracle, y, uv, w, h, want, canvas, AREA, fourcc, planes, norm, pad)
        assert int(nbytes) == ref.size
        assert int(crc) == zlib.crc32(ref.tobytes()), f"canvas {idx} {(w, h)} -> {canvas}"
    # (after the canvases the program asks for a rectangle outside the canvas: refused with VREADER_ERROR; exit code 0 = all of it held)
    assert rc == 0, (rc, *tails)


def test_fp16_crc_per_canvas(oracle, tmp_path):
    canvas, pad = (70, 66), (114, 128, 128)
    mean = ",".join("%.9g" % np.float32(m) for m in T.IMAGENET[0])  # %.9g prints a float32 so that it reads back as the same float32
    scale = ",".join("%.9g" % s for s in T.scales(T.IMAGENET[1]))
    rc, lines, tails, frames = run(oracle, tmp_path, ["--dtype", "f16", "--mean", mean, "--scale", scale], canvas, RGB24, PLANAR, True, pad)
    for k, ln in enumerate(lines):
        w, h, _ = GEO[k]
        rect = default_rect(w, h, *canvas)
        assert tuple(int(v) for v in ln[3:7]) == rect
        q = expected_canvas(oracle, frames[k][0], frames[k][1], w, h, rect, canvas, AREA, RGB24, PLANAR, True, pad).view(np.float32)
        want = T.expected(q, 3, T.IMAGENET, T.F16)
        assert int(ln[2]) == want.size == 3 * 70 * 66 * 2
        assert int(ln[1]) == T.crc32_zlib(want), f"canvas {k}"
    assert rc == 0, (rc, *tails)
