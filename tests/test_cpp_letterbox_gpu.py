"""GPU: VideoProcessor::ConvertLetterbox of the C++ class (tensor-stream_amd/cpp/VideoProcessor.h) through its check program vpp_letterbox: the CRC-32 it prints
per canvas (zlib's, over the device result) equals zlib.crc32 of the expected canvas (tests/letterbox_util.py: the contract of tsvpp_convert_letterbox)."""
import os
import zlib

import pytest

from cpp_check import run_check, write_nv12
from letterbox_util import default_rect, expected_canvas
from util import synth_nv12

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tensor-stream_amd", "lib", "vpp_letterbox")

GEO = [(128, 72, 192), (72, 128, 96), (64, 64, 64), (322, 182, 384)]


@pytest.mark.parametrize("canvas,rtype,fourcc,planes,norm,pad", [
    ((64, 64), 1, 2, 0, True, (114, 128, 128)),     # BILINEAR, BGR24 planar fp32: the detector's usual request
    ((70, 66), 2, 1, 1, False, (16, 128, 128)),     # BICUBIC, RGB24 merged uint8, a width of the form 4 k + 2, black pad
    ((96, 64), 0, 0, 1, False, (3, 250, 7)),        # NEAREST, Y800
])
def test_crc_per_canvas(oracle, tmp_path, canvas, rtype, fourcc, planes, norm, pad):
    assert os.path.exists(EXE), "vpp_letterbox not built (python -c 'import __graft_entry__ as g; g.build()')"
    frames, args = [], [EXE, *canvas, rtype, fourcc, planes, int(norm), *pad]
    for k, (w, h, pitch) in enumerate(GEO):
        y, uv = synth_nv12(w, h, seed=900 + k + canvas[0], pitch=pitch)
        src = tmp_path / f"in{k}.nv12"
        write_nv12(src, y, uv)
        frames.append((y, uv))
        args += [src, w, h, pitch]
    rc, lines, tails = run_check(args)
    assert len(lines) == len(GEO), (rc, *tails)
    for (idx, crc, nbytes, *rect), (w, h, _), (y, uv) in zip(lines, GEO, frames):
        want = default_rect(w, h, *canvas)
        assert tuple(int(v) for v in rect) == want, (idx, rect, want)
        ref = expected_canvas(oracle, y, uv, w, h, want, canvas, rtype, fourcc, planes, norm, pad)
        assert int(nbytes) == ref.size
        assert int(crc) == zlib.crc32(ref.tobytes()), f"canvas {idx} {(w, h)} -> {canvas}"
    # (after the canvases the program asks for a rectangle outside the canvas: refused with VREADER_ERROR; exit code 0 = all of it held)
    assert rc == 0, (rc, *tails)
