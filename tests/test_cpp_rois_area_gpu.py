"""GPU: VideoProcessor::ConvertRoisArea of the C++ class (tensor-stream_amd/cpp/VideoProcessor.h) through its check program `vpp_rois --area`: the CRC-32 it prints
per box (libavutil's AV_CRC_32_IEEE over the device result) equals the oracle's over its own bytes for the box's sliced planes, resized with AREA."""
import os

import numpy as np
import pytest

from cpp_check import run_check, write_nv12
from util import synth_nv12

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tensor-stream_amd", "lib", "vpp_rois")
AREA = 3

# a down-scale, an up-scale with odd corners, a full-width strip, the whole frame (11 x 7 taps at 112 x 112: it gathers)
BOXES = [(100, 50, 700, 550), (301, 201, 365, 249), (0, 100, 1280, 400), (0, 0, 1280, 720)]


@pytest.mark.parametrize("pitch,dst,fourcc,planes,norm", [
    (1280, (224, 224), 2, 0, True),     # BGR24 planar fp32
    (1344, (112, 112), 1, 1, False),    # RGB24 merged uint8, pitched input
])
def test_crc_per_box(oracle, tmp_path, pitch, dst, fourcc, planes, norm):
    assert os.path.exists(EXE), "vpp_rois not built (python -c 'import __graft_entry__ as g; g.build()')"
    w, h = 1280, 720
    y, uv = synth_nv12(w, h, seed=pitch + dst[0] + fourcc, pitch=pitch)
    src = tmp_path / "in.nv12"
    write_nv12(src, y, uv)
    args = [EXE, "--area", str(src), w, h, pitch, *dst, AREA, fourcc, planes, int(norm)] + [v for b in BOXES for v in b]
    rc, lines, tails = run_check(args)
    assert len(lines) == len(BOXES), (rc, *tails)
    for (idx, crc, nbytes), (l, t, rr, b) in zip(lines, BOXES):
        ys = y[t:b, l:rr]
        uvs = uv[t // 2:t // 2 + (b - t) // 2, l:rr]
        ref = oracle.convert(ys, uvs, dst=dst, resize_type=AREA, fourcc=fourcc, planes=planes, normalization=norm, nthreads=4)[0]
        assert int(nbytes) == ref.view(np.uint8).size
        assert int(crc) == oracle.av_crc32_ieee(ref), f"box {idx} {(l, t, rr, b)}"
    assert rc == 0, (rc, *tails)
