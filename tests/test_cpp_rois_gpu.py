"""GPU: VideoProcessor::ConvertRois of the C++ class (tensor-stream_amd/cpp/VideoProcessor.h) through its check program vpp_rois: the CRC-32 it prints per box
(libavutil's AV_CRC_32_IEEE over the device result) equals the oracle's over its own bytes for the box's sliced planes (the contract of tsvpp_convert_rois)."""
import os

import numpy as np
import pytest

from cpp_check import run_check, write_nv12
from util import synth_nv12

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tensor-stream_amd", "lib", "vpp_rois")

BOXES = [(100, 50, 700, 550), (301, 201, 365, 249), (0, 0, 224, 224), (0, 100, 1280, 324), (900, 0, 1100, 720), (1278, 718, 1280, 720), (640, 360, 1280, 720)]


@pytest.mark.parametrize("pitch,dst,rtype,fourcc,planes,norm", [
    (1280, (224, 224), 1, 2, 0, True),     # BILINEAR, BGR24 planar fp32: the cascade's usual request
    (1344, (112, 112), 2, 1, 1, False),    # BICUBIC, RGB24 merged uint8, pitched input
    (1280, (250, 250), 0, 0, 1, False),    # NEAREST, Y800, a width of the form 4 k + 2
    (1280, (224, 224), 2, 1, 1, True),     # BICUBIC, merged fp32
])
def test_crc_per_box(oracle, tmp_path, pitch, dst, rtype, fourcc, planes, norm):
    assert os.path.exists(EXE), "vpp_rois not built (python -c 'import __graft_entry__ as g; g.build()')"
    w, h = 1280, 720
    y, uv = synth_nv12(w, h, seed=pitch + dst[0] + fourcc, pitch=pitch)
    src = tmp_path / "in.nv12"
    write_nv12(src, y, uv)
    args = [EXE, str(src), w, h, pitch, *dst, rtype, fourcc, planes, int(norm)] + [v for b in BOXES for v in b]
    rc, lines, tails = run_check(args)
    assert len(lines) == len(BOXES), (rc, *tails)
    for (idx, crc, nbytes), (l, t, rr, b) in zip(lines, BOXES):
        ys = y[t:b, l:rr]
        uvs = uv[t // 2:t // 2 + (b - t) // 2, l:rr]
        ref = oracle.convert(ys, uvs, dst=dst, resize_type=rtype, fourcc=fourcc, planes=planes, normalization=norm, nthreads=4)[0]
        assert int(nbytes) == ref.view(np.uint8).size
        assert int(crc) == oracle.av_crc32_ieee(ref), f"box {idx} {(l, t, rr, b)}"
    # (after the boxes the program asks for a box outside the frame: refused with VREADER_ERROR, reported as CHECK_STATUS does; exit code 0 = all of it held)
    assert rc == 0, (rc, *tails)
