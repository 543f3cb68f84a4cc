"""GPU: VideoProcessor::ConvertRoisSized of the C++ class (tensor-stream_amd/cpp/VideoProcessor.h) through its check program vpp_rois_sized: the CRC-32 it prints
per box (libavutil's AV_CRC_32_IEEE over the device result) equals the oracle's over its own bytes for the box's sliced planes at the box's own size (the contract
of tsvpp_convert_rois_sized); then the program asks for a request with the parameters' own size set and checks that it is refused."""
import os

import numpy as np
import pytest

from cpp_check import run_check, write_nv12
from util import synth_nv12

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tensor-stream_amd", "lib", "vpp_rois_sized")

# seven boxes of seven sizes: text lines, a face, a plate, a person, a thumbnail of the frame, a 2 x 2 corner
BOXES = [(100, 50, 700, 150, 192, 32), (301, 201, 365, 249, 42, 32), (0, 0, 224, 224, 112, 112), (0, 100, 1280, 324, 640, 48), (900, 0, 1100, 720, 128, 256),
         (1278, 718, 1280, 720, 2, 2), (0, 0, 1280, 720, 240, 134)]


@pytest.mark.parametrize("pitch,rtype,fourcc,planes,norm", [
    (1280, 1, 2, 0, True),     # BILINEAR, BGR24 planar fp32
    (1344, 2, 1, 1, False),    # BICUBIC, RGB24 merged uint8, pitched input
])
def test_crc_per_box(oracle, tmp_path, pitch, rtype, fourcc, planes, norm):
    assert os.path.exists(EXE), "vpp_rois_sized not built (python -c 'import __graft_entry__ as g; g.build()')"
    w, h = 1280, 720
    y, uv = synth_nv12(w, h, seed=pitch + rtype + fourcc, pitch=pitch)
    src = tmp_path / "in.nv12"
    write_nv12(src, y, uv)
    args = [EXE, str(src), w, h, pitch, rtype, fourcc, planes, int(norm)] + [v for b in BOXES for v in b]
    rc, lines, tails = run_check(args)
    assert len(lines) == len(BOXES), (rc, *tails)
    for (idx, crc, nbytes), (l, t, rr, b, dw, dh) in zip(lines, BOXES):
        ys = y[t:b, l:rr]
        uvs = uv[t // 2:t // 2 + (b - t) // 2, l:rr]
        ref = oracle.convert(ys, uvs, dst=(dw, dh), resize_type=rtype, fourcc=fourcc, planes=planes, normalization=norm, nthreads=4)[0]
        assert int(nbytes) == ref.view(np.uint8).size
        assert int(crc) == oracle.av_crc32_ieee(ref), f"box {idx} {(l, t, rr, b)} -> {(dw, dh)}"
    # (after the boxes the program sets the parameters' own size: refused with VREADER_ERROR, reported as CHECK_STATUS does; exit code 0 = all of it held)
    assert rc == 0, (rc, *tails)
