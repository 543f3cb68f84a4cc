"""GPU: the tensor overloads of the C++ class (VideoProcessor::ConvertRois / ConvertLetterbox with a tsvpp_tensor_spec) through its check programs: the CRC-32
`vpp_rois --dtype f16 ...` and `vpp_letterbox --dtype bf16 ...` print per output equals the CRC of the expected bytes (tensor_util: the existing oracle's fp32
result, the float32 affine step, a round-to-nearest-even conversion)."""
import os

import numpy as np
import pytest

import tensor_util as T
from cpp_check import run_check, write_nv12
from letterbox_util import default_rect, expected_canvas
from util import synth_nv12

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tensor-stream_amd", "lib")
BILINEAR, BICUBIC = 1, 2
RGB24, BGR24 = 1, 2
PLANAR = 0
MEAN, STD = T.IMAGENET


def flags(dtype):
    # %.9g prints a float32 so that it reads back as the same float32
    mean = ",".join("%.9g" % np.float32(m) for m in MEAN)
    scale = ",".join("%.9g" % s for s in T.scales(STD))
    return ["--dtype", dtype, "--mean", mean, "--scale", scale]


def test_vpp_rois_fp16_crc_per_box(oracle, tmp_path):
    exe = os.path.join(LIB, "vpp_rois")
    assert os.path.exists(exe), "vpp_rois not built (python -c 'import __graft_entry__ as g; g.build()')"
    w, h, pitch, dst = 322, 182, 384, (64, 64)
    y, uv = synth_nv12(w, h, seed=41, pitch=pitch)
    write_nv12(tmp_path / "in.nv12", y, uv)
    boxes = [(40, 30, 140, 100), (101, 20, 201, 90), (100, 60, 164, 124), (262, 132, 322, 182)]
    args = [exe] + flags("f16") + [str(tmp_path / "in.nv12"), w, h, pitch, *dst, BILINEAR, BGR24, PLANAR, 1] + [v for b in boxes for v in b]
    rc, lines, tails = run_check(args)
    assert len(lines) == len(boxes), (rc, *tails)
    for (idx, crc, nbytes), (l, t, rr, b) in zip(lines, boxes):
        q = oracle.convert(y[t:b, l:rr], uv[t // 2:t // 2 + (b - t) // 2, l:rr], dst=dst, resize_type=BILINEAR, fourcc=BGR24, planes=PLANAR, normalization=True)[0]
        want = T.expected(q, 3, T.IMAGENET, T.F16)
        assert int(nbytes) == want.size == 3 * 64 * 64 * 2
        assert int(crc) == oracle.av_crc32_ieee(want), f"box {idx} {(l, t, rr, b)}"
    assert rc == 0, (rc, *tails)


def test_vpp_letterbox_bf16_crc_per_canvas(oracle, tmp_path):
    exe = os.path.join(LIB, "vpp_letterbox")
    assert os.path.exists(exe), "vpp_letterbox not built (python -c 'import __graft_entry__ as g; g.build()')"
    geo = [(128, 72, 192), (72, 128, 96)]
    canvas, pad = (70, 66), (114, 128, 128)
    args = [exe] + flags("bf16") + [*canvas, BICUBIC, RGB24, PLANAR, 1, *pad]
    host = []
    for k, (w, h, p) in enumerate(geo):
        y, uv = synth_nv12(w, h, seed=51 + k, pitch=p)
        host.append((y, uv))
        write_nv12(tmp_path / f"f{k}.nv12", y, uv)
        args += [str(tmp_path / f"f{k}.nv12"), w, h, p]
    rc, lines, tails = run_check(args)
    assert len(lines) == len(geo), (rc, *tails)
    for k, ln in enumerate(lines):
        w, h, _ = geo[k]
        rect = default_rect(w, h, *canvas)
        assert tuple(int(v) for v in ln[3:7]) == rect
        q = expected_canvas(oracle, host[k][0], host[k][1], w, h, rect, canvas, BICUBIC, RGB24, PLANAR, True, pad).view(np.float32)
        want = T.expected(q, 3, T.IMAGENET, T.BF16)
        assert int(ln[2]) == want.size == 3 * 70 * 66 * 2
        assert int(ln[1]) == T.crc32_zlib(want), f"canvas {k}"
    assert rc == 0, (rc, *tails)
