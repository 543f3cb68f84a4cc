"""GPU: VideoProcessor::ConvertWarp of the C++ class (tensor-stream_amd/cpp/VideoProcessor.h) through its check program vpp_warp: the CRC-32 it prints per output
(zlib's, over the device result) equals zlib.crc32 of the expected output (tests/warp_util.py: the contract of tsvpp_convert_warp)."""
import math
import os
import zlib

import numpy as np
import pytest

import tensor_util as T
import warp_util as W
from cpp_check import run_check, write_nv12
from util import synth_nv12

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tensor-stream_amd", "lib", "vpp_warp")

GEO = (322, 182, 384)


def rotated(dst):
    import tensor_stream as ts
    w, h, _ = GEO
    return [ts.warp_rotated_box(w / 2, h / 2, 1.7 * dst[0], 1.7 * dst[1], math.radians(30), *dst), ts.warp_rotated_box(0, h / 2, w, h, 0.2, *dst),
            tuple(float(np.float32(v)) for v in (0.37, 0.1, 0.3 * w, 0.05, 0.37, 0.3 * h))]


@pytest.mark.parametrize("dst,fourcc,planes,norm,border,dtype", [
    ((70, 66), 1, 1, False, (-1, -1, -1), None),        # RGB24 merged uint8, a width of the form 4 k + 2, replicate
    ((112, 112), 2, 0, True, (114, 128, 128), None),    # BGR24 planar fp32, gray border
    ((112, 112), 2, 0, True, (114, 128, 128), T.F16),   # ... as fp16 with ImageNet mean / std, through the overload with a spec
])
@pytest.mark.parametrize("kind", ["scale_only", "rotated"])
def test_crc_per_output(oracle, tmp_path, kind, dst, fourcc, planes, norm, border, dtype):
    assert os.path.exists(EXE), "vpp_warp not built (python -c 'import __graft_entry__ as g; g.build()')"
    w, h, pitch = GEO
    y, uv = synth_nv12(w, h, seed=1400 + dst[0], pitch=pitch)
    src = tmp_path / "in.nv12"
    write_nv12(src, y, uv)
    ms = [W.scale_only(w, h, *dst)] if kind == "scale_only" else rotated(dst)
    args = [EXE]
    if dtype is not None:
        sc = T.scales(T.IMAGENET[1])
        args += ["--dtype", dtype, "--mean", ",".join(float(np.float32(v)).hex() for v in T.IMAGENET[0]), "--scale", ",".join(float(v).hex() for v in sc)]
    args += [*dst, fourcc, planes, int(norm), *border, src, w, h, pitch]
    for m in ms:
        args += [float(np.float32(v)).hex() for v in m]
    rc, lines, tails = run_check(args)
    assert len(lines) == len(ms), (rc, *tails)
    for (idx, crc, nbytes), m in zip(lines, ms):
        ref = W.expected(oracle, y, uv, w, h, m, dst, fourcc, planes, norm, None if border[0] < 0 else border)
        if dtype is not None:
            ref = T.expected(ref.view(np.float32), 3, T.IMAGENET, dtype)
        assert int(nbytes) == ref.size
        assert int(crc) == zlib.crc32(ref.tobytes()), f"output {idx} m={m} -> {dst}"
    # (after the outputs the program asks for a matrix of a frame it did not give: refused with VREADER_ERROR; exit code 0 = all of it held)
    assert rc == 0, (rc, *tails)
