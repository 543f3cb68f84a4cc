"""GPU: VideoProcessor::ConvertPerspective of the C++ class (tensor-stream_amd/cpp/VideoProcessor.h) through its check program vpp_persp: the CRC-32 it prints per
output (zlib's, over the device result) equals zlib.crc32 of the expected output (tests/persp_util.py: the contract of tsvpp_convert_perspective)."""
import os
import zlib

import numpy as np
import pytest

import persp_util as P
import tensor_util as T
import warp_util as W
from cpp_check import run_check, write_nv12
from util import synth_nv12

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tensor-stream_amd", "lib", "vpp_persp")

GEO = (322, 182, 384)


def quads(dst):
    w, h, _ = GEO
    qs = [[(0.1 * w, 0.1 * h), (0.9 * w, 0.15 * h), (0.85 * w, 0.9 * h), (0.12 * w, 0.85 * h)],       # a mild keystone
          [(0.42 * w, 0.2 * h), (0.58 * w, 0.2 * h), (0.98 * w, 0.9 * h), (0.02 * w, 0.9 * h)],       # a strong one
          [(-0.4 * w, 0.1 * h), (0.4 * w, 0.15 * h), (0.35 * w, 0.9 * h), (-0.38 * w, 0.85 * h)]]     # half outside
    return [P.from_quad(q, *dst) for q in qs]


@pytest.mark.parametrize("dst,fourcc,planes,norm,border,dtype", [
    ((70, 66), 1, 1, False, (-1, -1, -1), None),        # RGB24 merged uint8, a width of the form 4 k + 2, replicate
    ((112, 112), 2, 0, True, (114, 128, 128), None),    # BGR24 planar fp32, gray border
    ((112, 112), 2, 0, True, (114, 128, 128), T.F16),   # ... as fp16 with ImageNet mean / std, through the overload with a spec
])
@pytest.mark.parametrize("kind", ["scale_only", "quads"])
def test_crc_per_output(oracle, tmp_path, kind, dst, fourcc, planes, norm, border, dtype):
    assert os.path.exists(EXE), "vpp_persp not built (python -c 'import __graft_entry__ as g; g.build()')"
    w, h, pitch = GEO
    y, uv = synth_nv12(w, h, seed=1600 + dst[0], pitch=pitch)
    src = tmp_path / "in.nv12"
    write_nv12(src, y, uv)
    hs = [P.affine(W.scale_only(w, h, *dst))] if kind == "scale_only" else quads(dst)
    args = [EXE]
    if dtype is not None:
        sc = T.scales(T.IMAGENET[1])
        args += ["--dtype", dtype, "--mean", ",".join(float(np.float32(v)).hex() for v in T.IMAGENET[0]), "--scale", ",".join(float(v).hex() for v in sc)]
    args += [*dst, fourcc, planes, int(norm), *border, src, w, h, pitch]
    for hm in hs:
        args += [float(np.float32(v)).hex() for v in hm]
    rc, lines, tails = run_check(args)
    assert len(lines) == len(hs), (rc, *tails)
    for (idx, crc, nbytes), hm in zip(lines, hs):
        ref = P.expected(oracle, y, uv, w, h, hm, dst, fourcc, planes, norm, None if border[0] < 0 else border)
        if dtype is not None:
            ref = T.expected(ref.view(np.float32), 3, T.IMAGENET, dtype)
        assert int(nbytes) == ref.size
        assert int(crc) == zlib.crc32(ref.tobytes()), f"output {idx} h={hm} -> {dst}"
    # (after the outputs the program asks for a homography of a frame it did not give: refused with VREADER_ERROR; exit code 0 = all of it held)
    assert rc == 0, (rc, *tails)
