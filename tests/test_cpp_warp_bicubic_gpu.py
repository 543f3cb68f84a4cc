"""GPU: VideoProcessor::ConvertWarpBicubic and ConvertPerspectiveBicubic of the C++ class (tensor-stream_amd/cpp/VideoProcessor.h) through the check programs
vpp_warp --bicubic and vpp_persp --bicubic: the CRC-32 each prints per output (zlib's, over the device result) equals zlib.crc32 of the expected output
(tests/warp_bicubic_util.py: the contract of tsvpp_convert_warp_bicubic / tsvpp_convert_perspective_bicubic).  One run per program without a spec and one with."""
import os
import zlib

import numpy as np
import pytest

import coord_paths as cp
import tensor_util as T
import warp_bicubic_util as B
import warp_util as W
from cpp_check import run_check, write_nv12
from util import synth_nv12

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tensor-stream_amd", "lib")

GEO = (322, 182, 384)


def items(program, dst):
    w, h, _ = GEO
    if program == "vpp_warp":
        ms = cp.matrices(w, h, *dst)
        return [W.scale_only(w, h, *dst), ms["rot30"], ms["left"], ms["up_shear"]]
    hs = cp.homographies(w, h, *dst)
    return [hs["strong"], hs["left"], hs["affine"]]


@pytest.mark.parametrize("dst,fourcc,planes,norm,border,dtype", [
    ((70, 66), 1, 1, False, (-1, -1, -1), None),        # RGB24 merged uint8, a width of the form 4 k + 2, replicate
    ((112, 112), 2, 0, True, (114, 128, 128), T.F16),   # BGR24 planar as fp16 with ImageNet mean / std, gray border: the overload with a spec
])
@pytest.mark.parametrize("program", ["vpp_warp", "vpp_persp"])
def test_crc_per_output(oracle, tmp_path, program, dst, fourcc, planes, norm, border, dtype):
    exe = os.path.join(LIB, program)
    assert os.path.exists(exe), f"{program} not built (python -c 'import __graft_entry__ as g; g.build()')"
    w, h, pitch = GEO
    y, uv = synth_nv12(w, h, seed=1700 + dst[0], pitch=pitch)
    src = tmp_path / "in.nv12"
    write_nv12(src, y, uv)
    cs = items(program, dst)
    args = [exe, "--bicubic"]
    if dtype is not None:
        sc = T.scales(T.IMAGENET[1])
        args += ["--dtype", dtype, "--mean", ",".join(float(np.float32(v)).hex() for v in T.IMAGENET[0]), "--scale", ",".join(float(v).hex() for v in sc)]
    args += [*dst, fourcc, planes, int(norm), *border, src, w, h, pitch]
    for c in cs:
        args += [float(np.float32(v)).hex() for v in c]
    rc, lines, tails = run_check(args)
    assert len(lines) == len(cs), (rc, *tails)
    for (idx, crc, nbytes), c in zip(lines, cs):
        ref = B.expected(oracle, y, uv, w, h, c, dst, fourcc, planes, norm, None if border[0] < 0 else border)
        if dtype is not None:
            ref = T.expected(ref.view(np.float32), 3, T.IMAGENET, dtype)
        assert int(nbytes) == ref.size
        assert int(crc) == zlib.crc32(ref.tobytes()), f"{program} output {idx} {c} -> {dst}"
    # (after the outputs the program asks for an item of a frame it did not give: refused with VREADER_ERROR; exit code 0 = all of it held)
    assert rc == 0, (rc, *tails)
