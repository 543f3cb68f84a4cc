"""GPU: VideoProcessor::ConvertMesh of the C++ class (tensor-stream_amd/cpp/VideoProcessor.h) through its check program vpp_mesh: the CRC-32 it prints per output
(zlib's, over the device result) equals zlib.crc32 of the expected output (tests/mesh_util.py's E(mesh) through tests/remap_util.py: the contract of
tsvpp_convert_mesh)."""
import os
import zlib

import numpy as np
import pytest

import mesh_util as M
import remap_util as R
import tensor_util as T
from cpp_check import run_check, write_nv12
from util import synth_nv12

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tensor-stream_amd", "lib", "vpp_mesh")

GEO = (322, 182, 384)
NAMES = ("barrel", "affine30", "far", "garbage")


@pytest.mark.parametrize("dst,cell,fourcc,planes,norm,border,dtype", [
    ((70, 66), (16, 8), 1, 1, False, (-1, -1, -1), None),         # RGB24 merged uint8, a width of the form 4 k + 2, replicate
    ((112, 112), (4, 32), 2, 0, True, (114, 128, 128), None),     # BGR24 planar fp32, gray border
    ((112, 112), (16, 16), 2, 0, True, (114, 128, 128), T.F16),   # ... as fp16 with ImageNet mean / std, through the overload with a spec
])
def test_crc_per_output(oracle, tmp_path, dst, cell, fourcc, planes, norm, border, dtype):
    assert os.path.exists(EXE), "vpp_mesh not built (python -c 'import __graft_entry__ as g; g.build()')"
    w, h, pitch = GEO
    y, uv = synth_nv12(w, h, seed=1800 + dst[0], pitch=pitch)
    src = tmp_path / "in.nv12"
    write_nv12(src, y, uv)
    ms = M.mesh_set(w, h, *dst, cell)
    files = []
    for name in NAMES:
        files.append(tmp_path / f"{name}.f32")
        ms[name].tofile(files[-1])
    args = [EXE]
    if dtype is not None:
        sc = T.scales(T.IMAGENET[1])
        args += ["--dtype", dtype, "--mean", ",".join(float(np.float32(v)).hex() for v in T.IMAGENET[0]), "--scale", ",".join(float(v).hex() for v in sc)]
    args += [*dst, fourcc, planes, int(norm), *border, src, w, h, pitch, M.log2(cell[0]), M.log2(cell[1]), *files]
    rc, lines, tails = run_check(args)
    assert len(lines) == len(NAMES), (rc, *tails)
    for (idx, crc, nbytes), name in zip(lines, NAMES):
        ref = R.expected(oracle, y, uv, w, h, M.expand(ms[name], *dst, cell), fourcc, planes, norm, None if border[0] < 0 else border)
        if dtype is not None:
            ref = T.expected(ref.view(np.float32), 3, T.IMAGENET, dtype)
        assert int(nbytes) == ref.size
        assert int(crc) == zlib.crc32(ref.tobytes()), f"output {idx} mesh {name} cell {cell} -> {dst}"
    # (after the outputs the program asks for a mesh index it did not give: refused with VREADER_ERROR; exit code 0 = all of it held)
    assert rc == 0, (rc, *tails)
