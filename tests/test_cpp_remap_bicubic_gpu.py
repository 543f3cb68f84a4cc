"""GPU: VideoProcessor::ConvertBicubicRemap / ConvertBicubicMesh through vpp_remap --bicubic and vpp_mesh --bicubic: the CRC-32 printed per output is that of the
model's output (tests/remap_bicubic_util.py; a mesh's is its expansion's), as tests/test_cpp_warp_bicubic_gpu.py does.  One run without a spec, one with."""
import os
import zlib

import numpy as np
import pytest

import mesh_util as M
import remap_bicubic_util as RB
import remap_util as R
import tensor_util as T
from cpp_check import run_check, write_nv12
from util import synth_nv12

pytestmark = pytest.mark.gpu
LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tensor-stream_amd", "lib")
NAMES = ("barrel", "affine30", "far", "garbage")
CELL = (16, 8)


@pytest.mark.parametrize("dst,fourcc,planes,norm,border,dtype", [
    ((70, 66), 1, 1, False, (-1, -1, -1), None),        # RGB24 merged uint8, a width of the form 4 k + 2, replicate
    ((112, 112), 2, 0, True, (114, 128, 128), T.F16),   # BGR24 planar as fp16 with ImageNet mean / std, gray border: the overload with a spec
])
@pytest.mark.parametrize("program", ["vpp_remap", "vpp_mesh"])
def test_crc_per_output(oracle, tmp_path, program, dst, fourcc, planes, norm, border, dtype):
    exe = os.path.join(LIB, program)
    assert os.path.exists(exe), f"{program} not built (python -c 'import __graft_entry__ as g; g.build()')"
    w, h, pitch = 322, 182, 384
    y, uv = synth_nv12(w, h, seed=1750 + dst[0], pitch=pitch)
    write_nv12(tmp_path / "in.nv12", y, uv)
    mesh = program == "vpp_mesh"
    tables = M.mesh_set(w, h, *dst, CELL) if mesh else R.map_set(w, h, *dst)
    for name in NAMES:
        tables[name].tofile(tmp_path / f"{name}.f32")
    spec = [] if dtype is None else ["--dtype", dtype, "--mean", ",".join(float(np.float32(v)).hex() for v in T.IMAGENET[0]),
                                     "--scale", ",".join(float(v).hex() for v in T.scales(T.IMAGENET[1]))]
    rc, lines, tails = run_check([exe, "--bicubic", *spec, *dst, fourcc, planes, int(norm), *border, tmp_path / "in.nv12", w, h, pitch,
                                  *([M.log2(CELL[0]), M.log2(CELL[1])] if mesh else []), *[tmp_path / f"{name}.f32" for name in NAMES]])
    assert len(lines) == len(NAMES), (rc, *tails)
    for (idx, crc, nbytes), name in zip(lines, NAMES):
        xy = M.expand(tables[name], *dst, CELL) if mesh else tables[name]
        ref = R.expected(oracle, None, None, 0, 0, None, fourcc, planes, norm, virtual=RB.virtual_frame_from_map(y, uv, w, h, xy, None if border[0] < 0 else border))
        ref = ref if dtype is None else T.expected(ref.view(np.float32), 3, T.IMAGENET, dtype)
        assert int(nbytes) == ref.size and int(crc) == zlib.crc32(ref.tobytes()), f"{program} output {idx} {name} -> {dst}"
    assert rc == 0, (rc, *tails)  # (after the outputs the program asks for a table it did not give: refused with VREADER_ERROR; 0 = all of it held)
