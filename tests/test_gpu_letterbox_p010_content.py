"""GPU: tsvpp_convert_letterbox_p010 on the boundary content of tests/p010_content.py -- flat frames whose blends land on c or c - 1, checker, edges, ramp -- bit for
bit against the model, for every class x geometry x mode x the four flavours of tests/test_gpu_letterbox_p010.py.  On random words a weight one ulp off flips one
sample in ~1e5; here 5 .. 12 % of the samples sit on the truncation boundary (tests/test_letterbox_p010_witness_cpu.py holds that)."""
import pytest
import torch

import p010_cases as P
import p010_content as C
import p010_util as M

pytestmark = pytest.mark.gpu

PAD = (940, 64, 960)
_virtual = {}


def pitches(g, w):
    """words: even geometries at the next multiple of 8 words above w (16-byte rows, 4-byte pairs), odd ones at w + 3 / w + 1 (a per-row phase, 2-byte pairs)"""
    return (w + 8 - w % 8, w + 8 - w % 8) if g % 2 == 0 else (w + 3, w + 1)


def resized(name, g, mode):
    """(frame, rectangle, the model's Y, U, V): computed once per (class, geometry, mode), shared by the flavours"""
    if (name, g, mode) not in _virtual:
        (w, h), canvas = C.GEOMETRIES[g]
        fr = C.frame(name, w, h, *pitches(g, w), seed=g)
        rect = P.rects_of([(w, h)], canvas)[0]
        _virtual[(name, g, mode)] = (fr, rect, M.virtual_frame(*fr, w, h, rect, canvas, mode, PAD))
    return _virtual[(name, g, mode)]


@pytest.mark.parametrize("flavour", P.FOUR)
@pytest.mark.parametrize("mode", [M.NEAREST, M.BILINEAR])
@pytest.mark.parametrize("name", C.CLASSES)
def test_boundary_content(vpp, name, mode, flavour):
    for g, ((w, h), canvas) in enumerate(C.GEOMETRIES):
        fr, rect, yuv = resized(name, g, mode)
        py, puv = pitches(g, w)
        planes = ([P.dev(fr[0]).as_strided((h, w), (py, 1))], [P.dev(fr[1]).as_strided((h // 2, w), (puv, 1))])
        got, used = P.convert(vpp, [fr], [(w, h)], canvas, mode, flavour, PAD, planes_dev=planes)
        torch.cuda.synchronize()
        assert tuple(used[0]) == rect
        P.same(got[0], P.stored(M.channels(*yuv, P.FLAVOURS[flavour][0]), flavour), f"{name} {w} x {h} (pitches {py} / {puv} words) -> {canvas} rect {rect} mode={mode} {flavour}")
