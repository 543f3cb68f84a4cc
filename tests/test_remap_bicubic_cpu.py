"""CPU: the host side of the BICUBIC map calls -- footprint, LDS hint, describe line, refusals -- and their model (tests/remap_bicubic_util.py) against its float64
judge (tests/sampler64_cubic.py on tests/sampler64.py's map positions)."""
import ctypes

import numpy as np
import pytest

import remap_bicubic_util as RB
import remap_util as R
import sampler64 as S
import sampler64_cubic as C
from letterbox_util import BGR24, BICUBIC, PLANAR
from util import synth_nv12

DSTS = [(70, 66), (30, 34)]


@pytest.mark.parametrize("dst", DSTS)
@pytest.mark.parametrize("geo", C.FRAMES)
def test_footprint_holds_every_tap_and_sizes_the_hint(geo, dst):
    from tensor_stream import _native
    lib = _native.lib()
    w, h, _ = geo
    maps = R.map_set(w, h, *dst)
    for name in ("barrel", "affine30", "far", "garbage"):
        xy = maps[name]
        ptr = xy.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        boxes = []
        for vec in (False, True):
            for tile in R.tiles(*dst, vec):
                out8 = (ctypes.c_int32 * 8)()
                assert lib.tsvpp_remap_bicubic_footprint(ptr, 0, *dst, w, h, *tile, out8) == 0
                box, (hull, formula) = tuple(out8), RB.tile_boxes(xy, w, h, tile)
                assert box == formula, (name, tile)
                assert all(box[a] <= hull[a] and hull[a + 1] <= box[a + 1] for a in (0, 2, 4, 6)), (name, tile, box, hull)
                boxes.append(box)
        for luma_only in (False, True):
            assert lib.tsvpp_remap_bicubic_lds_need(ptr, 0, *dst, w, h, int(luma_only)) == max(R.lds_need(b, luma_only) for b in boxes), (name, luma_only)


@pytest.mark.parametrize("dst", DSTS)
def test_describe_names_the_kernels_and_only_bicubic_is_taken(dst):
    import tensor_stream as ts
    import torch
    geo = [C.FRAMES[0]]

    def fp(rt):
        return ts.FrameParameters(width=dst[0], height=dst[1], resize_type=rt, pixel_format=BGR24, planes_pos=PLANAR, normalization=True)
    for name in ("remap", "mesh"):
        cubic, plain, tables = getattr(ts, f"describe_{name}_bicubic"), getattr(ts, f"describe_{name}"), [(0, 0)]  # (pitch, hint): no table is read
        d = cubic(fp(BICUBIC), geo, tables)
        assert d["mode"] == f"{name}_bicubic" and d["kernel"].startswith(f"vpp_{name}_bicubic<O_F32_PLANAR,"), d
        assert cubic(fp(BICUBIC), geo, tables, dtype=torch.float16)["kernel"].startswith(f"vpp_{name}_bicubic_tensor<PLANAR,EL_HALF,")
        for call, rt in [(plain, BICUBIC)] + [(cubic, rt) for rt in (0, 1, 3)]:  # the BILINEAR call keeps refusing BICUBIC; NEAREST, BILINEAR, AREA
            with pytest.raises(RuntimeError, match="-2"):
                call(fp(rt), geo, tables)


@pytest.mark.parametrize("border", C.BORDERS)
@pytest.mark.parametrize("dst", DSTS)
@pytest.mark.parametrize("k", range(len(C.FRAMES)))
def test_model_lies_inside_the_float64_bracket(k, dst, border):
    w, h, pitch = C.FRAMES[k]
    y, uv = synth_nv12(w, h, seed=1700 + k, pitch=pitch)
    maps = R.map_set(w, h, *dst)
    for name in ("affine30", "barrel"):
        vb = C.virtual_bracket(y, uv, w, h, S.remap_positions(maps[name]), border)
        assert S.holds(vb, *RB.virtual_frame_from_map(y, uv, w, h, maps[name], border)) == 0, (name, sum(vb.two), sum(vb.size))
