"""GPU: tsvpp_convert_remap_bicubic against the model (tests/remap_bicubic_util.py: the contract of include/tsvpp.h), bit for bit; and the cases every
coordinate path has (tests/coord_suite.py) for both BICUBIC map calls, on the descriptors of tests/map_bicubic_paths.py."""
import numpy as np
import pytest
import torch

import coord_paths as cp
import coord_suite as cs
import remap_util as R
import sampler64 as S
import sampler64_cubic as C
import tensor_util as T
import warp_util as W
from coord_bicubic_paths import BORDERS, TENSORS, frames_fixture
from letterbox_util import BGR24, BICUBIC, FLAVOURS, MERGED, PLANAR, RGB24, Y800, bits
from map_bicubic_paths import MESH_BICUBIC, REMAP_BICUBIC as PATH

pytestmark = pytest.mark.gpu

GEO = C.FRAMES  # 322 x 182 (pitch 384), 32 x 18 (pitch 48), 4 x 2: every upper tap collapses, the chroma plane is 2 x 1 pairs
NAMES = ("barrel", "affine30", "far", "garbage")
JUDGED = ((BGR24, PLANAR, True), (RGB24, MERGED, False))  # fp32 and uint8: the flavours held to the float64 judge's bracket
frames = cs.frames_fixture(1800)
frames3 = frames_fixture(1800 + 5)  # the frames of GEO


@pytest.mark.parametrize("dst", C.DSTS)
def test_bits_against_the_model_and_inside_the_float64_bracket(vpp, oracle, frames3, dst):
    """every frame through its four maps -- garbage holds NaN, both infinities and subnormals; the first and the last map travel pitch-padded with NaN -- in
    every colour flavour and three tensor forms, replicate and a border; the finite maps' fp32 and uint8 results inside the judge's bracket, every element"""
    import tensor_stream as ts
    host, dev = frames3
    items = cp.remap_pick([(k, nm) for k in range(len(GEO)) for nm in NAMES], GEO, dst)
    items.dev = [cp.padded_to_device(t) if m in (0, len(items.tables) - 1) else cs.to_device(t) for m, (_, t) in enumerate(items.tables)]
    kw = dict(width=[g[0] for g in GEO], height=[g[1] for g in GEO])
    forms = [(f, None, None) for f in FLAVOURS] + [((fcc, planes, True), dt, sp) for dt, sp, fcc, planes in TENSORS]
    for border in BORDERS:
        for f, dt, sp in forms:
            spec = {} if dt is None else dict(dtype=T.TORCH[dt], mean=T.SPECS[sp][0], std=T.SPECS[sp][1])
            got = PATH.call(vpp, [d[0] for d in dev], [d[1] for d in dev], items, cs.params(ts, dst, *f), border=border, **kw, **spec)
            torch.cuda.synchronize()
            for i, (k, m) in enumerate(items.remaps):
                name, xy = items.tables[m]
                ref = PATH.expected(oracle, xy, dst, *f, border, cs.virtual(PATH, host, k, GEO, xy, name, dst, border))
                ref = ref if dt is None else T.expected(ref.view(np.float32), 1 if f[0] == Y800 else 3, T.SPECS[sp], dt)
                assert np.array_equal(T.bits(got[i]), ref), (name, dst, f, dt, sp, border)
                if dt is None and f in JUDGED and name.split("@")[0] in ("barrel", "affine30"):
                    vb = C.virtual_bracket(host[k][0], host[k][1], *GEO[k][:2], S.remap_positions(xy), border)
                    lo, hi = S.output_bracket(oracle, vb, *f)
                    assert S.outside(got[i].cpu().numpy().ravel().view(lo.dtype), lo, hi).size == 0, (name, dst, border, f)


@pytest.mark.parametrize("fcc,planes,norm", [(BGR24, PLANAR, True), (RGB24, MERGED, False)])
def test_identities_against_convert(vpp, frames, frames3, fcc, planes, norm):
    """the identity map is Convert without a resize; the maps of the exact ratios 2 : 1 and 1 : 2 are Convert(BICUBIC); an even translation is the crop"""
    import tensor_stream as ts
    flavour = dict(pixel_format=fcc, planes_pos=planes, normalization=norm)
    one = [(frames[1][0], cs.GEO[0]), *zip(frames3[1], GEO)]  # 128 x 72, then 322 x 182, 32 x 18, 4 x 2 (there every tap sits at an edge)
    cases = [(k, (w, h), R.identity(w, h), dict()) for k, (_, (w, h, _)) in enumerate(one)]
    for k, r in ((0, 2), (0, 0.5), (3, 0.5)):
        dst = (int(one[k][1][0] / r), int(one[k][1][1] / r))
        cases.append((k, dst, R.exact_ratio(*dst, r), dict(width=dst[0], height=dst[1], resize_type=BICUBIC)))
    cases.append((0, (70, 34), R.translation(70, 34, 20, 6), dict(crop_coords=(20, 6, 90, 40))))
    for k, dst, xy, convert in cases:
        (y, uv), (w, h, _) = one[k]
        fp = ts.FrameParameters(width=dst[0], height=dst[1], resize_type=BICUBIC, **flavour)
        for border in (None, (114, 128, 128)):
            got = vpp.convert_remap_bicubic(y, uv, cs.to_device(xy), fp, border=border, width=w, height=h)
            ref = vpp.Convert(y, uv, ts.FrameParameters(**convert, **flavour), width=w, height=h)
            torch.cuda.synchronize()
            assert np.array_equal(bits(got[0]), bits(ref)), (w, h, dst, convert, border)


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("dst", C.DSTS)
def test_affine_luma_coordinates_give_the_warp_calls_y800(vpp, frames3, dst, norm):
    import tensor_stream as ts
    fp = ts.FrameParameters(width=dst[0], height=dst[1], resize_type=BICUBIC, pixel_format=Y800, planes_pos=MERGED, normalization=norm)
    for (y, uv), (w, h, _) in zip(frames3[1], GEO):
        for name in ("rot30", "up_shear", "left"):
            m = cp.matrices(w, h, *dst)[name]
            xy = R.stack(*W.coords(m, *W.translations(m)[:2], np.arange(dst[1]), np.arange(dst[0])))
            for border in BORDERS:
                a = vpp.convert_remap_bicubic(y, uv, cs.to_device(xy), fp, border=border, width=w, height=h)
                b = vpp.convert_warp_bicubic(y, uv, [m], fp, border=border, width=w, height=h)
                torch.cuda.synchronize()
                assert np.array_equal(bits(a), bits(b)), (w, h, dst, name, border)


@pytest.mark.parametrize("path", [PATH, MESH_BICUBIC], ids=["remap", "mesh"])
def test_staging_runs_splitting_at_33_items_and_capture_with_table_updates(vpp, oracle, frames, monkeypatch, path):
    cs.staged_gather_and_mixed_launches(path, oracle, frames, monkeypatch)  # TSVPP_LDS_KB default / 0 / 3, the BILINEAR hint, the BICUBIC hint: the same bits
    cs.splitting_over_launches(path, vpp, oracle, frames, path.LIMIT + 1)
    cs.graph_capture_replays(path, vpp, oracle, seed=1800 + 10)
