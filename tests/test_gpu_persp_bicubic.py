"""GPU: tsvpp_convert_perspective_bicubic -- homography-warped outputs sampled with the library's BICUBIC, one launch per 32 outputs.

The contract (include/tsvpp.h): the output is, bit for bit, what the oracle's conversion WITHOUT a resize returns for the virtual NV12 frame that the stated
coordinate, edge rule and cubic sums sample (tests/warp_bicubic_util.py: a numpy restatement, checked on the CPU in tests/test_warp_bicubic_cpu.py against the
oracle and against its float64 judge, tests/sampler64_cubic.py).  Every comparison is np.array_equal on the raw bits or, for the judge, a bracket per element.
The cases every coordinate path has are tests/coord_suite.py's, run on the descriptor PERSP_BICUBIC of tests/coord_bicubic_paths.py, which also holds the bodies of
the cases the two BICUBIC calls share."""
import numpy as np
import pytest
import torch

import coord_bicubic_paths as cb
import coord_suite as cs
import coord_paths as cp
import persp_util as P
import warp_util as W
from coord_bicubic_paths import PERSP_BICUBIC as PATH, PERSP_PICKS as PICKS
from letterbox_util import BGR24, BICUBIC, PLANAR, bits

pytestmark = pytest.mark.gpu

frames = cs.frames_fixture(1600)      # the suite's frames, for its shared cases
frames3 = cb.frames_fixture(1600 + 5)  # 322 x 182, 32 x 18 and 4 x 2, for the bits


@pytest.mark.parametrize("dst", cb.DSTS)
def test_bits_against_the_model_and_inside_the_float64_bracket(vpp, oracle, frames3, dst):
    cb.bits_and_bracket(PATH, PICKS, vpp, oracle, frames3, dst)


@pytest.mark.parametrize("dst", cb.DSTS)
def test_scale_only_is_convert_bicubic_and_the_oracle(vpp, oracle, frames3, dst):
    cb.scale_only_is_convert_bicubic(PATH, lambda w, h, dw, dh: P.affine(W.scale_only(w, h, dw, dh)), vpp, oracle, frames3, dst)


def test_last_row_0_0_1_gives_the_bits_of_the_affine_call(vpp, frames3):
    """h = (m0 .. m5, 0, 0, 1): nw = rw = 1 and nx * 1 is exact -- the call stores the bits of convert_warp_bicubic with m, border included"""
    import tensor_stream as ts
    host, dev = frames3
    dst = (70, 66)
    ms = [(k, m) for k, (w, h, _) in enumerate(cb.GEO) for m in cp.matrices(w, h, *dst).values()]
    fp = cs.params(ts, dst, BGR24, PLANAR, True, rt=BICUBIC)
    kw = dict(width=[g[0] for g in cb.GEO], height=[g[1] for g in cb.GEO])
    ys, uvs = [d[0] for d in dev], [d[1] for d in dev]
    for border in (None, (3, 250, 7)):
        a = vpp.convert_warp_bicubic(ys, uvs, [(k,) + m for k, m in ms], fp, border=border, **kw)
        b = vpp.convert_perspective_bicubic(ys, uvs, [(k,) + P.affine(m) for k, m in ms], fp, border=border, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(bits(a), bits(b)), border


def test_a_homography_and_four_times_it_give_the_same_bits(vpp, frames3):
    """every operation of the coordinate scales exactly by 4"""
    import tensor_stream as ts
    host, dev = frames3
    dst = (112, 112)
    qs = [(k, q) for k, (w, h, _) in enumerate(cb.GEO) for n, q in cp.homographies(w, h, *dst).items() if n in ("mild", "strong", "keyrot", "left")]
    fp = cs.params(ts, dst, BGR24, PLANAR, True, rt=BICUBIC)
    kw = dict(width=[g[0] for g in cb.GEO], height=[g[1] for g in cb.GEO], border=(3, 250, 7))
    ys, uvs = [d[0] for d in dev], [d[1] for d in dev]
    a = vpp.convert_perspective_bicubic(ys, uvs, [(k,) + q for k, q in qs], fp, **kw)
    b = vpp.convert_perspective_bicubic(ys, uvs, [(k,) + tuple(4.0 * v for v in q) for k, q in qs], fp, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(bits(a), bits(b))


def test_edge_content_classes(vpp, oracle):
    cb.edge_content_classes(PATH, lambda w, h, dw, dh: [cp.homographies(w, h, dw, dh)[n] for n in ("strong", "affine")], vpp, oracle)


def test_seeded_fuzz_chunk(vpp, oracle):
    cb.fuzz_chunk(PATH, cb.draw_homography, vpp, oracle, seed=1600 + 40)


def test_staged_gather_and_mixed_launches(oracle, frames, monkeypatch):
    cs.staged_gather_and_mixed_launches(PATH, oracle, frames, monkeypatch)


def test_splitting_over_launches_at_33_items(vpp, oracle, frames):
    cs.splitting_over_launches(PATH, vpp, oracle, frames, PATH.LIMIT + 1)


@pytest.mark.parametrize("dst", cs.GUARD_DSTS)
@pytest.mark.parametrize("fcc,planes,norm,off", cs.GUARD_FLAVOURS[1:5])  # fp32 planar + 4, fp32 merged + 4, uint8 merged + 0 and + 1
def test_unaligned_outputs_and_guard_bytes(vpp, oracle, frames, fcc, planes, norm, off, dst):
    cs.unaligned_outputs_and_guard_bytes(PATH, vpp, oracle, frames, fcc, planes, norm, off, dst)


@pytest.mark.parametrize("g_term,ct_bits", [(1, 0), (2, 2048)])
def test_colour_g_term_variants(oracle, frames, g_term, ct_bits):
    cs.colour_g_term_variants(PATH, oracle, frames, g_term, ct_bits)


def test_graph_capture_replays_bit_exact(vpp, oracle):
    cs.graph_capture_replays(PATH, vpp, oracle, seed=1600 + 10)


def test_refusals_with_a_live_context(vpp, frames):
    cb.live_refusals(PATH, "perspective", vpp, frames)
