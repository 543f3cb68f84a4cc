"""GPU: tsvpp_convert_warp_bicubic -- rotated and affine-warped boxes sampled with the library's BICUBIC, one launch per 32 outputs.

The contract (include/tsvpp.h): the output is, bit for bit, what the oracle's conversion WITHOUT a resize returns for the virtual NV12 frame that the stated
coordinate, edge rule and cubic sums sample (tests/warp_bicubic_util.py: a numpy restatement, checked on the CPU in tests/test_warp_bicubic_cpu.py against the
oracle and against its float64 judge, tests/sampler64_cubic.py).  Every comparison is np.array_equal on the raw bits or, for the judge, a bracket per element.
The cases every coordinate path has are tests/coord_suite.py's, run on the descriptor WARP_BICUBIC of tests/coord_bicubic_paths.py, which also holds the bodies of
the cases the two BICUBIC calls share."""
import numpy as np
import pytest
import torch

import coord_bicubic_paths as cb
import coord_suite as cs
import coord_paths as cp
import warp_util as W
from coord_bicubic_paths import WARP_BICUBIC as PATH, WARP_PICKS as PICKS
from letterbox_util import BGR24, BICUBIC, PLANAR, bits

pytestmark = pytest.mark.gpu

frames = cs.frames_fixture(1500)      # the suite's frames, for its shared cases
frames3 = cb.frames_fixture(1500 + 5)  # 322 x 182, 32 x 18 and 4 x 2, for the bits


@pytest.mark.parametrize("dst", cb.DSTS)
def test_bits_against_the_model_and_inside_the_float64_bracket(vpp, oracle, frames3, dst):
    cb.bits_and_bracket(PATH, PICKS, vpp, oracle, frames3, dst)


@pytest.mark.parametrize("dst", cb.DSTS)
def test_scale_only_is_convert_bicubic_and_the_oracle(vpp, oracle, frames3, dst):
    cb.scale_only_is_convert_bicubic(PATH, W.scale_only, vpp, oracle, frames3, dst)


def test_identity_fp32_spec_is_the_plain_call(vpp, frames):
    """mean 0, std 1, float32: the entry point with a spec stores the bits it stores without one"""
    cs.identity_fp32_is_the_plain_call(PATH, vpp, frames, PATH.pick([(2, "rot30"), (3, "left")], cs.GEO, (70, 66)), (70, 66))


def test_edge_content_classes(vpp, oracle):
    cb.edge_content_classes(PATH, lambda w, h, dw, dh: [cp.matrices(w, h, dw, dh)[n] for n in ("rot30", "up_shear")], vpp, oracle)


def test_seeded_fuzz_chunk(vpp, oracle):
    cb.fuzz_chunk(PATH, cb.draw_matrix, vpp, oracle, seed=1500 + 40)


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
    cs.graph_capture_replays(PATH, vpp, oracle, seed=1500 + 10)


def test_refusals_with_a_live_context(vpp, frames):
    cb.live_refusals(PATH, "warp", vpp, frames)
