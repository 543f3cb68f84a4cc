"""CPU: the request grid of tests/dispatch_grid.py reaches every kernel the launchers can name, and every kernel family the GPU coverage test
(tests/test_gpu_dispatch_cover.py) runs.  A kernel instance that no request of the grid reaches is listed below with the request or knob that reaches it,
or why it stays although nothing does."""

import pytest

import dispatch_grid as G
from util import knob_run

# {kernel name as describe spells it: why the grid does not reach it}
UNREACHABLE = {
    "vpp_area_cols_kernel<1,32,OUT>": "TSVPP_AREA_COLS=2 only: by default the column-per-lane AREA kernel takes 5+ horizontal taps (nkx >= 2); one tap quad goes to vpp_area_direct_float_kernel<1>",
    "vpp_area_cols_kernel<1,8,OUT>": "TSVPP_AREA_COLS=2 only (as <1,32>)",
    "vpp_area_cols_kernel<3,32,OUT>": "TSVPP_AREA_COLS_ROWS=32 only: 9..12 horizontal taps get 8-row tiles by default (sel_area)",
    "vpp_area_direct_float_kernel<2,OUT>": "TSVPP_AREA_COLS=0 only: by default vpp_area_cols_kernel<2,*> takes every request with 5..8 horizontal taps",
    "vpp_area_direct_float_kernel<3,OUT>": "TSVPP_AREA_COLS=0 only: by default vpp_area_cols_kernel<3,*> takes every request with 9..12 horizontal taps",
    "vpp_areaf_kernel<3,3,OUT>": "dead with the default thresholds: 3 x 3 float taps means both ratios > 2 = area_direct_fmin, where the un-staged AREA kernels "
                                 "take over; kept because the staged float AREA kernel's dispatch instantiates its whole 2..3 x 2..3 family (A/B of area_direct_fmin)",
}
SIGNATURE_FLOOR = 3000  # what the finished grid reaches (3 044): a change to the grid or the selection that loses signatures shows up here
NAME_FLOOR = 67


@pytest.fixture(scope="module")
def sigs():
    return G.signatures()


def test_grid_reaches_every_kernel_name_or_says_why(sigs):
    literals = G.kernel_literals()
    assert len(literals) >= 70, sorted(literals)  # (the scrape itself works)
    reached = {G.kernel_name(s) for s in sigs}
    if knob_run():
        pytest.skip("knob runs route requests elsewhere on purpose: the exemptions are about the defaults")
    missing = literals - reached - set(UNREACHABLE)
    assert not missing, f"kernel names no request of the grid reaches and UNREACHABLE does not explain: {sorted(missing)}"
    stale = set(UNREACHABLE) & reached
    assert not stale, f"UNREACHABLE lists kernels the grid now reaches: {sorted(stale)}"
    unknown = set(UNREACHABLE) - literals
    assert not unknown, f"UNREACHABLE lists names no launcher reports: {sorted(unknown)}"
    assert len(literals & reached) >= NAME_FLOOR, len(literals & reached)
    assert reached - literals <= {"(none)"}, sorted(reached - literals)  # describe names nothing the scrape missed


def test_families_are_the_ones_the_gpu_test_runs(sigs):
    if knob_run():
        pytest.skip("knob runs route requests elsewhere on purpose")
    fams = {G.family(s) for s in sigs}
    assert fams == set(G.FAMILIES), (sorted(fams - set(G.FAMILIES)), sorted(set(G.FAMILIES) - fams))


def test_signature_floor(sigs):
    if knob_run():
        pytest.skip("knob runs route requests elsewhere on purpose")
    assert len(sigs) >= SIGNATURE_FLOOR, len(sigs)
    # every signature says whether its outputs are aligned, and both classes occur
    assert {s.rsplit(" ", 1)[1] for s in sigs} == {"aligned=0", "aligned=1"}


def test_representative_is_deterministic(sigs):
    for s in sorted(sigs)[::97]:
        a, b = G.representative(s), G.representative(s)
        assert a == b and a in sigs[s]
    # ... and the cheapest: no request of the signature moves fewer oracle bytes
    s = max(sigs, key=lambda k: len(sigs[k]))
    r = G.representative(s)
    assert all(G.oracle_bytes(r) <= G.oracle_bytes(q) for q in sigs[s])


def test_signature_drops_only_size_keys():
    answer = {"mode": "bilinear", "out": "f32_planar", "src": "1920x1080", "dst": "1280x720", "kernel": "k<OUT>", "shape": "32x8", "rpt": 1, "dma": 1,
              "lds": 100, "grid": 10, "tiles": "3x4", "frames": 64, "tail": 0, "geo": 0, "nt": 1, "staged": 1, "in4": 1}
    s = G.signature_of(answer, 0)
    for k in G.SIZE_KEYS:
        assert f" {k}=" not in f" {s}"
    for k in ("mode", "out", "kernel", "shape", "rpt", "dma", "tail", "geo", "nt", "staged", "in4", "aligned"):
        assert f" {k}=" in f" {s}", k


def test_enumeration_is_fast_enough(sigs):
    """the grid is enumerated once per process by both tests' fixtures (the module caches it): it must stay cheap -- ~9 s when this bound was set"""
    assert G._CACHE["seconds"] < 20, G._CACHE["seconds"]
