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


def test_table_constants_are_the_headers():
    import os
    import re
    text = open(os.path.join(G.ROOT, "include", "tsvpp.h")).read()
    assert int(re.search(r"#define\s+TSVPP_MAX_BATCH\s+(\d+)", text).group(1)) == G.MAX_BATCH
    assert int(re.search(r"#define\s+TSVPP_MAX_TABLE_LAUNCH\s+(\d+)", text).group(1)) == G.MAX_TABLE_LAUNCH
    assert G.TABLE_N_WANTED == G.MAX_TABLE_LAUNCH + 1 and G.TABLE_N_MIN == G.MAX_BATCH + 3
    # the pool's period shares no factor with the XCD count or the kernarg table's length: a wrapped or permuted frame index reads another frame
    assert G.TABLE_POOL % 2 == 1 and G.MAX_BATCH % G.TABLE_POOL != 0 and 8 % G.TABLE_POOL != 0


def test_every_family_has_table_candidates_and_the_choice_is_deterministic(sigs):
    """the signatures tests/test_gpu_dispatch_cover.py converts out of tables of more than TSVPP_MAX_BATCH entries: every family but "(none)" has some"""
    cands = G.table_candidates()
    assert set(cands) == set(G.FAMILIES) - {"(none)"}
    G._CACHE.pop("table")
    again = G.table_candidates()
    assert again == cands and [list(v) for v in again.values()] == [list(v) for v in cands.values()]
    reached = {G.family(s) for s in sigs}
    empty = [f for f in cands if not cands[f] and not (knob_run() and f not in reached)]  # (under A/B knobs a family the grid no longer reaches has none)
    assert not empty, f"families without a signature that fits a table launch of {G.TABLE_N_MIN}+ frames into {G.MAX_DEVICE_BYTES} bytes: {empty}"
    for fam, lst in cands.items():
        assert len(lst) <= G.TABLE_PER_FAMILY and len({s for s, _, _ in lst}) == len(lst)
        kinds = [G.out_kind(s) for s, _, _ in lst]
        fresh = [k not in kinds[:i] for i, k in enumerate(kinds)]
        assert fresh == sorted(fresh, reverse=True), (fam, kinds)  # distinct out= kinds first, repeats only behind them
        sizes = [G.out_bytes(G.representative(s)) for (s, _, _), f in zip(lst, fresh) if f]
        assert sizes == sorted(sizes), (fam, kinds, sizes)         # ... the fewest output bytes first
        for sig, n_big, cap in lst:
            req = G.representative(sig)
            assert sig in sigs and G.family(sig) == fam and " pass2=" not in sig
            assert G.TABLE_N_MIN <= n_big <= G.TABLE_N_WANTED and cap >= G.TABLE_N_MIN, (sig, n_big, cap)
            assert n_big * G.out_bytes(req) + G.pool_bytes(req) <= G.MAX_DEVICE_BYTES, (sig, n_big)
            # n_big is the largest count that fits, up to the wanted one
            assert n_big == G.TABLE_N_WANTED or (n_big + 1) * G.out_bytes(req) + G.pool_bytes(req) > G.MAX_DEVICE_BYTES, (sig, n_big)


def test_table_launch_cap_is_convert_impls():
    assert G.table_launch_cap(1280, 720) == 1024 and G.table_launch_cap(1920, 1080) == 1024   # 3 600 / 8 100 workgroups a frame
    assert G.table_launch_cap(2560, 1440) == (1 << 23) // (40 * 360) == 582
    assert G.table_launch_cap(3840, 2160) == 258 and G.table_launch_cap(5760, 3240) == 128   # (115 would be less than a kernarg launch takes)


def test_the_misaligned_table_case_exists(sigs):
    """with the default knobs and under every A/B knob: the GPU test never stands down for want of a case"""
    case = G.table_unaligned_case()
    assert case is not None, "no single-pass fp32 planar signature fits a table launch of 1024 + 128 frames"
    sig, req, unaligned_kernel = case
    assert sig in sigs and req == G.representative(sig) and " pass2=" not in sig
    assert G.out_kind(sig) == "f32_planar" and sig.endswith(" aligned=1") and unaligned_kernel.startswith("vpp_")
    assert (G.MAX_TABLE_LAUNCH + G.MAX_BATCH) * (G.out_bytes(req) + 4) + G.pool_bytes(req) <= G.MAX_DEVICE_BYTES
    if not knob_run():  # (a knob may leave one kernel for both alignment classes, TSVPP_FORCE_GATHER=1: the defaults do not)
        assert unaligned_kernel != G.kernel_name(sig), f"no fp32 planar signature whose kernel depends on the output alignment: {sig}"
    assert G.table_unaligned_case() == case
