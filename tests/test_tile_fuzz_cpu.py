"""No GPU: the generators of tests/tile_fuzz.py reach what tests/test_gpu_tile_fuzz.py is there for.  Everything is asked of ts.describe_rois, describe_rois_area,
describe_letterbox, describe_warp and describe_perspective (host logic only), with aligned_outputs as drawn and with the tensor arguments where drawn: every drawn
call is accepted, few draws had to be repeated, and per family the calls name every kind of kernel, every edge of the geometry and both launch-group shapes."""
import pytest

import tile_fuzz as F
from util import knob_run

SAMPLERS = {"rois": ("M_NEAREST", "M_BILINEAR", "M_BICUBIC"), "letterbox": ("M_NEAREST", "M_BILINEAR", "M_BICUBIC")}  # (rois_area: per box, see below; warp, persp: one)
OUTS = {"u8_planar", "u8_merged", "f32_planar", "f32_merged", "y800_u8", "y800_f32"}
TENSOR_OUTS = ("f32n_", "f16_", "bf16_")  # out= of a tensor call starts with its element's name


@pytest.fixture(scope="module")
def drawn():
    """family -> [(call, describe line)] over its 8 chunks, and family -> the summed draw counts"""
    calls, stats = {}, {}
    for family in F.FAMILIES:
        calls[family], stats[family] = [], {}
        for chunk in range(F.CHUNKS):
            cs, st = F.generate(family, chunk)
            assert len(cs) == F.CALLS and all(c["seed"] == F.BASE_SEED + 8 * F.FAMILIES.index(family) + chunk for c in cs)
            for c in cs:
                calls[family].append((c, F.describe(c)))  # (a refused call raises here)
            for k, n in st.items():
                stats[family][k] = stats[family].get(k, 0) + n
    return calls, stats


@pytest.mark.parametrize("family", F.FAMILIES)
def test_every_call_is_accepted_and_few_draws_were_repeated(drawn, family):
    calls, stats = drawn
    st = stats[family]
    items = sum(len(c["items"]) for c, _ in calls[family])
    redraws = sum(n for k, n in st.items() if k != "draws")
    assert st["draws"] == items + redraws
    assert redraws <= 0.10 * st["draws"], st
    for c, d in calls[family]:
        n = len(c["items"])
        assert d["dst"] == "%dx%d" % c["dst"] and d["launches"] == (n + F.LIMIT[family] - 1) // F.LIMIT[family] and d["limit"] == F.LIMIT[family]
        assert 1 <= len(c["frames"]) <= 3 and (F.LIMIT[family] < n <= F.LIMIT[family] + 8 if c["split"] else 1 <= n <= 8)
        assert (c["tensor"] is None) or F.tensor_allowed(c["flavour"])


@pytest.mark.parametrize("family", F.FAMILIES)
def test_the_calls_are_the_same_every_time(family):
    for chunk in range(F.CHUNKS):
        assert F.cases(family, chunk) == F.cases(family, chunk)
    assert F.cases(family, 0) != F.cases(family, 1)


@pytest.mark.parametrize("family", F.FAMILIES)
def test_kernels_named(drawn, family):
    if knob_run():  # (replayed under A/B knobs: the selections are the knobs')
        return
    lines = [d for _, d in drawn[0][family]]
    names = {d["kernel"] for d in lines}
    assert any(",vec," in k for k in names) and any(",elem," in k for k in names)
    for mode in SAMPLERS.get(family, ()):
        assert any(mode in k for k in names), mode
    assert OUTS <= {d["out"] for d in lines}
    if family in ("warp", "persp"):
        assert any(k.endswith(",replicate>") for k in names) and any(k.endswith(",border>") for k in names)
    for el in TENSOR_OUTS:
        assert any(d["out"].startswith(el) and "_tensor<" in d["kernel"] for d in lines), el
    # half the tensor-capable calls, no others
    tensor = [c["tensor"] is not None for c, _ in drawn[0][family] if F.tensor_allowed(c["flavour"])]
    assert 0.3 * len(tensor) <= sum(tensor) <= 0.7 * len(tensor)


@pytest.mark.parametrize("family", F.FAMILIES)
def test_geometry_kinds(drawn, family):
    pairs = drawn[0][family]
    frames = [f for c, _ in pairs for f in c["frames"]]
    if not knob_run():
        assert any(d["tail"] == 2 for _, d in pairs)  # 4 k + 2 columns, at least a tile wide, aligned outputs: the shifted last tile column
    assert any(c["dst"][0] == 2 for c, _ in pairs) and any(c["dst"][1] == 2 for c, _ in pairs)
    assert any(d["launches"] == 2 for _, d in pairs)
    assert any(d["tiles"] == "1x1" for _, d in pairs) and any(d["tiles"] != "1x1" for _, d in pairs)  # one-tile grids and larger ones
    assert any(f["w"] <= 8 and f["h"] <= 8 for f in frames)
    assert any(f["pitch_y"] % 16 != 0 for f in frames)
    assert any(f["pitch_uv"] % 16 != 0 and f["pitch_uv"] != f["pitch_y"] for f in frames)
    assert any(f["off_y"] != 0 for f in frames) and any(f["off_uv"] != 0 for f in frames)
    assert {c["placement"] for c, _ in pairs} == {"aligned", "unaligned", "mixed"}


@pytest.mark.parametrize("family", F.FAMILIES)
def test_a_split_call_runs_a_vector_and_an_element_wise_kernel(drawn, family):
    """one call per chunk: two launch groups, the first with aligned outputs, the second without (tile_convert chooses the store kernel per launch group)"""
    split = [c for c, _ in drawn[0][family] if c["split"]]
    assert len(split) == F.CHUNKS
    for c in split:
        n, limit = len(c["items"]), F.LIMIT[family]
        assert c["placement"] == "mixed" and max(c["dst"]) <= 16
        starts, total = F.slot_starts(c)
        assert all(s % 16 == 0 for s in starts[:limit]) and all(s % 16 == F.element_bytes(c) for s in starts[limit:])
        assert all(b - a >= F.output_bytes(c) + F.GUARD for a, b in zip(starts, starts[1:] + [total]))
        first, second = F.describe(c, aligned_outputs=True), F.describe(c, aligned_outputs=False)
        assert first["launches"] == 2
        if not knob_run():
            assert ",vec," in first["kernel"] and ",elem," in second["kernel"]


def test_area_boxes(drawn):
    pairs = drawn[0]["rois_area"]
    assert any(d["launches"] == 1 and 0 < d["down"] < d["rois"] for _, d in pairs)  # both rules in one launch
    assert any(d["down"] == d["rois"] for _, d in pairs) and any(d["down"] == 0 for _, d in pairs)
    taps = [max(tx, ty) for c, _ in pairs for it in c["items"] for down, tx, ty in [F.area_taps(it[1:], c["dst"])] if down]
    assert all(t <= F.MAX_TAPS for t in taps)
    assert any(33 <= t <= 40 for t in taps) and any(t == 40 for t in taps)
    for c, d in pairs:
        assert d["down"] == sum(F.area_taps(it[1:], c["dst"])[0] for it in c["items"])


def test_matrix_kinds(drawn):
    """warp: the four translation kinds in turn; persp: every eighth entry is affine (h6 = h7 = 0, h8 = 1), the others are not"""
    persp = [it for c, _ in drawn[0]["persp"] for it in c["items"]]
    affine = sum(1 for it in persp if it[7:] == (0.0, 0.0, 1.0))
    assert 0.10 * len(persp) <= affine <= 0.15 * len(persp)
    warp = [(c, it) for c, _ in drawn[0]["warp"] for it in c["items"]]
    far = sum(1 for c, it in warp if abs(it[3]) > 2000 or abs(it[6]) > 2000)
    assert 0.2 * len(warp) <= far <= 0.3 * len(warp)
    for fam in ("warp", "persp"):
        borders = [c["border"] for c, _ in drawn[0][fam]]
        assert any(b is None for b in borders) and any(b is not None for b in borders)


@pytest.mark.parametrize("family", F.FAMILIES)
def test_the_lds_budget_reaches_gather_and_mixed_launches(drawn, family, monkeypatch):
    if knob_run(("TSVPP_LDS_KB",)):
        return
    pairs = drawn[0][family]
    monkeypatch.setenv("TSVPP_LDS_KB", "0")
    for c, _ in pairs:
        d = F.describe(c)
        assert d["kernel"].endswith("gather>") or ",gather," in d["kernel"], (c, d)
        assert d["staged"] == 0
    monkeypatch.setenv("TSVPP_LDS_KB", "3")
    mixed = [c for c, _ in pairs if 0 < F.describe(c)["staged"] < len(c["items"])]
    assert mixed
    assert any(c["seed"] == F.seed_of(family, 0) for c in mixed), "chunk 0 (the one the GPU test replays under this budget) has no mixed launch"
