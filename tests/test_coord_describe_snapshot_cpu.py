"""CPU: what describe_warp, describe_perspective, describe_remap, describe_mesh and their tensor forms answer for 277 requests against the committed snapshot
(tests/golden/coord_describe_snapshot.json, regenerate with tests/golden/make_coord_describe_snapshot.py after an INTENDED change).  The four paths share their
launch fill, staging budgets, launch split, describe line and request skeleton; a change to one of them must show up in review as a diff of that file, not as
another kernel, grid, LDS size or status for some request of another path."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _maker():
    spec = importlib.util.spec_from_file_location("make_coord_describe_snapshot", os.path.join(HERE, "golden", "make_coord_describe_snapshot.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.skipif(any(k.startswith("TSVPP_") and k not in ("TSVPP_DEBUG_KNOBS", "TSVPP_BENCH_STUB") for k in os.environ), reason="knob runs select other kernels on purpose")
def test_coordinate_paths_answer_as_the_committed_snapshot():
    m = _maker()
    with open(os.path.join(HERE, "golden", "coord_describe_snapshot.json")) as f:
        want = json.load(f)
    got = m.snapshot()
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:10]
    diff = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    assert not diff, f"{len(diff)} requests are answered differently, e.g. {list(diff.items())[:3]} -- intended? then regenerate the snapshot"
    assert 200 <= len(want) <= 300
    ok = [v for v in want.values() if "error" not in v]
    # the snapshot spans the paths, not one corner of them: all eight kernel families, both store kinds, staged and gathered launches, 1 to 3 launches, both
    # borders, both statuses -- and the matrix paths count what they stage while the map paths cannot
    families = {f"vpp_{p}{t}" for p in ("warp", "persp", "remap", "mesh") for t in ("", "_tensor")}
    assert {v["kernel"].split("<")[0] for v in ok} == families
    assert {v["mode"] for v in ok} == {"warp_bilinear", "persp_bilinear", "remap_bilinear", "mesh_bilinear"}
    for fam in families:
        mine = [v for v in ok if v["kernel"].split("<")[0] == fam]
        assert any(",vec," in v["kernel"] for v in mine) and any(",elem," in v["kernel"] for v in mine), fam
        assert any(v["kernel"].endswith(",border>") for v in mine) and any(v["kernel"].endswith(",replicate>") for v in mine), fam
        # the host sees a matrix path's footprints: it counts what stages, and a launch none of whose tiles fit takes the gather kernel; a map path's launch
        # takes the staged kernel with the hint or the budget as its LDS, and every workgroup decides for itself
        matrix = fam.startswith(("vpp_warp", "vpp_persp"))
        assert all(("staged" in v) == matrix for v in mine), fam
        assert any(",staged," in v["kernel"] for v in mine) and any(",gather," in v["kernel"] for v in mine) == matrix, fam
    assert {v["launches"] for v in ok} >= {1, 2, 3}
    assert any(v["tail"] == 2 for v in ok) and any(v["nt"] == 0 for v in ok)
    assert {v["border"] for v in ok} == {"replicate", "16,128,128"}
    refused = {k: v["error"] for k, v in want.items() if "error" in v}
    assert set(refused.values()) == {"-2", "-3"}
    # every refusal is named after its status: where a request has two faults, the one that wins comes first in its name
    for k, sts in refused.items():
        first = next(w for w in k.split() if w in ("ERROR", "UNSUPPORTED"))
        assert k.startswith("refused ") and sts == {"ERROR": "-3", "UNSUPPORTED": "-2"}[first], (k, sts)
    assert not [k for k in want if k.startswith("refused ") and k not in refused]
