"""CPU: what describe_rois, describe_rois_area, describe_letterbox and their tensor forms answer for ~300 requests against the committed snapshot
(tests/golden/tile_describe_snapshot.json, regenerate with tests/golden/make_tile_describe_snapshot.py after an INTENDED change).  The three paths share their
launch fill, staging budget, launch split and request rules; a change to one of them must show up in review as a diff of that file, not as another kernel,
grid or LDS size for some request of another path."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _maker():
    spec = importlib.util.spec_from_file_location("make_tile_describe_snapshot", os.path.join(HERE, "golden", "make_tile_describe_snapshot.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.skipif(any(k.startswith("TSVPP_") and k not in ("TSVPP_DEBUG_KNOBS", "TSVPP_BENCH_STUB") for k in os.environ), reason="knob runs select other kernels on purpose")
def test_tile_paths_answer_as_the_committed_snapshot():
    m = _maker()
    want = json.load(open(os.path.join(HERE, "golden", "tile_describe_snapshot.json")))
    got = m.snapshot()
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:10]
    diff = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    assert not diff, f"{len(diff)} requests are answered differently, e.g. {list(diff.items())[:3]} -- intended? then regenerate the snapshot"
    assert len(want) >= 200
    ok = [v for v in want.values() if "error" not in v]
    # the snapshot spans the paths, not one corner of them: all six kernel families, both store kinds, staged and gathered launches, 1 to 3 launches, both statuses
    assert {v["kernel"].split("<")[0] for v in ok} == {"vpp_rois", "vpp_rois_area", "vpp_rois_tensor", "vpp_rois_area_tensor", "vpp_letterbox", "vpp_letterbox_tensor"}
    assert any(",vec," in v["kernel"] for v in ok) and any(",elem," in v["kernel"] for v in ok)
    assert any(v["kernel"].endswith("staged>") for v in ok) and any(v["kernel"].endswith("gather>") for v in ok)
    assert {v["launches"] for v in ok} >= {1, 2, 3}
    assert any(v["tail"] == 2 for v in ok) and any(v["nt"] == 0 for v in ok)
    assert {v["error"] for v in want.values() if "error" in v} == {"-2", "-3"}
