"""GPU: seeded differential fuzz of convert_rois_sized and its tensor form on the requests of tests/rois_sized_fuzz.py: frames of 2 x 2 .. 320 x 180 with odd
pitches and planes that start anywhere, 1 .. 60 boxes per call, output sizes 2 x 2 .. 160 x 100 drawn per box, every flavour, aligned, unaligned and mixed
placement.  Every output is compared on raw bits with oracle.convert on the box's sliced planes (the tensor forms: through tensor_util.expected), never with
the library; every call writes into a poisoned buffer with guards (rois_sized_util.run).  Nothing is redrawn or skipped: the number of calls run is asserted."""
import numpy as np
import pytest

import rois_sized_fuzz as Z
import rois_sized_util as U
import tensor_util as T
import tile_fuzz as F
from tile_fuzz import device_frames, host_frames

pytestmark = pytest.mark.gpu

_ran = []


def run_call(vpp, oracle, call):
    """one drawn call (tests/test_gpu_edge_content.py: the same call with its frames' content replaced) against the oracle, guards included"""
    import tensor_stream as ts
    host = host_frames(call)
    dev = device_frames(host, call)
    planes_host = [(h[2], h[3]) for h in host]
    fcc, planes, norm = call["flavour"]
    what = f"seed {call['seed']} call {call['index']}: request {call}"
    refs = []
    for b, s in zip(call["items"], call["sizes"]):
        ref = U.expect(oracle, planes_host, b, s, call["rt"], fcc, planes, norm)
        if call["tensor"] is not None:
            ref = T.expected(ref.view(np.float32), U.channels(fcc), T.SPECS[call["tensor"][1]], call["tensor"][0])
        refs.append(ref)
    kw = F.tensor_kwargs(call)
    dtype = kw.get("dtype")
    outs = U.run(vpp, dev, call["items"], call["sizes"], U.frame_parameters(ts, call["rt"], fcc, planes, norm), fcc, Z.element_bytes(call), aligned=call["aligned"],
                 frames=[(fr["w"], fr["h"]) for fr in call["frames"]], dtype=dtype, what=what, **({k: v for k, v in kw.items() if k != "dtype"}))
    U.compare(outs, refs, call["items"], call["sizes"], what)


@pytest.mark.parametrize("chunk", range(Z.CHUNKS))
def test_calls_match_the_oracle(vpp, oracle, chunk):
    calls = Z.cases(chunk)
    for call in calls:
        run_call(vpp, oracle, call)
        _ran.append((chunk, call["index"]))
    assert len(calls) == Z.CALLS and sum(1 for c, _ in _ran if c == chunk) == Z.CALLS  # every drawn call ran


def test_the_generator_reaches_the_split_and_both_forms():
    """(host only, but it belongs with the calls above) the 24 calls hold more than 48 boxes in one call, all three placements, tensor and plain forms, all three
    resize types, narrow tails and shifted last columns"""
    calls = [c for k in range(Z.CHUNKS) for c in Z.cases(k)]
    assert len(calls) == Z.CHUNKS * Z.CALLS == 24
    assert max(len(c["items"]) for c in calls) > U.LIMIT and min(len(c["items"]) for c in calls) <= 8
    assert {c["placement"] for c in calls} == {"aligned", "unaligned", "mixed"}
    assert any(c["tensor"] for c in calls) and any(c["tensor"] is None for c in calls) and {c["rt"] for c in calls} == {0, 1, 2}
    sizes = [s for c in calls for s in c["sizes"]]
    assert any(U.narrow_tail(w) for w, _ in sizes) and any(w % 4 and w >= 32 for w, _ in sizes) and max(w for w, _ in sizes) > 150 and max(h for _, h in sizes) > 90
