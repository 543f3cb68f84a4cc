"""GPU: tsvpp_convert_rois_sized_tensor -- convert_rois_sized with dtype= / mean= / std=: fp16 / bf16 / fp32 elements, per-channel mean and scale, on the twelve
sizes of rois_sized_util.SIZES in one call.  The expected bytes are tensor_util.expected of the oracle's fp32 result for the box at its own size; every
comparison is np.array_equal on raw bytes, every call writes into a poisoned buffer with guards (rois_sized_util.run)."""
import numpy as np
import pytest
import torch

import rois_sized_util as U
import tensor_util as T
from rois_sized_util import BGR24, BICUBIC, BILINEAR, BOXES, MERGED, NEAREST, PLANAR, RGB24, SIZES, Y800

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def frames():
    host = U.host_frames()
    return host, U.device_frames(host)


@pytest.mark.parametrize("spec", sorted(T.SPECS))
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("rt,fcc,planes", [(BILINEAR, BGR24, PLANAR), (BICUBIC, Y800, MERGED), (NEAREST, BGR24, PLANAR)])
def test_tensor_outputs_match_the_oracle(vpp, oracle, frames, rt, fcc, planes, dtype, spec):
    import tensor_stream as ts
    host, dev = frames
    fp = U.frame_parameters(ts, rt, fcc, planes, True)
    mean, std = T.SPECS[spec]
    want = [T.expected(U.expect(oracle, host, b, s, rt, fcc, planes, True, key="fixed").view(np.float32), U.channels(fcc), T.SPECS[spec], dtype)
            for b, s in zip(BOXES, SIZES)]
    for aligned in (True, [i % 2 == 0 for i in range(12)]):
        outs = U.run(vpp, dev, BOXES, SIZES, fp, fcc, T.ESIZE[dtype], aligned=aligned, dtype=T.TORCH[dtype], what=f"{dtype} {spec}", mean=mean, std=std)
        U.compare(outs, want, BOXES, SIZES, f"rt={rt} fcc={fcc} {dtype} {spec} aligned={aligned is True}")


@pytest.mark.parametrize("fcc,planes", [(BGR24, PLANAR), (Y800, MERGED)])
def test_the_identity_fp32_spec_gives_the_plain_call(vpp, frames, fcc, planes):
    import tensor_stream as ts
    host, dev = frames
    fp = U.frame_parameters(ts, BILINEAR, fcc, planes, True)
    plain = U.run(vpp, dev, BOXES, SIZES, fp, fcc, 4, what="plain")
    ident = U.run(vpp, dev, BOXES, SIZES, fp, fcc, 4, what="identity", dtype=torch.float32, mean=0.0, std=1.0)
    U.compare(ident, plain, BOXES, SIZES, "identity spec")


def test_merged_with_a_spec_is_unsupported(vpp, frames):
    import tensor_stream as ts
    host, dev = frames
    fp = U.frame_parameters(ts, BILINEAR, RGB24, MERGED, True)
    with pytest.raises(RuntimeError, match="-2"):
        U.run(vpp, dev, BOXES, SIZES, fp, RGB24, 2, dtype=torch.float16, what="merged", mean=0.5, std=0.5)
    with pytest.raises(RuntimeError, match="-2"):
        ts.describe_rois_sized(fp, U.FRAMES, BOXES, SIZES, dtype=torch.float16)
    # an fp16 output that is not aligned to its element: TSVPP_ERROR
    fp = U.frame_parameters(ts, BILINEAR, RGB24, PLANAR, True)
    buf = torch.zeros(3 * 32 * 32 * 2 + 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="-3"):
        vpp.convert_rois_sized(dev[0][0], dev[0][1], [(0, 0, 64, 64)], fp, [(32, 32)], out=[buf[1:1 + 3 * 32 * 32 * 2]], width=320, height=180, dtype=torch.float16)
