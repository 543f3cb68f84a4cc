"""Seeded differential fuzz of tsvpp_convert_letterbox_area: the cases of tests/letterbox_area_fuzz.py (canvases up to 134 a side, frames up to 420, default and
drawn rectangles, every flavour, tensor forms, aligned and unaligned outputs) on the GPU against the oracle, bit for bit -- and the same cases through the describe
call on the CPU, which must accept each and count its down-scale frames as the generator does."""
import numpy as np
import pytest

import letterbox_area_fuzz as Z
import tensor_util as T
from letterbox_util import AREA, PLANAR, Y800, bits, expected_canvas

CASES = Z.cases()


def params(ts, case):
    fcc, planes, norm = case["flavour"]
    return ts.FrameParameters(width=case["canvas"][0], height=case["canvas"][1], resize_type=AREA, pixel_format=fcc, planes_pos=planes, normalization=norm)


def spec_kw(case):
    import torch  # noqa: F401
    if case["tensor"] is None:
        return {}
    dtype, name = case["tensor"]
    return dict(dtype=T.TORCH[dtype], mean=T.SPECS[name][0], std=T.SPECS[name][1])


def test_the_generator_is_stable_and_small():
    assert len(CASES) == Z.CASES <= 40 and Z.cases() == CASES
    assert all(max(c["canvas"]) <= 134 and max(max(f[:2]) for f in c["frames"]) <= 420 for c in CASES)
    assert any(c["rects"] is None for c in CASES) and any(c["rects"] is not None for c in CASES) and any(c["tensor"] for c in CASES)
    assert any(c["canvas"][0] % 4 and c["canvas"][0] >= 32 for c in CASES) and any(c["canvas"][0] < 32 for c in CASES)
    assert any(0 < Z.down_frames(c) < len(c["frames"]) for c in CASES)  # a launch that mixes both rules


@pytest.mark.parametrize("index", range(Z.CASES))
def test_describe_accepts_every_case(index):
    import tensor_stream as ts
    case = CASES[index]
    d = ts.describe_letterbox_area(params(ts, case), case["frames"], rects=case["rects"], aligned_outputs=case["aligned"], **spec_kw(case))
    r0 = Z.rects_of(case)[0]
    assert d["mode"] == "area" and d["frames"] == len(case["frames"]) and d["launches"] == 1 and d["down"] == Z.down_frames(case)
    assert d["inner"] == "%dx%d+%d+%d" % (r0[2], r0[3], r0[0], r0[1]) and d["chain"] >= 0
    assert d["kernel"].startswith("vpp_letterbox_area_tensor<" if case["tensor"] else "vpp_letterbox_area<")


def run_case(vpp, oracle, case):
    """one case (tests/test_gpu_edge_content.py: the same case with its frames' content replaced) against the oracle, the bytes between the canvases included"""
    import torch
    import tensor_stream as ts
    index = case["index"]
    canvas, (fcc, planes, norm) = case["canvas"], case["flavour"]
    host = Z.host_frames(case)
    dev = [(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()) for y, uv in host]
    n, c = len(host), (1 if fcc == Y800 else 3)
    esz = T.ESIZE[case["tensor"][0]] if case["tensor"] else (4 if norm else 1)
    tdt = T.TORCH[case["tensor"][0]] if case["tensor"] else (torch.float32 if norm else torch.uint8)
    nbytes = c * canvas[0] * canvas[1] * esz
    stride = (nbytes + 16 + 255) // 256 * 256
    buf = torch.full((n * stride + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    off = 0 if case["aligned"] else esz
    out = [buf[k * stride + off:k * stride + off + nbytes].view(tdt) for k in range(n)]  # (flat: the call reads addresses only)
    assert all((o.data_ptr() % 16 == 0) == case["aligned"] for o in out)
    got, used = vpp.convert_letterbox_area([d[0] for d in dev], [d[1] for d in dev], params(ts, case), pad=case["pad"], rects=case["rects"], out=out,
                                           width=[f[0] for f in case["frames"]], height=[f[1] for f in case["frames"]], **spec_kw(case))
    torch.cuda.synchronize()
    rects = Z.rects_of(case)
    assert [tuple(u) for u in used] == [tuple(r) for r in rects]
    for k, ((w, h, _), (y, uv)) in enumerate(zip(case["frames"], host)):
        if case["tensor"]:
            q = expected_canvas(oracle, y, uv, w, h, rects[k], canvas, AREA, fcc, PLANAR, True, case["pad"]).view(np.float32)
            ref = T.expected(q, c, T.SPECS[case["tensor"][1]], case["tensor"][0])
            g = T.bits(got[k])
        else:
            ref = expected_canvas(oracle, y, uv, w, h, rects[k], canvas, AREA, fcc, planes, norm, case["pad"])
            g = bits(got[k])
        bad = np.flatnonzero(g != ref) if g.size == ref.size else np.array([-1])
        assert bad.size == 0, f"case {index} content {case.get('content')} frame {k} {case['frames'][k]} rect {rects[k]} canvas {canvas} {case['flavour']} {case['tensor']}: {bad.size} bytes differ, first at {bad[:4]}"
    # the bytes between the canvases stay as they were
    keep = torch.ones_like(buf, dtype=torch.bool)
    for k in range(n):
        keep[k * stride + off:k * stride + off + nbytes] = False
    assert bool((buf[keep] == 0xA5).all()), f"case {index}: bytes outside the canvases were written"


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(Z.CASES))
def test_case_against_the_oracle(vpp, oracle, index):
    assert CASES[index]["index"] == index
    run_case(vpp, oracle, CASES[index])
