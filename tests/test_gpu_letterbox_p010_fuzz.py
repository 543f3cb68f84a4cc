"""Seeded differential fuzz of tsvpp_convert_letterbox_p010: the cases of tests/letterbox_p010_fuzz.py (launches of 1 .. 5 frames at drawn plane offsets and
pitches, canvases up to 200 wide, default and drawn rectangles, both modes, all ten flavours, aligned and unaligned outputs) on the GPU against the model of
tests/p010_util.py, bit for bit, no case skipped -- and the same cases through the describe call on the CPU, which must accept each; the committed seed must
reach the paths the generator exists for."""
import numpy as np
import pytest

import letterbox_p010_fuzz as Z
import p010_cases as P
import p010_util as M
import tensor_util as T

CASES = Z.cases()


def describe(case):
    import tensor_stream as ts
    fp, kw = P.params(case["canvas"], case["mode"], case["flavour"])
    return ts.describe_letterbox_p010(fp, [(f[0], f[1], *Z.byte_pitches(f)) for f in case["frames"]], rects=case["rects"], aligned_outputs=case["aligned"], **kw)


def test_the_generator_is_stable_and_names_every_flavour():
    assert len(CASES) == Z.CASES <= 48 and Z.cases() == CASES
    assert sorted(Z.FLAVOURS) == sorted(P.FLAVOURS)
    for name, (_, _, norm, tensor) in P.FLAVOURS.items():
        assert Z.element_size(name) == (T.ESIZE[tensor[0]] if tensor else (4 if norm else 1)), name


def test_the_committed_seed_reaches_every_path():
    """every request is accepted (describe raises on any other status); a quarter of the frames have chroma pairs that are not 4-byte aligned; a quarter have a
    pitch that is no multiple of 16 bytes; a tenth stage and a tenth gather; every flavour, both modes, both output alignments, 4 k + 2 and sub-tile canvases"""
    frames = [f for c in CASES for f in c["frames"]]
    staged = 0
    for c in CASES:
        d = describe(c)
        assert d["src"] == "p010" and d["frames"] == len(c["frames"]) and d["launches"] == 1 and 0 <= d["staged"] <= len(c["frames"]), (c, d)
        staged += d["staged"]
    n = len(frames)
    no_uv4 = sum(1 for f in frames if not Z.uv4(f))
    off16 = sum(1 for f in frames if any(p % 16 for p in Z.byte_pitches(f)))
    split = sum(1 for f in frames if f[2][1] != f[2][3])
    print(f"{len(CASES)} cases, {n} frames: uv4 false {no_uv4}, a pitch off 16 bytes {off16}, luma and chroma pitches differ {split}, staged {staged}, gathered {n - staged}")
    assert 4 * no_uv4 >= n and 4 * off16 >= n and 10 * staged >= n and 10 * (n - staged) >= n
    assert {c["flavour"] for c in CASES} == set(Z.FLAVOURS) and {c["mode"] for c in CASES} == {M.NEAREST, M.BILINEAR} and {c["aligned"] for c in CASES} == {True, False}
    assert any(c["canvas"][0] % 4 == 2 and c["canvas"][0] >= 32 for c in CASES) and any(c["canvas"][0] < 32 for c in CASES)
    assert any(c["rects"] is None for c in CASES) and any(c["rects"] is not None for c in CASES)
    assert {len(c["frames"]) for c in CASES} == {1, 2, 3, 4, 5}


def run_case(vpp, case):
    """one case against the model, the bytes around the canvases included"""
    import torch
    canvas, flavour = case["canvas"], case["flavour"]
    fcc, _, norm, tensor = P.FLAVOURS[flavour]
    host = Z.host_frames(case)
    sizes = [f[:2] for f in case["frames"]]
    placed = [P.embed(*fr, *f[:2], f[2]) for fr, f in zip(host, case["frames"])]
    n, esz = len(host), Z.element_size(flavour)
    tdt = T.TORCH[tensor[0]] if tensor else (torch.float32 if norm else torch.uint8)
    nbytes = (1 if fcc == M.Y800 else 3) * canvas[0] * canvas[1] * esz
    stride = (nbytes + 16 + 255) // 256 * 256
    buf = torch.full((n * stride + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    off = 0 if case["aligned"] else esz  # (unaligned: the items start one element into the buffer)
    out = [buf[k * stride + off:k * stride + off + nbytes].view(tdt) for k in range(n)]
    assert all((o.data_ptr() % 16 == 0) == case["aligned"] for o in out)
    got, used = P.convert(vpp, host, sizes, canvas, case["mode"], flavour, case["pad"], case["rects"], planes_dev=([p[0] for p in placed], [p[1] for p in placed]), out=out)
    torch.cuda.synchronize()
    rects = P.rects_of(sizes, canvas, case["rects"])
    assert [tuple(u) for u in used] == rects
    for k in range(n):
        P.same(got[k], P.want(host[k], sizes[k], rects[k], canvas, case["mode"], flavour, case["pad"]),
               f"case {case['index']} frame {k} {case['frames'][k]} rect {rects[k]} canvas {canvas} mode={case['mode']} {flavour} aligned={case['aligned']}")
    keep = torch.ones_like(buf, dtype=torch.bool)  # the element before each canvas and everything after it stay as they were
    for k in range(n):
        keep[k * stride + off:k * stride + off + nbytes] = False
    assert bool((buf[keep] == 0xA5).all()), f"case {case['index']}: bytes outside the canvases were written"


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(Z.CASES))
def test_case_against_the_model(vpp, index):
    assert CASES[index]["index"] == index
    run_case(vpp, CASES[index])
