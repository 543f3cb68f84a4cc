"""GPU: a small seeded differential fuzz of tsvpp_convert_mesh in the manner of tests/test_gpu_remap_fuzz.py (40 calls): frames of 2 x 2 .. 320 x 180 whose
pitches are no multiple of 16 and whose planes start anywhere, outputs of 2 x 2 .. 160 x 100, every flavour, replicate or a drawn border, a drawn cell per mesh,
meshes of every kind with drawn parameters, tight or padded rows, hints drawn below and above the need.  Every output is compared on raw bits with the model of
E(mesh) (tests/mesh_util.py, tests/remap_util.py; never with the library itself) and every call writes into the slots of one poisoned buffer: the bytes outside
the slots must stay as they were.  A CPU test checks that the generator covers its ground."""
import numpy as np
import pytest

import mesh_util as M
import remap_util as R
from letterbox_util import FLAVOURS, Y800, bits

SEED, CALLS, GUARD, POISON = 20261020, 40, 64, 0xA5
KINDS = ("identity", "translate", "affine", "barrel", "far", "garbage", "noise")
SIDES = (4, 8, 16, 32, 64, 128, 256)
BUDGET = 40 * 1024 - 64  # the default launch's dynamic LDS


def draw_call(rng):
    """one call: 1 .. 3 frames, 1 .. 3 meshes, 1 .. 6 outputs (or 33 .. 36: two launches) of one drawn size"""
    dst = (2 * int(rng.integers(1, 81)), 2 * int(rng.integers(1, 51)))
    frames = []
    for _ in range(int(rng.integers(1, 4))):
        w, h = 2 * int(rng.integers(1, 161)), 2 * int(rng.integers(1, 91))
        frames.append(dict(w=w, h=h, pitch_y=w + int(rng.integers(0, 40)), pitch_uv=w + int(rng.integers(0, 40)), off_y=int(rng.integers(0, 16)), off_uv=int(rng.integers(0, 16)),
                           seed=int(rng.integers(0, 1 << 30))))
    n_meshes = int(rng.integers(1, 4))
    n = int(rng.integers(33, 37)) if rng.random() < 0.15 else int(rng.integers(1, 7))
    remaps = [(int(rng.integers(0, len(frames))), int(rng.integers(0, n_meshes))) for _ in range(n)]
    meshes = []
    for m in range(n_meshes):
        fr = frames[next((f for f, mm in remaps if mm == m), 0)]  # (made for the frame of the first output that uses it: any mesh is legal on any frame)
        meshes.append(dict(kind=KINDS[int(rng.integers(0, len(KINDS)))], w=fr["w"], h=fr["h"], seed=int(rng.integers(0, 1 << 30)), extra=2 * int(rng.integers(0, 5)),
                           cell=(SIDES[int(rng.integers(0, len(SIDES)))], SIDES[int(rng.integers(0, len(SIDES)))]),
                           hint=int(rng.choice([0, 0, 512, 3000, 20000, 1 << 20])), p=rng.uniform(-1, 1, 4).tolist()))
    return dict(dst=dst, frames=frames, meshes=meshes, remaps=remaps, flavour=FLAVOURS[int(rng.integers(0, len(FLAVOURS)))],
                border=None if rng.random() < 0.5 else tuple(int(v) for v in rng.integers(0, 256, 3)), off=int(rng.choice([0, 0, 1, 4, 8])))


def make_mesh(m, dst):
    dw, dh = dst
    w, h, p, cell, kind = m["w"], m["h"], m["p"], m["cell"], m["kind"]
    if kind == "identity":
        return M.identity(dw, dh, cell)
    if kind == "translate":
        return M.translation(dw, dh, cell, round(p[0] * w), round(p[1] * h))
    if kind == "affine":
        return M.affine(dw, dh, cell, w, h, degrees=180 * p[0], scale=0.2 + 2.5 * abs(p[1]) * max(w / dw, 1))
    if kind == "barrel":
        return M.barrel(dw, dh, cell, w, h, k1=0.4 * p[0], k2=0.1 * p[1])
    if kind == "far":
        return M.far(dw, dh, cell)
    if kind == "garbage":
        return M.garbage(dw, dh, cell, m["seed"])
    rng = np.random.default_rng(m["seed"])  # noise: every control point anywhere in or slightly around the frame
    rows, cols = M.dims(dw, dh, cell)
    return M.stack(rng.uniform(-4, w + 4, (rows, cols)), rng.uniform(-4, h + 4, (rows, cols)))


def planes(fr):
    if fr.get("content"):  # a class of tests/edge_content.py in place of the seeded random bytes
        import edge_content
        return edge_content.planes(fr["content"], fr)
    rng = np.random.default_rng(fr["seed"])
    flat_y = rng.integers(0, 256, fr["off_y"] + fr["h"] * fr["pitch_y"] + 16, dtype=np.uint8)
    flat_uv = rng.integers(0, 256, fr["off_uv"] + (fr["h"] // 2) * fr["pitch_uv"] + 16, dtype=np.uint8)
    y = flat_y[fr["off_y"]:fr["off_y"] + fr["h"] * fr["pitch_y"]].reshape(fr["h"], fr["pitch_y"])
    uv = flat_uv[fr["off_uv"]:fr["off_uv"] + (fr["h"] // 2) * fr["pitch_uv"]].reshape(fr["h"] // 2, fr["pitch_uv"])
    return flat_y, flat_uv, y, uv


CALLS_DRAWN = [draw_call(np.random.default_rng([SEED, k])) for k in range(CALLS)]


def tile_paths(call):
    """(a tile stages, a tile gathers) over the call's launches of 32 outputs: the launch's LDS is the budget or the largest hint of the meshes it uses (a mesh
    without one counts as the budget), and a tile stages iff its footprint -- the dense call's on E(mesh) -- is stageable and needs no more"""
    staged = gathered = False
    dst = call["dst"]
    dense = [M.expand(make_mesh(m, dst), *dst, m["cell"]) for m in call["meshes"]]
    vec = call["off"] == 0 and not (dst[0] % 4 and dst[0] < 32)
    for base in range(0, len(call["remaps"]), 32):
        group = call["remaps"][base:base + 32]
        lds = min(max(call["meshes"][m]["hint"] or BUDGET for _, m in group), BUDGET)
        for f, m in group:
            fr = call["frames"][f]
            for (j0, j1, i0, i1) in R.tiles(*dst, vec):
                j1, i1 = j1 | 1, i1 | 1
                x, y, cx, cy = (c[(i0 >> s):(i1 >> s) + 1, (j0 >> s):(j1 >> s) + 1] for c, s in zip(R.coords(dense[m], fr["w"], fr["h"]), (0, 0, 1, 1)))
                box = []
                for c, limit in ((x, fr["w"]), (y, fr["h"]), (cx, fr["w"] // 2), (cy, fr["h"] // 2)):
                    lo, hi = int(np.floor(c.min())), int(np.floor(c.max())) + 1
                    box += [min(max(lo, 0), limit - 1), min(max(hi, 0), limit - 1)]
                fits = R.stageable(box) and R.lds_need(box, call["flavour"][0] == Y800) <= lds
                staged, gathered = staged or fits, gathered or not fits
    return staged, gathered


def test_the_generator_covers_its_ground():
    """4 k + 2 widths of at least a tile with aligned outputs (the shifted tile column, where a thread tile can straddle two cells), every cell side on each axis,
    every kind, both launch counts, both borders, aligned and unaligned outputs, padded rows, hints, and calls with staged tiles and calls with gathered ones"""
    kinds = {m["kind"] for c in CALLS_DRAWN for m in c["meshes"]}
    assert kinds == set(KINDS), set(KINDS) - kinds
    assert {m["cell"][0] for c in CALLS_DRAWN for m in c["meshes"]} == set(SIDES) and {m["cell"][1] for c in CALLS_DRAWN for m in c["meshes"]} == set(SIDES)
    shifted = [c for c in CALLS_DRAWN if c["dst"][0] % 4 and c["dst"][0] >= 32 and c["off"] == 0]
    assert shifted and any(m["cell"][0] <= 16 for c in shifted for m in c["meshes"])
    assert any(len(c["remaps"]) > 32 for c in CALLS_DRAWN) and any(c["border"] is None for c in CALLS_DRAWN) and any(c["border"] is not None for c in CALLS_DRAWN)
    assert any(c["dst"][0] < 32 for c in CALLS_DRAWN) and any(c["off"] for c in CALLS_DRAWN)
    assert any(m["extra"] for c in CALLS_DRAWN for m in c["meshes"]) and any(m["hint"] for c in CALLS_DRAWN for m in c["meshes"])
    paths = [tile_paths(c) for c in CALLS_DRAWN]
    assert any(s for s, _ in paths) and any(g for _, g in paths) and any(s and g for s, g in paths)


def run_call(vpp, oracle, call, index):
    """one drawn call (tests/test_gpu_edge_content.py: the same call with its frames' content replaced) against the model, guards included"""
    import torch
    import tensor_stream as ts
    dst, (fcc, planes_pos, norm), border = call["dst"], call["flavour"], call["border"]
    host = [planes(fr) for fr in call["frames"]]
    dev = []
    for (flat_y, flat_uv, _, _), fr in zip(host, call["frames"]):
        ty, tuv = torch.from_numpy(flat_y).cuda(), torch.from_numpy(flat_uv).cuda()
        dev.append((ty[fr["off_y"]:fr["off_y"] + fr["h"] * fr["pitch_y"]].view(fr["h"], fr["pitch_y"]),
                    tuv[fr["off_uv"]:fr["off_uv"] + (fr["h"] // 2) * fr["pitch_uv"]].view(fr["h"] // 2, fr["pitch_uv"])))
    host_meshes = [make_mesh(m, dst) for m in call["meshes"]]
    dense = [M.expand(mesh, *dst, m["cell"]) for m, mesh in zip(call["meshes"], host_meshes)]
    dev_meshes = []
    for m, mesh in zip(call["meshes"], host_meshes):
        _, back = M.padded(mesh, extra=m["extra"])
        t = torch.from_numpy(back).cuda()[:, :2 * mesh.shape[1]].unflatten(1, (mesh.shape[1], 2))
        dev_meshes.append((t, m["hint"]) if m["hint"] else t)
    n = len(call["remaps"])
    esize = 4 if norm else 1
    nbytes = (1 if fcc == Y800 else 3) * dst[0] * dst[1] * esize
    off = call["off"] if not norm else call["off"] // 4 * 4  # (an fp32 output is aligned to its element)
    stride = (GUARD + off + nbytes + GUARD + 15) // 16 * 16
    total = n * stride
    pat = torch.from_numpy(((np.arange(total, dtype=np.int64) * 131 + 17) % 251).astype(np.uint8)).cuda()
    buf = pat.clone()
    starts = [k * stride + GUARD + off for k in range(n)]
    out = []
    for s in starts:
        buf[s:s + nbytes] = POISON
        out.append(buf[s:s + nbytes].view(torch.float32) if norm else buf[s:s + nbytes])
    vpp.convert_mesh([d[0] for d in dev], [d[1] for d in dev], dev_meshes, ts.FrameParameters(width=dst[0], height=dst[1], resize_type=1, pixel_format=fcc,
                     planes_pos=planes_pos, normalization=norm), cell=[m["cell"] for m in call["meshes"]], remaps=call["remaps"], border=border, out=out,
                     width=[fr["w"] for fr in call["frames"]], height=[fr["h"] for fr in call["frames"]])
    torch.cuda.synchronize()
    cache = {}
    for i, (f, m) in enumerate(call["remaps"]):
        if (f, m) not in cache:
            fr = call["frames"][f]
            cache[(f, m)] = R.expected(oracle, host[f][2], host[f][3], fr["w"], fr["h"], dense[m], fcc, planes_pos, norm, border)
        g = bits(out[i])
        bad = np.flatnonzero(g != cache[(f, m)])
        assert bad.size == 0, f"call {index} output {i}: frame {call['frames'][f]} mesh {call['meshes'][m]} -> {dst} flavour {call['flavour']} border {border}: {bad.size} bytes differ"
    want = buf.clone()
    for s in starts:
        want[s:s + nbytes] = pat[s:s + nbytes]
    assert torch.equal(want, pat), f"call {index}: a byte outside the outputs changed"

@pytest.mark.gpu
@pytest.mark.parametrize("index", range(CALLS))
def test_fuzz_call(vpp, oracle, index):
    run_call(vpp, oracle, CALLS_DRAWN[index], index)
