"""GPU: a small seeded differential fuzz of tsvpp_convert_remap with a generator of its own (24 calls): frames of 2 x 2 .. 320 x 180 whose pitches are no multiple
of 16 and whose planes start anywhere, outputs of 2 x 2 .. 160 x 100, every flavour, replicate or a drawn border, maps of every kind of tests/remap_util.py's set
with drawn parameters, tight or padded rows, hints drawn below and above the need.  Every output is compared on raw bits with the model (never with the library
itself) and every call writes into the slots of one poisoned buffer: the bytes outside the slots must stay as they were."""
import numpy as np
import pytest
import torch

import remap_util as R
from letterbox_util import FLAVOURS, Y800, bits

pytestmark = pytest.mark.gpu

SEED, CALLS, GUARD, POISON = 20261019, 24, 64, 0xA5
KINDS = ("translate", "affine", "barrel", "transpose", "constant", "split", "far", "garbage", "noise")


def draw_call(rng):
    """one call: 1 .. 3 frames, 1 .. 3 maps, 1 .. 6 outputs (or 33 .. 36: two launches) of one drawn size"""
    dst = (2 * int(rng.integers(1, 81)), 2 * int(rng.integers(1, 51)))
    frames = []
    for _ in range(int(rng.integers(1, 4))):
        w, h = 2 * int(rng.integers(1, 161)), 2 * int(rng.integers(1, 91))
        frames.append(dict(w=w, h=h, pitch_y=w + int(rng.integers(0, 40)), pitch_uv=w + int(rng.integers(0, 40)), off_y=int(rng.integers(0, 16)), off_uv=int(rng.integers(0, 16)),
                           seed=int(rng.integers(0, 1 << 30))))
    n_maps = int(rng.integers(1, 4))
    n = int(rng.integers(33, 37)) if rng.random() < 0.15 else int(rng.integers(1, 7))
    remaps = [(int(rng.integers(0, len(frames))), int(rng.integers(0, n_maps))) for _ in range(n)]
    maps = []
    for m in range(n_maps):
        # (a map is made for the frame of the first output that uses it, or frame 0: any map is legal on any frame)
        fr = frames[next((f for f, mm in remaps if mm == m), 0)]
        maps.append(dict(kind=KINDS[int(rng.integers(0, len(KINDS)))], w=fr["w"], h=fr["h"], seed=int(rng.integers(0, 1 << 30)), extra=2 * int(rng.integers(0, 5)),
                         hint=int(rng.choice([0, 0, 512, 3000, 20000, 1 << 20])), p=rng.uniform(-1, 1, 4).tolist()))
    return dict(dst=dst, frames=frames, maps=maps, remaps=remaps, flavour=FLAVOURS[int(rng.integers(0, len(FLAVOURS)))],
                border=None if rng.random() < 0.5 else tuple(int(v) for v in rng.integers(0, 256, 3)), off=int(rng.choice([0, 0, 1, 4, 8])))


def make_map(m, dst):
    dw, dh = dst
    w, h, p = m["w"], m["h"], m["p"]
    kind = m["kind"]
    if kind == "translate":
        return R.translation(dw, dh, round(p[0] * w), round(p[1] * h))
    if kind == "affine":
        return R.affine(dw, dh, w, h, degrees=180 * p[0], scale=0.2 + 2.5 * abs(p[1]) * max(w / dw, 1))
    if kind == "barrel":
        return R.barrel(dw, dh, w, h, k1=0.4 * p[0], k2=0.1 * p[1])
    if kind == "transpose":
        return R.transpose(dw, dh)
    if kind == "constant":
        return R.constant(dw, dh, (0.5 + 0.7 * p[0]) * w, (0.5 + 0.7 * p[1]) * h)
    if kind == "split":
        return R.split(dw, dh, w, h)
    if kind == "far":
        return R.far(dw, dh)
    if kind == "garbage":
        return R.garbage(dw, dh, m["seed"])
    rng = np.random.default_rng(m["seed"])  # noise: every pixel anywhere in or slightly around the frame
    return R.stack(rng.uniform(-4, w + 4, (dh, dw)), rng.uniform(-4, h + 4, (dh, dw)))


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


def test_the_generator_covers_its_ground():
    kinds = {m["kind"] for c in CALLS_DRAWN for m in c["maps"]}
    assert kinds == set(KINDS), set(KINDS) - kinds
    assert any(len(c["remaps"]) > 32 for c in CALLS_DRAWN) and any(c["border"] is None for c in CALLS_DRAWN) and any(c["border"] is not None for c in CALLS_DRAWN)
    assert any(c["dst"][0] % 4 and c["dst"][0] >= 32 for c in CALLS_DRAWN) and any(c["dst"][0] < 32 for c in CALLS_DRAWN)
    assert any(c["off"] for c in CALLS_DRAWN) and any(not c["off"] for c in CALLS_DRAWN)
    assert any(m["extra"] for c in CALLS_DRAWN for m in c["maps"]) and any(m["hint"] for c in CALLS_DRAWN for m in c["maps"])


def run_call(vpp, oracle, call, index):
    """one drawn call (tests/test_gpu_edge_content.py: the same call with its frames' content replaced) against the model, guards included"""
    import tensor_stream as ts
    dst, (fcc, planes_pos, norm), border = call["dst"], call["flavour"], call["border"]
    host = [planes(fr) for fr in call["frames"]]
    dev = []
    for (flat_y, flat_uv, _, _), fr in zip(host, call["frames"]):
        ty, tuv = torch.from_numpy(flat_y).cuda(), torch.from_numpy(flat_uv).cuda()
        dev.append((ty[fr["off_y"]:fr["off_y"] + fr["h"] * fr["pitch_y"]].view(fr["h"], fr["pitch_y"]),
                    tuv[fr["off_uv"]:fr["off_uv"] + (fr["h"] // 2) * fr["pitch_uv"]].view(fr["h"] // 2, fr["pitch_uv"])))
    host_maps = [make_map(m, dst) for m in call["maps"]]
    dev_maps = []
    for m, xy in zip(call["maps"], host_maps):
        _, back = R.padded(xy, extra=m["extra"])
        t = torch.from_numpy(back).cuda()[:, :2 * dst[0]].unflatten(1, (dst[0], 2))
        dev_maps.append((t, m["hint"]) if m["hint"] else t)
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
    vpp.convert_remap([d[0] for d in dev], [d[1] for d in dev], dev_maps, ts.FrameParameters(width=dst[0], height=dst[1], resize_type=1, pixel_format=fcc,
                      planes_pos=planes_pos, normalization=norm), remaps=call["remaps"], border=border, out=out,
                      width=[fr["w"] for fr in call["frames"]], height=[fr["h"] for fr in call["frames"]])
    torch.cuda.synchronize()
    cache = {}
    for i, (f, m) in enumerate(call["remaps"]):
        if (f, m) not in cache:
            fr = call["frames"][f]
            cache[(f, m)] = R.expected(oracle, host[f][2], host[f][3], fr["w"], fr["h"], host_maps[m], fcc, planes_pos, norm, border)
        g = bits(out[i])
        bad = np.flatnonzero(g != cache[(f, m)])
        assert bad.size == 0, f"call {index} output {i}: frame {call['frames'][f]} map {call['maps'][m]} -> {dst} flavour {call['flavour']} border {border}: {bad.size} bytes differ"
    want = buf.clone()
    for s in starts:
        want[s:s + nbytes] = pat[s:s + nbytes]
    assert torch.equal(want, pat), f"call {index}: a byte outside the outputs changed"

@pytest.mark.parametrize("index", range(CALLS))
def test_fuzz_call(vpp, oracle, index):
    run_call(vpp, oracle, CALLS_DRAWN[index], index)
