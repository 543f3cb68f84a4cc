"""GPU: seeded differential fuzz of the tile-pipeline calls -- convert_rois, convert_rois_area, convert_letterbox, convert_warp, convert_perspective and their
tensor forms (dtype= / mean= / std=) -- on the requests of tests/tile_fuzz.py: frames of 2 x 2 .. 320 x 180 whose pitches are no multiple of 16 and whose planes
start anywhere, outputs of 2 x 2 .. 160 x 100, every flavour, aligned, unaligned and mixed output placement, calls of two launch groups.

Every output is compared on raw bits (np.array_equal on uint8 views) with the reference models the tree already has, never with the library itself:
    rois, rois_area   oracle.convert on the box's sliced planes (tests/test_gpu_rois_area.py: expect)
    letterbox         letterbox_util.expected_canvas
    warp, persp       warp_util.expected / persp_util.expected
    tensor forms      the fp32 result of the above through tensor_util.expected
Every call writes into the slots of one poisoned buffer (tile_fuzz.slot_starts: 64 guard bytes before and after each output); every byte outside the slots must
stay as it was.  The generator has redrawn whatever the library or a model refuses, so no call is skipped here."""
import numpy as np
import pytest
import torch

import persp_util as P
import tensor_util as T
import tile_fuzz as F
import warp_util as W
from letterbox_util import PLANAR, Y800, default_rect, expected_canvas
from tile_fuzz import device_frames, host_frames
from util import knob_run

pytestmark = pytest.mark.gpu

_TILE = ((np.arange(4096, dtype=np.int64) * 131 + 17) % 251).astype(np.uint8)  # the guard pattern of the test_unaligned_outputs_and_guard_bytes tests
POISON = 0xA5


def pattern(total):
    return np.tile(_TILE, (total + 4095) // 4096)[:total]


def _tensor_form(call, ref):
    """ref: the model's bytes in the call's own flavour -> the expected bytes of the call (the tensor forms: through mean / scale and the element conversion)"""
    if call["tensor"] is None:
        return ref
    dtype, spec = call["tensor"]
    assert call["flavour"][2] and (call["flavour"][0] == Y800 or call["flavour"][1] == PLANAR)
    return T.expected(ref.view(np.float32), 1 if call["flavour"][0] == Y800 else 3, T.SPECS[spec], dtype)


_expected = {}


def expected(oracle, call, host):
    """the expected bytes of every output of the call, computed once per module"""
    key = (call["family"], call["seed"], call["index"], call.get("content"))  # (content: tests/edge_content.py's class, where a test has replaced the frames)
    if key in _expected:
        return _expected[key]
    fcc, planes, norm = call["flavour"]
    dst, rt, family = call["dst"], call["rt"], call["family"]
    out = []
    for item in call["items"]:
        fr = call["frames"][item[0]]
        w, h = fr["w"], fr["h"]
        _, _, y, uv = host[item[0]]
        if family in ("rois", "rois_area"):
            l, t, r, b = item[1:]
            ys, uvs = y[t:b, l:r], uv[t // 2:t // 2 + (b - t) // 2, l:r]  # byte columns: an odd `left` swaps U and V, as the crop stage does
            ref = oracle.convert(ys, uvs, dst=dst, resize_type=rt, fourcc=fcc, planes=planes, normalization=norm)[0].view(np.uint8).ravel()
        elif family == "letterbox":
            rect = item[1] if item[1] is not None else default_rect(w, h, *dst)
            ref = expected_canvas(oracle, y, uv, w, h, rect, dst, rt, fcc, planes, norm, call["pad"])
        elif family == "warp":
            ref = W.expected(oracle, y, uv, w, h, item[1:], dst, fcc, planes, norm, call["border"])
        else:
            ref = P.expected(oracle, y, uv, w, h, item[1:], dst, fcc, planes, norm, call["border"])
        out.append(_tensor_form(call, np.ascontiguousarray(ref)))
    _expected[key] = out
    return out


def convert(v, call, dev, out):
    import tensor_stream as ts
    fp = F.frame_parameters(ts, call)
    family, items = call["family"], call["items"]
    kw = dict(out=out, **F.tensor_kwargs(call))
    if family == "letterbox":
        used = [call["frames"][f] for f, _ in items]
        v.convert_letterbox([dev[f][0] for f, _ in items], [dev[f][1] for f, _ in items], fp, pad=call["pad"], rects=F.letterbox_rects(call),
                            width=[fr["w"] for fr in used], height=[fr["h"] for fr in used], **kw)
        return
    kw.update(width=[fr["w"] for fr in call["frames"]], height=[fr["h"] for fr in call["frames"]])
    ys, uvs = [d[0] for d in dev], [d[1] for d in dev]
    if family == "rois":
        v.convert_rois(ys, uvs, items, fp, **kw)
    elif family == "rois_area":
        v.convert_rois_area(ys, uvs, items, fp, **kw)
    elif family == "warp":
        v.convert_warp(ys, uvs, items, fp, border=call["border"], **kw)
    else:
        v.convert_perspective(ys, uvs, items, fp, border=call["border"], **kw)


def where(call, what=""):
    """the failure message's head: seed, family, call index, the full drawn request and -- outside a knob replay -- the kernel of its first launch group"""
    text = f"seed {call['seed']} family {call['family']} call {call['index']}{what}: request {call}"
    if not knob_run(("TSVPP_LDS_KB",)):
        text += f"; kernel {F.describe(call)['kernel']}"
    return text


def run(v, call, dev):
    """one call into the slots of a poisoned buffer -> the bytes of every output; every byte outside the slots must be unchanged"""
    starts, total = F.slot_starts(call)
    nbytes = F.output_bytes(call)
    pat = pattern(total)
    host = pat.copy()
    for s in starts:
        host[s:s + nbytes] = POISON
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 16 == 0
    dtype = {1: torch.uint8, 4: torch.float32}[F.element_bytes(call)] if call["tensor"] is None else T.TORCH[call["tensor"][0]]
    convert(v, call, dev, [buf[s:s + nbytes].view(dtype) for s in starts])
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    outs = [got[s:s + nbytes].copy() for s in starts]
    for s in starts:
        got[s:s + nbytes] = pat[s:s + nbytes]
    bad = np.flatnonzero(got != pat)
    if bad.size:
        k = int(np.searchsorted(np.array(starts), bad[0], side="right")) - 1
        raise AssertionError(f"{where(call)}: {bad.size} guard bytes damaged, the first at {int(bad[0]) - starts[max(k, 0)]} relative to output {max(k, 0)} of {nbytes} bytes")
    return outs


def compare(call, outs, refs, what=""):
    for i, (g, ref) in enumerate(zip(outs, refs)):
        assert g.size == ref.size, f"{where(call, what)}: output {i} has {g.size} bytes, the model {ref.size}"
        bad = np.flatnonzero(g != ref)
        assert bad.size == 0, f"{where(call, what)}: output {i} (item {call['items'][i]}): {bad.size} of {g.size} bytes differ, first at {bad[:4]}"


@pytest.mark.parametrize("chunk", range(F.CHUNKS))
@pytest.mark.parametrize("family", F.FAMILIES)
def test_calls_match_the_models(vpp, oracle, family, chunk):
    for call in F.cases(family, chunk):
        host = host_frames(call)
        compare(call, run(vpp, call, device_frames(host, call)), expected(oracle, call, host))


@pytest.mark.parametrize("kb", ["0", "3"])
def test_lds_budgets_give_the_same_bits(vpp, oracle, monkeypatch, kb):
    """TSVPP_LDS_KB (read when a context is created) = 0: every tile gathers from global memory; = 3: launches mix staged and gathering tiles.  Chunk 0 of every
    family under the default budget and under this one: the same bits, and the models'"""
    import tensor_stream as ts
    monkeypatch.setenv("TSVPP_LDS_KB", kb)
    v = ts.VideoProcessor(device=0, max_consumers=1)
    try:
        for family in F.FAMILIES:
            for call in F.cases(family, 0):
                host = host_frames(call)
                dev = device_frames(host, call)
                refs = expected(oracle, call, host)
                a, b = run(vpp, call, dev), run(v, call, dev)
                compare(call, a, refs, " (default budget)")
                compare(call, b, refs, f" (TSVPP_LDS_KB={kb})")
    finally:
        v.Close()
