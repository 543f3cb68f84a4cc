"""GPU: tsvpp_convert_letterbox_p010 at the plane layouts a decoder's allocator can hand it, against a second witness on the device, and under the context options
its header promises.  Every comparison is on raw bits.

layouts   each frame embedded in one larger int16 buffer of 0xFFFF words (tests/p010_cases.py: LAYOUTS), its planes strided views at word offsets 0, 1, 2, 3 and 5
          and pitches of w, w + 1, w + 2, w + 3 and w + 8 words, luma and chroma apart: chroma pairs that are not 4-byte aligned (the two-halfword reader, from
          global memory and from LDS), pitches that are no multiple of 16 bytes (a per-row LDS phase), staged and gathered frames in one launch.  Expected: the model
          on the tight frame, and the same call's output for a tight, freshly allocated copy.
witness   frames of words (b << 8) | r through the 8-bit call and the P010 call with the same rectangles: the samples are 4 b, every float32 step of the blend scales
          exactly, so k >> 2 of the P010 call's luma is the 8-bit call's byte; under the coefficient block (0, 1, 1, 0, 0, 0, 0, 0) R is the V sample and B the U
          sample in both calls, which holds chroma to the same statement.
options   TSVPP_OPT_COLOR_G_TERM 1, 2 and 0 again, and a non-default coefficient block, in a private context, on content whose bits depend on them."""
import numpy as np
import pytest
import torch

import p010_cases as P
import p010_util as M
import tensor_util as T
from p010_cases import BT709

pytestmark = pytest.mark.gpu

CLAMPS = (30, 1000, 12)  # a pad that reaches both clamps of the colour expression
# (frame sizes, canvas, rectangles or None for the default ones, pad).  The last: tests/test_gpu_letterbox_p010.py's launch whose 416 x 416 frame exceeds the
# launch's LDS and gathers while its neighbours stage
LAUNCHES = [([(72, 56)], (64, 64), None, CLAMPS), ([(40, 24)], (64, 64), None, P.GRAY), ([(322, 182)], (70, 66), None, P.BLACK), ([(2, 2), (4, 2)], (66, 34), None, P.GRAY),
            ([(48, 48), (416, 416), (64, 96)], (32, 32), [(0, 0, 32, 32)] * 3, P.BLACK)]
# frames of each launch whose every tile stages, at every layout and in both modes.  322 x 182 -> 70 x 66 stages or gathers by flavour and mode (merged outputs
# keep LDS for their stores, BILINEAR footprints are larger): whatever the tight frame does -- the budget is worst-case over alignments, so the layout cannot move it
STAGED = [1, 1, None, 2, 2]

_frames, _virtual, _tight = {}, {}, {}


def frames_of(i):
    if i not in _frames:
        _frames[i] = [P.frame(w, h, 500 + 10 * i + k) for k, (w, h) in enumerate(LAUNCHES[i][0])]
    return _frames[i]


def expected(i, k, mode, flavour, g_term=0, block=M.COEFFS):
    """the model on the tight frame; the resize stage is computed once per (launch, frame, mode)"""
    sizes, canvas, rects, pad = LAUNCHES[i]
    if (i, k, mode) not in _virtual:
        _virtual[(i, k, mode)] = M.virtual_frame(*frames_of(i)[k], *sizes[k], P.rects_of(sizes, canvas, rects)[k], canvas, mode, pad)
    return P.stored(M.channels(*_virtual[(i, k, mode)], P.FLAVOURS[flavour][0], g_term, block), flavour)


def layout_of(first, k):
    return P.LAYOUTS[(first + k) % len(P.LAYOUTS)]


@pytest.mark.parametrize("flavour", P.FOUR)
@pytest.mark.parametrize("mode", [M.NEAREST, M.BILINEAR])
@pytest.mark.parametrize("first", range(len(P.LAYOUTS)))
def test_plane_layouts(vpp, first, mode, flavour):
    """every launch of LAUNCHES with frame k at layout (first + k) mod 6"""
    import tensor_stream as ts
    for i, (sizes, canvas, rects, pad) in enumerate(LAUNCHES):
        frames, layouts = frames_of(i), [layout_of(first, k) for k in range(len(sizes))]
        fp, kw = P.params(canvas, mode, flavour)
        d = ts.describe_letterbox_p010(fp, [(w, h, *P.byte_pitches(l, w)) for (w, h), l in zip(sizes, layouts)], rects=rects, **kw)
        staged = ts.describe_letterbox_p010(fp, sizes, rects=rects, **kw)["staged"] if STAGED[i] is None else STAGED[i]
        assert d["staged"] == staged and d["src"] == "p010" and ("staged" in d["kernel"]) == (staged > 0), (i, d)
        placed = [P.embed(*fr, *s, l) for fr, s, l in zip(frames, sizes, layouts)]
        got, used = P.convert(vpp, frames, sizes, canvas, mode, flavour, pad, rects, planes_dev=([p[0] for p in placed], [p[1] for p in placed]))
        torch.cuda.synchronize()
        assert [tuple(u) for u in used] == P.rects_of(sizes, canvas, rects)
        if (i, mode, flavour) not in _tight:
            tight, _ = P.convert(vpp, frames, sizes, canvas, mode, flavour, pad, rects)
            torch.cuda.synchronize()
            _tight[(i, mode, flavour)] = [T.bits(t) for t in tight]
        for k, (size, l) in enumerate(zip(sizes, layouts)):
            what = f"launch {i} frame {k} {size} -> {canvas} layout {l} (uv4 {P.uv4(l, size[0])}, pitches {P.byte_pitches(l, size[0])} bytes) mode={mode} {flavour}"
            P.same(got[k], expected(i, k, mode, flavour), what)
            assert np.array_equal(T.bits(got[k]), _tight[(i, mode, flavour)][k]), what + ": differs from the tight copy's output"


# ---- the 8-bit call as a second witness ----------------------------------------------------------------------------------------------------------------------------
PADS = [((114, 128, 128), (456, 512, 512)), ((30, 200, 77), (120, 800, 308))]  # 8-bit and 10-bit pads, a factor of four apart
SWAP = (0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0)  # y_scale, v_to_r, u_to_b, v_to_g, u_to_g, round_bias, y_offset, c_offset: R is the V sample, B the U sample


def both_calls(v, i, mode, fcc, pads):
    """(8-bit canvases as uint8 arrays, P010 canvases as fp32 arrays, the P010 frames, sizes, canvas, rectangles) of launch i on frames of words (b << 8) | r"""
    import tensor_stream as ts
    sizes, canvas, rects, _ = LAUNCHES[i]
    host = [P.frame_of_bytes(w, h, 700 + 10 * i + k) for k, (w, h) in enumerate(sizes)]
    kw = dict(rects=rects, width=[s[0] for s in sizes], height=[s[1] for s in sizes])
    pos = M.MERGED if fcc == M.Y800 else M.PLANAR
    fp8 = ts.FrameParameters(width=canvas[0], height=canvas[1], resize_type=mode, pixel_format=fcc, planes_pos=pos, normalization=False)
    fp10 = ts.FrameParameters(width=canvas[0], height=canvas[1], resize_type=mode, pixel_format=fcc, planes_pos=pos, normalization=True)
    got8, used8 = v.convert_letterbox([torch.from_numpy(f[0]).cuda() for f in host], [torch.from_numpy(f[1]).cuda() for f in host], fp8, pad=pads[0], **kw)
    placed = [P.embed(f[2], f[3], *s, layout_of(1, k)) for k, (f, s) in enumerate(zip(host, sizes))]
    got10, used10 = v.convert_letterbox_p010([p[0] for p in placed], [p[1] for p in placed], fp10, pad=pads[1], **kw)
    torch.cuda.synchronize()
    assert [tuple(u) for u in used8] == [tuple(u) for u in used10] == P.rects_of(sizes, canvas, rects)
    c = 1 if fcc == M.Y800 else 3
    shape = (c, canvas[1], canvas[0])
    return ([g.cpu().numpy().reshape(shape) for g in got8], [g.cpu().numpy().reshape(shape) for g in got10], [(f[2], f[3]) for f in host], sizes, canvas,
            P.rects_of(sizes, canvas, rects))


def recover(q):
    """k of the fp32 quotients q = k / 1023: the rounding is undone and the quotient's bits are checked"""
    k = np.rint(q.astype(np.float64) * 1023).astype(np.int64)
    assert k.min() >= 0 and k.max() <= 1023 and np.array_equal(M.quotient(k).view(np.uint32), q.view(np.uint32)), "an output that is no k / 1023"
    return k


@pytest.mark.parametrize("pads", PADS, ids=["gray", "odd"])
@pytest.mark.parametrize("i", range(4))
@pytest.mark.parametrize("mode", [M.NEAREST, M.BILINEAR])
def test_luma_is_four_times_the_8_bit_calls(vpp, mode, i, pads):
    got8, got10, _, sizes, canvas, _ = both_calls(vpp, i, mode, M.Y800, pads)
    for k in range(len(sizes)):
        bad = int(np.sum((recover(got10[k]) >> 2) != got8[k]))
        assert bad == 0, f"launch {i} frame {k} {sizes[k]} -> {canvas} mode={mode}: {bad} of {got8[k].size} luma samples differ from the 8-bit call's"


@pytest.mark.parametrize("pads", PADS, ids=["gray", "odd"])
@pytest.mark.parametrize("i", range(4))
@pytest.mark.parametrize("mode", [M.NEAREST, M.BILINEAR])
def test_chroma_is_four_times_the_8_bit_calls(mode, i, pads):
    """in a private context whose coefficient block makes R the V sample and B the U sample (G is 0) in both calls; the session's context is never altered"""
    import tensor_stream as ts
    v = ts.VideoProcessor(device=0, max_consumers=1)
    try:
        v.set_option(ts.vpp.OPT_UNSAFE_COEFFS, 1)
        v.set_coeffs(SWAP)
        got8, got10, frames, sizes, canvas, rects = both_calls(v, i, mode, M.RGB24, pads)
        torch.cuda.synchronize()
    finally:
        v.Close()
    block = tuple(np.float32(c) for c in SWAP)
    for k in range(len(sizes)):
        what = f"launch {i} frame {k} {sizes[k]} -> {canvas} mode={mode}"
        k10 = recover(got10[k])
        Y, U, V = M.virtual_frame(*frames[k], *sizes[k], rects[k], canvas, mode, pads[1])
        assert np.array_equal(k10, M.channels(Y, U, V, M.RGB24, 0, block)), what + ": not the model's channels under the block"
        assert np.array_equal(k10[0], np.repeat(np.repeat(V, 2, 0), 2, 1)) and np.array_equal(k10[2], np.repeat(np.repeat(U, 2, 0), 2, 1)) and not k10[1].any(), what
        bad = int(np.sum((k10 >> 2) != got8[k]))
        assert bad == 0, what + f": {bad} of {got8[k].size} channel values differ from the 8-bit call's"


# ---- options -----------------------------------------------------------------------------------------------------------------------------------------------------
# (Y, U, V) on which the three variants of the green term give different k (the first five: different bytes too), found with the model; the last reaches the clamps
TRIPLES = [(407, 853, 729), (462, 966, 778), (437, 716, 828), (392, 729, 777), (651, 920, 992), (382, 711, 823), (487, 734, 902), (295, 411, 887), (72, 969, 137),
           (156, 943, 271), (489, 803, 975), (409, 772, 852), (419, 779, 783), (680, 984, 956), (99, 849, 333), (1000, 30, 1000)]
SIZE, CANVAS = (72, 56), (64, 64)


def blocks_frame():
    """72 x 56 in 4 x 4 flat blocks of 18 x 14 luma samples, one triple each, random low six bits"""
    y, uv = P.frame(*SIZE, 77)
    for n, (Y, U, V) in enumerate(TRIPLES):
        r, c = 14 * (n // 4), 18 * (n % 4)
        y[r:r + 14, c:c + 18] = (Y << 6) | (y[r:r + 14, c:c + 18] & 63)
        uv[r // 2:r // 2 + 7, c:c + 18:2] = (U << 6) | (uv[r // 2:r // 2 + 7, c:c + 18:2] & 63)
        uv[r // 2:r // 2 + 7, c + 1:c + 18:2] = (V << 6) | (uv[r // 2:r // 2 + 7, c + 1:c + 18:2] & 63)
    return y, uv


@pytest.fixture
def private():
    import tensor_stream as ts
    v = ts.VideoProcessor(device=0, max_consumers=1)
    try:
        yield v
    finally:
        v.Close()


def run(v, fr, mode, flavour, g_term, block):
    rect = P.rects_of([SIZE], CANVAS)[0]
    got, _ = P.convert(v, [fr], [SIZE], CANVAS, mode, flavour, CLAMPS, planes_dev=tuple([p] for p in P.embed(*fr, *SIZE, P.LAYOUTS[2])[:2]))
    torch.cuda.synchronize()
    ref = P.want(fr, SIZE, rect, CANVAS, mode, flavour, CLAMPS, g_term, block)
    P.same(got[0], ref, f"g_term {g_term} mode={mode} {flavour}")
    return ref


@pytest.mark.parametrize("flavour", ["u8_merged", "f32_planar", "f16_tensor"])
def test_the_green_term_option_is_honoured(private, flavour):
    """TSVPP_OPT_COLOR_G_TERM 1 and 2 against the model's variants, then 0 again; the flat blocks (NEAREST keeps their triples) make the three expectations differ"""
    import tensor_stream as ts
    blocks, noise = blocks_frame(), P.frame(*SIZE, 78)
    ref = {}
    for g_term in (1, 2, 0):
        private.set_option(ts.vpp.OPT_COLOR_G_TERM, g_term)
        ref[g_term] = run(private, blocks, M.NEAREST, flavour, g_term, M.COEFFS)
        run(private, noise, M.BILINEAR, flavour, g_term, M.COEFFS)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert int(np.sum(ref[a] != ref[b])) >= 64, f"variants {a} and {b} expect the same bits: the content is no probe"


@pytest.mark.parametrize("flavour", ["u8_merged", "f32_planar", "f16_tensor"])
def test_the_coefficient_block_is_honoured(private, flavour):
    """the BT.709 limited-range literals (tests/p010_cases.py: BT709) instead of the default BT.601 ones, with each green term"""
    import tensor_stream as ts
    private.set_option(ts.vpp.OPT_UNSAFE_COEFFS, 1)
    private.set_coeffs([float(c) for c in BT709])
    blocks, noise = blocks_frame(), P.frame(*SIZE, 79)
    for g_term in (0, 2):
        private.set_option(ts.vpp.OPT_COLOR_G_TERM, g_term)
        ref = run(private, blocks, M.NEAREST, flavour, g_term, BT709)
        assert int(np.sum(ref != P.want(blocks, SIZE, P.rects_of([SIZE], CANVAS)[0], CANVAS, M.NEAREST, flavour, CLAMPS, g_term))) >= ref.size // 4
        run(private, noise, M.BILINEAR, flavour, g_term, BT709)
