"""No GPU: independent witnesses for tests/p010_util.py, the model every P010 test takes its expected bits from.

A1  the resize stage against the 8-bit oracle.  For bytes b the P010 words (b << 8) | r have the samples 4 b.  Every float32 step of the contract's blend scales
    exactly by that power of two, so the 10-bit blend is four times the 8-bit blend before the truncation, and floor(4 s) >> 2 == floor(s): the model's Y, U and V,
    each >> 2, are the oracle's 8-bit result for the same bytes -- luma from its Y800 output, chroma from its NV12 output.  Whole canvases, no sample left out.
A2  the colour stage against exact arithmetic: p010_util.channels held to an evaluation in fractions.Fraction in which every step of the contract is rounded once to
    float32 (a fused step once after the exact product-sum), written without warp_util.fma32.  Equality of k everywhere.
E   the condition of tests/p010_content.py: the model puts a flat 1023 frame on the truncation boundary in at least 5 % of the samples of every named geometry."""
from fractions import Fraction

import numpy as np
import pytest

import p010_content as C
import p010_util as M
from letterbox_util import default_rect
import p010_cases as P
from p010_cases import BT709, frame_of_bytes

NV12_OUT = 3
# (frame w x h, canvas, rectangle or None for the default one).  The last two: left % 4 == 2 and an odd top / 2, a down-scale and an up-scale
RESIZE = [((72, 56), (64, 64), None), ((40, 24), (64, 64), None), ((322, 182), (70, 66), None), ((2, 2), (66, 34), None), ((128, 72), (30, 34), None),
          ((98, 54), (64, 36), None), ((72, 56), (96, 96), (6, 34, 52, 40)), ((40, 24), (64, 64), (10, 6, 44, 26))]
PAD8 = (114, 77, 201)


@pytest.mark.parametrize("mode", [M.NEAREST, M.BILINEAR])
@pytest.mark.parametrize("size,canvas,rect", RESIZE, ids=["%dx%d-%dx%d%s" % (*s, *c, "-rect" if r else "") for s, c, r in RESIZE])
def test_resize_stage_is_the_oracles_on_bytes(oracle, size, canvas, rect, mode):
    (w, h), (cw, ch) = size, canvas
    rect = rect or default_rect(w, h, cw, ch)
    left, top, iw, ih = rect
    assert rect[0] % 2 == 0 and rect[1] % 2 == 0
    y8, uv8, y, uv = frame_of_bytes(w, h, 900 + w + h + mode)
    pitch = w + 1 + 2 * mode  # words: the model reads planes of any pitch
    yp, uvp = np.full((h, pitch), 0xFFFF, np.uint16), np.full((h // 2, pitch), 0xFFFF, np.uint16)
    yp[:, :w], uvp[:, :w] = y, uv
    Y, U, V = M.virtual_frame(yp, uvp, w, h, rect, canvas, mode, tuple(4 * p + k for k, p in enumerate(PAD8)))  # (pads 4 p + 0 / 1 / 2: >> 2 gives p)
    luma = oracle.convert(y8, uv8, dst=(iw, ih), resize_type=mode, fourcc=M.Y800, planes=M.MERGED, normalization=False)[0].view(np.uint8).ravel()
    nv12 = oracle.convert(y8, uv8, dst=(iw, ih), resize_type=mode, fourcc=NV12_OUT, planes=M.MERGED, normalization=False)[0].view(np.uint8).ravel()
    assert luma.size == iw * ih and nv12.size == iw * ih * 3 // 2 and np.array_equal(nv12[:iw * ih], luma)
    want_y = np.full((ch, cw), PAD8[0], np.int64)
    want_y[top:top + ih, left:left + iw] = luma.reshape(ih, iw)
    chroma = nv12[iw * ih:].reshape(ih // 2, iw // 2, 2)
    for name, got, pad, inner in (("U", U, PAD8[1], chroma[:, :, 0]), ("V", V, PAD8[2], chroma[:, :, 1])):
        want = np.full((ch // 2, cw // 2), pad, np.int64)
        want[top // 2:(top + ih) // 2, left // 2:(left + iw) // 2] = inner
        assert got.shape == want.shape and np.array_equal(got >> 2, want), f"{name}: {int(np.sum((got >> 2) != want))} of {want.size} samples differ"
    assert Y.shape == want_y.shape and np.array_equal(Y >> 2, want_y), f"Y: {int(np.sum((Y >> 2) != want_y))} of {want_y.size} samples differ"


# ---- A2 ----------------------------------------------------------------------------------------------------------------------------------------------------------
def rn32(x):
    """the float32 nearest to the rational x, ties to even, as a Fraction: ONE rounding, in integer arithmetic (normal range only)"""
    x = Fraction(x)
    if x == 0:
        return x
    sign, a = (-1 if x < 0 else 1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()  # 2^(e-1) < a < 2^(e+1)
    if a < Fraction(2) ** e:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1) and -126 <= e <= 127, "outside float32's normal range"
    ulp = Fraction(2) ** (e - 23)
    q = a / ulp
    n = q.numerator // q.denominator
    rest = q - n
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n & 1):
        n += 1
    return sign * n * ulp


def exact(v):
    """a float32 as a Fraction"""
    return Fraction(float(np.float32(v)))


def test_rn32_is_float32_rounding():
    rng = np.random.default_rng(3)
    for a, b in zip(rng.standard_normal(200).astype(np.float32), (rng.standard_normal(200) * 1000).astype(np.float32)):
        assert rn32(exact(a) * exact(b)) == exact(a * b) and rn32(exact(a) + exact(b)) == exact(a + b)
    assert rn32(Fraction(1, 3)) == exact(np.float32(1) / np.float32(3))
    assert rn32(Fraction((1 << 24) + 1)) == 1 << 24 and rn32(Fraction((1 << 24) + 3)) == (1 << 24) + 4  # ties to even


UV_PAIRS = [(0, 0), (0, 1023), (1023, 0), (1023, 1023)] + [(u, v) for u in (511, 512, 513) for v in (511, 512, 513)] + \
    [tuple(int(t) for t in p) for p in np.random.default_rng(20261126).integers(0, 1024, (4, 2))]


def colour_exact(block):
    """{(g_term, U, V): (R, G, B) arrays over Y = 0..1023}, every step of the contract in exact arithmetic and rounded once"""
    y_scale, v_to_r, u_to_b, v_to_g, u_to_g, bias, y_off, c_off = (exact(c) for c in block)
    y4, c4 = rn32(4 * y_off), rn32(4 * c_off)
    yv = [rn32(max(Fraction(0), rn32(Y - y4)) * y_scale) for Y in range(1024)]

    def channel(term):
        return np.array([min(max(int(rn32(t + term)), 0), 1023) for t in yv])  # int(): truncation toward zero

    out = {}
    for U, V in UV_PAIRS:
        u, v = rn32(U - c4), rn32(V - c4)
        r, b = channel(rn32(v * v_to_r + bias)), channel(rn32(u * u_to_b + bias))
        greens = (rn32(v * v_to_g + rn32(u * u_to_g)), rn32(rn32(v * v_to_g) + rn32(u * u_to_g)), rn32(u * u_to_g + rn32(v * v_to_g)))
        for g_term, g in enumerate(greens):
            out[(g_term, U, V)] = (r, channel(rn32(g + bias)), b)
    return out


@pytest.mark.parametrize("block", [M.COEFFS, BT709], ids=["default", "bt709"])
def test_colour_stage_against_exact_arithmetic(block):
    assert len(UV_PAIRS) == 17
    ref = colour_exact(block)
    Y = np.arange(1024, dtype=np.int64).reshape(2, 512)
    for (g_term, U, V), rgb in ref.items():
        Up, Vp = np.full((1, 256), U, np.int64), np.full((1, 256), V, np.int64)
        for fcc, order in ((M.RGB24, rgb), (M.BGR24, rgb[::-1])):
            k = M.channels(Y, Up, Vp, fcc, g_term, block)
            assert k.shape == (3, 2, 512)
            for c in range(3):
                assert np.array_equal(k[c].ravel(), order[c]), (g_term, U, V, fcc, c, np.flatnonzero(k[c].ravel() != order[c])[:4])
    assert np.array_equal(M.channels(Y, Up, Vp, M.Y800)[0], Y)


# ---- E -----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_flat_1023_frame_puts_the_model_on_the_boundary():
    """the 5 % rule of tests/test_edge_content_cpu.py: a geometry whose share of 1022 measures less is no probe and has no place in p010_content.GEOMETRIES"""
    for (w, h), canvas in C.GEOMETRIES:
        left, top, iw, ih = rect = default_rect(w, h, *canvas)
        y, uv = C.frame("flat_1023_512_512", w, h, w + 3, w + 1)
        Y, U, V = M.virtual_frame(y, uv, w, h, rect, canvas, M.BILINEAR, (0, 0, 0))
        luma = Y[top:top + ih, left:left + iw]
        share = float(np.mean(luma == 1022))
        y2, uv2 = C.frame("flat_800_361_963", w, h)
        _, U2, _ = M.virtual_frame(y2, uv2, w, h, rect, canvas, M.BILINEAR, (0, 0, 0))
        cu = U2[top // 2:(top + ih) // 2, left // 2:(left + iw) // 2]
        print(f"{w} x {h} -> {canvas[0]} x {canvas[1]}: {100 * share:.1f} % of {luma.size} luma samples are 1022; {100 * float(np.mean(cu == 360)):.1f} % of U are 360")
        assert set(np.unique(luma).tolist()) <= {1022, 1023} and set(np.unique(cu).tolist()) <= {360, 361}
        assert share >= 0.05, (w, h, canvas, share)


# ---- the plane layouts of tests/test_gpu_letterbox_p010_layout.py ---------------------------------------------------------------------------------------------
def test_the_layouts_cover_what_they_are_there_for():
    w = 72
    assert {l[0] for l in P.LAYOUTS} | {l[2] for l in P.LAYOUTS} >= {0, 1, 2, 3, 5}
    assert {l[1] for l in P.LAYOUTS} | {l[3] for l in P.LAYOUTS} >= {0, 1, 3, 8}
    assert 2 * sum(1 for l in P.LAYOUTS if l[1] != l[3]) >= len(P.LAYOUTS)
    assert any(not P.uv4(l, w) and (w + l[3]) % 2 for l in P.LAYOUTS), "uv4 false by an odd-word chroma pitch"
    assert any(not P.uv4(l, w) and (w + l[3]) % 2 == 0 and l[2] % 2 for l in P.LAYOUTS), "uv4 false by an odd-word chroma offset under an even-word pitch"
    assert any(P.uv4(l, w) and P.byte_pitches(l, w)[1] % 16 == 4 for l in P.LAYOUTS), "uv4 true with a pitch that is 4 but not 16 bytes aligned"
    host, at_y, at_uv = P.embed_host(*P.frame(w, 6, 1), w, 6, P.LAYOUTS[4])
    assert at_y % P.ALIGN == 5 and at_uv % P.ALIGN == 4 and int(np.sum(host != P.OUTSIDE)) <= w * 9 and (host[:P.ALIGN] == P.OUTSIDE).all() and (host[-P.ALIGN:] == P.OUTSIDE).all()
