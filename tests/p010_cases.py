"""Shared by the GPU tests of tsvpp_convert_letterbox_p010: the output flavours, the seeded frames, the call itself and the expected bits (tests/p010_util.py, the
numpy restatement of the contract) -- and the plane layouts: a frame embedded in one larger int16 device buffer whose every other word is 0xFFFF, its planes handed
over as strided views at a chosen word offset and pitch.  Contains no product code."""
import numpy as np

import p010_util as M
import tensor_util as T
from letterbox_util import default_rect

BLACK = (64, 512, 512)
GRAY = (456, 512, 512)
# name -> (fourcc, planes, normalization, (dtype, spec) of a tensor or None)
FLAVOURS = {"u8_merged": (M.RGB24, M.MERGED, False, None), "f32_planar": (M.BGR24, M.PLANAR, True, None), "f16_tensor": (M.RGB24, M.PLANAR, True, (T.F16, T.IMAGENET)),
            "y800_f32": (M.Y800, M.MERGED, True, None), "y800_u8": (M.Y800, M.MERGED, False, None), "y800_f16": (M.Y800, M.MERGED, True, (T.F16, T.IDENTITY)),
            "f32_merged": (M.RGB24, M.MERGED, True, None), "u8_planar": (M.BGR24, M.PLANAR, False, None), "bf16_tensor": (M.BGR24, M.PLANAR, True, (T.BF16, T.IMAGENET)),
            "f32_tensor": (M.RGB24, M.PLANAR, True, (T.F32, T.IMAGENET))}
FOUR = ["u8_merged", "f32_planar", "f16_tensor", "y800_f32"]
# a coefficient block with nothing trivial in it: the BT.709 limited-range literals, as float32, in tsvpp_coeffs' order (p010_util.COEFFS holds the default block)
BT709 = tuple(np.float32(v) for v in (1.164384, 1.792741, 2.112402, -0.532909, -0.213249, 0.5, 16.0, 128.0))


def frame(w, h, seed, pitch=None, fill=None):
    """(y, uv) uint16 planes of `pitch` words: random samples with random low six bits; `fill`: the words of the padding columns"""
    rng = np.random.default_rng(seed)
    pitch = pitch or w
    y = rng.integers(0, 65536, (h, pitch), dtype=np.uint16)
    uv = rng.integers(0, 65536, (h // 2, pitch), dtype=np.uint16)
    if fill is not None:
        y[:, w:] = fill
        uv[:, w:] = fill
    return y, uv


def frame_of_bytes(w, h, seed):
    """(y8, uv8, y, uv): tight uint8 planes b and the P010 words (b << 8) | r with random low six bits r -- the samples are 4 b"""
    rng = np.random.default_rng(seed)
    y8, uv8 = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)
    y = (y8.astype(np.uint16) << 8) | rng.integers(0, 64, (h, w), dtype=np.uint16)
    uv = (uv8.astype(np.uint16) << 8) | rng.integers(0, 64, (h // 2, w), dtype=np.uint16)
    return y8, uv8, y, uv


def dev(a):
    import torch
    return torch.from_numpy(a.view(np.int16)).cuda()


def stored(k, flavour):
    """channel values k (c, ch, cw) -> the raw bytes of the flavour's output"""
    _, planes, norm, tensor = FLAVOURS[flavour]
    if tensor is None:
        return M.stored(k, planes, norm)
    return T.expected(M.quotient(k), k.shape[0], tensor[1], tensor[0])


def want(fr, size, rect, canvas, mode, flavour, pad, g_term=0, k=M.COEFFS):
    return stored(M.channels(*M.virtual_frame(fr[0], fr[1], *size, rect, canvas, mode, pad), FLAVOURS[flavour][0], g_term, k), flavour)


def params(canvas, mode, flavour):
    import tensor_stream as ts
    fcc, planes, norm, tensor = FLAVOURS[flavour]
    fp = ts.FrameParameters(width=canvas[0], height=canvas[1], resize_type=mode, pixel_format=fcc, planes_pos=planes, normalization=norm)
    return fp, ({} if tensor is None else dict(dtype=T.TORCH[tensor[0]], mean=tensor[1][0], std=tensor[1][1]))


def convert(vpp, frames, sizes, canvas, mode, flavour, pad=BLACK, rects=None, planes_dev=None, out=None):
    fp, kw = params(canvas, mode, flavour)
    ys, uvs = planes_dev or ([dev(f[0]) for f in frames], [dev(f[1]) for f in frames])
    return vpp.convert_letterbox_p010(ys, uvs, fp, pad=pad, rects=rects, out=out, width=[s[0] for s in sizes], height=[s[1] for s in sizes], **kw)


def rects_of(sizes, canvas, rects=None):
    return [tuple(r) for r in rects] if rects else [default_rect(*s, *canvas) for s in sizes]


def same(got, ref, what):
    g = T.bits(got)
    assert g.size == ref.size, what
    bad = np.flatnonzero(g != ref)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at {bad[:4]}"


def check(vpp, frames, sizes, canvas, mode, flavour, pad=BLACK, rects=None):
    import torch
    got, used = convert(vpp, frames, sizes, canvas, mode, flavour, pad, rects)
    torch.cuda.synchronize()
    for k, (fr, size) in enumerate(zip(frames, sizes)):
        rect = tuple(rects[k]) if rects else default_rect(*size, *canvas)
        assert tuple(used[k]) == rect
        same(got[k], want(fr, size, rect, canvas, mode, flavour, pad), f"frame {k} {size} -> {canvas} rect {rect} mode={mode} {flavour}")
    return got


# ---- plane layouts ---------------------------------------------------------------------------------------------------------------------------------------------
OUTSIDE = 0xFFFF  # every word of an embedding buffer that is not a word of the picture
ALIGN = 8         # words: the buffer and each plane's slot start on a 16-byte boundary
# (luma offset, luma pitch - w, chroma offset, chroma pitch - w), in WORDS.  A chroma pair is 4-byte aligned (`uv4`, csrc/vpp_letterbox_p010_core.h) where the
# chroma offset and pitch are both even words.  In order: tight; uv4 false by an odd pitch; uv4 false by an odd offset under an even pitch; uv4 true at an offset of
# 4 bytes (322 words of pitch: 644 bytes, 4 mod 16); uv4 true at a pitch of w + 2 words (4 mod 16 bytes for every w that is a multiple of 8) and an offset of 8
# bytes; luma and chroma both at w + 1 words.  Offsets 0, 1, 2, 3, 5 words: addresses 0, 2, 4, 6, 10 mod 16.  Four of the six have differing pitches.
LAYOUTS = [(0, 0, 0, 0), (1, 1, 2, 3), (2, 3, 1, 8), (3, 8, 2, 0), (5, 3, 4, 2), (0, 1, 5, 1)]


def uv4(layout, w):
    return layout[2] % 2 == 0 and (w + layout[3]) % 2 == 0


def byte_pitches(layout, w):
    return 2 * (w + layout[1]), 2 * (w + layout[3])


def embed_host(y, uv, w, h, layout):
    """(buffer, first word of luma, of chroma): a flat uint16 buffer of OUTSIDE words with the w x h picture of (y, uv) at the layout's offsets and pitches; 16
    bytes of OUTSIDE lead in, separate the planes and trail"""
    off_y, dy, off_uv, duv = layout
    py, puv = w + dy, w + duv
    at_y = ALIGN + off_y
    slot_uv = -(-(at_y + h * py + ALIGN) // ALIGN) * ALIGN
    at_uv = slot_uv + off_uv
    buf = np.full(-(-(at_uv + (h // 2) * puv + ALIGN) // ALIGN) * ALIGN, OUTSIDE, np.uint16)
    buf[at_y:at_y + h * py].reshape(h, py)[:, :w] = y[:h, :w]
    buf[at_uv:at_uv + (h // 2) * puv].reshape(h // 2, puv)[:, :w] = uv[:h // 2, :w]
    return buf, at_y, at_uv


def embed(y, uv, w, h, layout):
    """(y plane, uv plane, buffer) on the device: int16 views of w columns with unit column stride, data_ptr() at the layout's word offset from a 16-byte-aligned
    base, the row stride the layout's pitch"""
    host, at_y, at_uv = embed_host(y, uv, w, h, layout)
    buf = dev(host)
    assert buf.data_ptr() % 16 == 0
    ty = buf.as_strided((h, w), (w + layout[1], 1), at_y)
    tuv = buf.as_strided((h // 2, w), (w + layout[3], 1), at_uv)
    assert ty.data_ptr() == buf.data_ptr() + 2 * at_y and (ty.data_ptr() - 2 * layout[0]) % 16 == 0 and (tuv.data_ptr() - 2 * layout[2]) % 16 == 0
    return ty, tuv, buf
