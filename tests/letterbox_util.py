"""Shared by the letterbox tests: the expected canvas of tsvpp_convert_letterbox, built from the existing oracle only, and the integer rule of the default
rectangle restated in Python."""
import numpy as np

NEAREST, BILINEAR, BICUBIC, AREA = 0, 1, 2, 3
Y800, RGB24, BGR24 = 0, 1, 2
PLANAR, MERGED = 0, 1

FLAVOURS = [(fcc, planes, norm) for fcc in (RGB24, BGR24) for planes in (PLANAR, MERGED) for norm in (False, True)] + [(Y800, MERGED, False), (Y800, MERGED, True)]

# the frames of the letterbox GPU tests, (width, height, pitch): pad above and below; pad left and right (in 64 x 64: 36 x 64 at left 14, the rectangle's edge
# splits 4-column thread tiles); no pad in 64 x 64 (the plain colour conversion); an up-scale; a frame a tile's footprint of which is several times the tile
GEO = [(128, 72, 192), (72, 128, 96), (64, 64, 80), (32, 18, 48), (322, 182, 384)]
# ... and their canvases.  70 x 66: 4 k + 2 columns (the shifted tile column); 30 x 34: narrower than a tile (element-wise stores)
CANVASES = [(64, 64), (96, 64), (70, 66), (30, 34)]


def default_rect(in_w, in_h, dst_w, dst_h):
    """(left, top, width, height): the rule of include/tsvpp.h, in Python's unbounded integers"""
    if in_w * dst_h >= in_h * dst_w:
        width = dst_w
        height = min(max(2 * ((in_h * dst_w + in_w) // (2 * in_w)), 2), dst_h)
    else:
        height = dst_h
        width = min(max(2 * ((in_w * dst_h + in_h) // (2 * in_h)), 2), dst_w)
    return (((dst_w - width) // 2) & ~1, ((dst_h - height) // 2) & ~1, width, height)


def pad_pixel(oracle, pad, fcc, planes, norm):
    """what the colour back end makes of the constant sample: the oracle's conversion, without a resize, of a 2 x 2 frame of that constant -> (channels,)"""
    y = np.full((2, 2), pad[0], np.uint8)
    uv = np.array([[pad[1], pad[2]]], np.uint8)
    ref, _, _ = oracle.convert(y, uv, fourcc=fcc, planes=planes, normalization=norm)
    c = 1 if fcc == Y800 else 3
    px = ref.reshape(c, 2, 2)[:, 0, 0] if (fcc == Y800 or planes == PLANAR) else ref.reshape(2, 2, c)[0, 0, :]
    return px.copy()


def expected_canvas(oracle, y, uv, w, h, rect, canvas, rt, fcc, planes, norm, pad, inner=None):
    """the canvas as raw bytes: pad everywhere, then oracle.convert of the frame to the rectangle's size written into the rectangle.  `inner`: that block, if the
    caller has it already (flat, as oracle.convert returns it)."""
    cw, ch = canvas
    left, top, iw, ih = rect
    c = 1 if fcc == Y800 else 3
    px = pad_pixel(oracle, pad, fcc, planes, norm)
    if inner is None:
        inner, _, _ = oracle.convert(y[:h, :w], uv[:h // 2, :w], dst=(iw, ih), resize_type=rt, fourcc=fcc, planes=planes, normalization=norm)
    assert inner.dtype == px.dtype
    if fcc == Y800 or planes == PLANAR:
        out = np.empty((c, ch, cw), px.dtype)
        out[:] = px[:, None, None]
        out[:, top:top + ih, left:left + iw] = inner.reshape(c, ih, iw)
    else:
        out = np.empty((ch, cw, c), px.dtype)
        out[:] = px
        out[top:top + ih, left:left + iw, :] = inner.reshape(ih, iw, c)
    return out.ravel().view(np.uint8)


def bits(t):
    return t.contiguous().cpu().numpy().ravel().view(np.uint8)
