"""Frame content that sits on the truncation boundaries of the arithmetic, for the bit-exact tests (tests/test_gpu_edge_content.py, tests/test_edge_content_cpu.py).
Every sampler ends in a truncation to 8 bits; on random content a weight one ulp off moves the value in front of the truncation by ~1e-5 and flips one pixel in
~1e5.  On the classes below 7 .. 47 % of the samples sit ON the boundary: the reference's own float arithmetic returns c or c - 1 for a flat frame of level c, and
the pattern of the two is a fingerprint of every weight and every rounding.  Contains no product code and touches no device: numpy only.

    flat_<Y>_<U>_<V>   every luma byte Y, every chroma pair (U, V)
    checker            luma 255 * ((r + x) & 1); U = 255 * ((r + cx) & 1), V = 255 - U: the largest BICUBIC overshoot, clamps in both directions
    edge_v, edge_h     0 on one side, 255 on the other of an odd column ((cols // 2) | 1) / an odd row ((rows // 2) | 1); chroma by the same rule on its own grid
                       (cols = pairs), U = V
    ramp               luma (x + 3 r) & 255; U = (2 cx + r) & 255, V = 255 - U: blends of a ramp land on or next to integers

Every byte outside the picture -- the pitch padding, the lead-in in front of a plane and the 16 bytes behind it -- holds a value the pixels next to it do not
have: 255 - c for a flat frame (chroma: 255 - U on even bytes, 255 - V on odd ones), 0x5A elsewhere.  A read past the picture therefore shows."""
import numpy as np

FLATS = ((255, 128, 128), (200, 90, 240), (17, 16, 240), (0, 255, 0))
CLASSES = tuple("flat_%d_%d_%d" % f for f in FLATS) + ("checker", "edge_v", "edge_h", "ramp")
PAD = 0x5A
TRAIL = 16  # bytes behind a plane, as the fuzz generators allocate them


# ---- the named AREA cases -----------------------------------------------------------------------------------------------------------------------------------
# The periods the jump start of the AREA letterbox kernel exists for, and the generator's scales of tests/test_rois_area_cpu.py, at content that shows a wrong
# weight.  A case probes only if the reference itself lands on the boundary: tests/test_edge_content_cpu.py holds the share of 254 in the reference's luma of a
# flat 255 frame at 5 % or more for every case.  Four of the original cases are exact in float32 and measured too little; each is replaced by its neighbour:
#     192 x 108 -> 64 x 36 (ratio 3)  0 %  ->  190 x 110 -> 64 x 36
#     448 -> 224 (ratio 2)            0 %  ->  446 -> 224
#     336 -> 224 (ratio 1.5)          0 %  ->  338 -> 224
#     226 -> 224                    1.5 %  ->  302 -> 224 (period 112, as 226's)
# (frame (w, h, pitch), canvas, rectangle (left, top, width, height)): tests/test_gpu_letterbox_area.py's PERIODS with the first replaced, 322 x 182 -> 70 x 66
# and 250 x 140 -> 64 x 36
LETTERBOX_AREA_CASES = [
    ((190, 110, 192), (64, 64), (0, 14, 64, 36)),
    ((240, 180, 256), (100, 100), (0, 12, 100, 76)),
    ((200, 150, 208), (96, 64), (10, 4, 76, 58)),
    ((214, 182, 224), (70, 66), (0, 0, 70, 66)),
    ((322, 182, 384), (64, 64), (0, 14, 64, 36)),
    ((322, 182, 384), (70, 66), (0, 0, 70, 66)),
    ((250, 140, 256), (64, 64), (0, 14, 64, 36)),
]
# (box (left, top, right, bottom) of a ROIS_AREA_FRAME frame, output size) through convert_rois_area: even, odd-left, odd-top and both-odd origins
ROIS_AREA_FRAME = (448, 448, 480)  # (w, h, pitch)
ROIS_AREA_CASES = [
    ((0, 0, 446, 446), (224, 224)),
    ((11, 21, 349, 359), (224, 224)),
    ((100, 31, 400, 331), (224, 224)),
    ((101, 40, 403, 342), (224, 224)),
    ((60, 200, 382, 382), (70, 66)),
    ((7, 9, 257, 149), (64, 36)),
]
NAMED_CLASSES = tuple("flat_%d_%d_%d" % f for f in FLATS) + ("ramp",)


def named_area_geometries():
    """(source w, h, output w, h) of every named case: what decides the weights"""
    out = [(w, h, r[2], r[3]) for (w, h, _), _, r in LETTERBOX_AREA_CASES]
    return out + [(b[2] - b[0], b[3] - b[1], d[0], d[1]) for b, d in ROIS_AREA_CASES]


def flat_levels(name):
    """(Y, U, V) of a flat class, None for any other"""
    if not name.startswith("flat_"):
        return None
    y, u, v = (int(s) for s in name.split("_")[1:])
    return y, u, v


def _picture(name, rows, cols, chroma):
    """the rows x cols bytes of the picture itself (chroma: cols bytes = cols // 2 pairs)"""
    r = np.arange(rows, dtype=np.int64)[:, None]
    if not chroma:
        x = np.arange(cols, dtype=np.int64)[None, :]
        if name == "checker":
            pic = 255 * ((r + x) & 1)
        elif name == "edge_v":
            pic = np.where(x >= ((cols // 2) | 1), 255, 0) + 0 * r
        elif name == "edge_h":
            pic = np.where(r >= ((rows // 2) | 1), 255, 0) + 0 * x
        elif name == "ramp":
            pic = (x + 3 * r) & 255
        else:
            pic = np.full((rows, cols), flat_levels(name)[0], np.int64)
        return pic.astype(np.uint8)
    pairs = cols // 2
    cx = np.arange(pairs, dtype=np.int64)[None, :]
    if name == "checker":
        u = 255 * ((r + cx) & 1)
        v = 255 - u
    elif name == "edge_v":
        u = v = np.where(cx >= ((pairs // 2) | 1), 255, 0) + 0 * r
    elif name == "edge_h":
        u = v = np.where(r >= ((rows // 2) | 1), 255, 0) + 0 * cx
    elif name == "ramp":
        u = (2 * cx + r) & 255
        v = 255 - u
    else:
        _, fu, fv = flat_levels(name)
        u, v = np.full((rows, pairs), fu, np.int64), np.full((rows, pairs), fv, np.int64)
    pic = np.empty((rows, 2 * pairs), np.uint8)
    pic[:, 0::2] = u
    pic[:, 1::2] = v
    return pic


def outside(name, count, chroma, first=0):
    """`count` bytes of what lies outside the picture; `first`: the index, relative to the plane's first byte, of the first of them (chroma: its parity chooses
    between 255 - U and 255 - V)"""
    lv = flat_levels(name)
    if lv is None:
        return np.full(count, PAD, np.uint8)
    if not chroma:
        return np.full(count, 255 - lv[0], np.uint8)
    k = np.arange(first, first + count, dtype=np.int64)
    return np.where(k & 1, 255 - lv[2], 255 - lv[1]).astype(np.uint8)


def buffer(name, rows, cols, pitch, chroma, off=0):
    """(flat, plane): a flat uint8 buffer of off + rows * pitch + TRAIL bytes and the plane (rows x pitch) as a view of it that starts `off` bytes in"""
    assert pitch >= cols and name in CLASSES, (name, cols, pitch)
    flat = np.empty(off + rows * pitch + TRAIL, np.uint8)
    flat[:off] = outside(name, off, chroma, -off)
    flat[off + rows * pitch:] = outside(name, TRAIL, chroma, rows * pitch)
    plane = flat[off:off + rows * pitch].reshape(rows, pitch)
    for r in range(rows if pitch > cols else 0):
        plane[r, cols:] = outside(name, pitch - cols, chroma, r * pitch + cols)
    plane[:, :cols] = _picture(name, rows, cols, chroma)
    return flat, plane


def make(name, rows, cols, pitch, chroma):
    """one plane, rows x pitch; the picture is its first `cols` byte columns"""
    return buffer(name, rows, cols, pitch, chroma)[1]


def frame(name, w, h, pitch_y, pitch_uv):
    """(y, uv) of an NV12 frame of w x h"""
    return make(name, h, w, pitch_y, False), make(name, h // 2, w, pitch_uv, True)


def planes(name, fr):
    """what tile_fuzz.planes returns, for a frame dict {w, h, pitch_y, pitch_uv, off_y, off_uv} of the fuzz generators: (flat_y, flat_uv, y, uv)"""
    flat_y, y = buffer(name, fr["h"], fr["w"], fr["pitch_y"], False, fr["off_y"])
    flat_uv, uv = buffer(name, fr["h"] // 2, fr["w"], fr["pitch_uv"], True, fr["off_uv"])
    return flat_y, flat_uv, y, uv


def complement(plane):
    """255 - x, every byte: the second frame of a two-frame batch"""
    return (255 - plane.astype(np.int16)).astype(np.uint8)


def with_content(call, name):
    """a copy of a fuzz call whose every frame draws the class `name`: the key "content" on every frame dict (tile_fuzz's frames and those of the remap and mesh
    generators) and on the call itself (letterbox_area_fuzz, whose frames are tuples)"""
    out = dict(call, content=name)
    out["frames"] = [dict(fr, content=name) if isinstance(fr, dict) else fr for fr in call["frames"]]
    return out
