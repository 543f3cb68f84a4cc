"""Frame content that sits on the truncation boundaries of the P010 arithmetic: the classes of tests/edge_content.py on the 10-bit scale, as P010 words with random
low six bits throughout (the contract ignores them).  The BILINEAR blend ends in a truncation to 0..1023: the model's own float32 arithmetic returns c or c - 1 for
a flat frame of level c, and the pattern of the two is a fingerprint of every weight and every rounding (tests/test_letterbox_p010_witness_cpu.py holds the share
of 1022 in the luma of a flat 1023 frame at 5 % or more for every geometry below).  Contains no product code and touches no device: numpy only.

    flat_<Y>_<U>_<V>   every luma sample Y, every chroma pair (U, V)
    checker            luma 1023 * ((r + x) & 1); U = 1023 * ((r + cx) & 1), V = 1023 - U
    edge_v, edge_h     0 on one side, 1023 on the other of an odd column ((cols // 2) | 1) / an odd row ((rows // 2) | 1); chroma by the same rule on its own grid
                       (cols = pairs), U = V
    ramp               luma (x + 3 r) & 1023; U = (2 cx + r) & 1023, V = 1023 - U

Every word of the pitch padding holds a sample the picture next to it does not have: 1023 - c for a flat frame (chroma: 1023 - U, 1023 - V by parity), 361
elsewhere.  A read past the picture therefore shows."""
import numpy as np

FLATS = ((1023, 512, 512), (800, 361, 963), (68, 64, 960), (1, 1023, 0))
CLASSES = tuple("flat_%d_%d_%d" % f for f in FLATS) + ("checker", "edge_v", "edge_h", "ramp")
PAD = 361
# (frame w x h, canvas) with the default rectangle: the model lands on the boundary in 5.6 .. 11.7 % of the luma samples (profiles/letterbox_p010_tests.txt).
# 98 x 54 -> 64 x 36 measures 0 % and is no probe.
GEOMETRIES = [((72, 56), (64, 64)), ((40, 24), (64, 64)), ((322, 182), (70, 66)), ((190, 110), (64, 36)), ((46, 26), (96, 64))]


def flat_levels(name):
    """(Y, U, V) of a flat class, None for any other"""
    return tuple(int(s) for s in name.split("_")[1:]) if name.startswith("flat_") else None


def samples(name, rows, cols, chroma):
    """the picture as samples 0..1023: rows x cols luma samples, or rows x cols chroma words (cols // 2 pairs, U then V)"""
    r = np.arange(rows, dtype=np.int64)[:, None]
    if not chroma:
        x = np.arange(cols, dtype=np.int64)[None, :]
        if name == "checker":
            return 1023 * ((r + x) & 1)
        if name == "edge_v":
            return np.where(x >= ((cols // 2) | 1), 1023, 0) + 0 * r
        if name == "edge_h":
            return np.where(r >= ((rows // 2) | 1), 1023, 0) + 0 * x
        if name == "ramp":
            return (x + 3 * r) & 1023
        return np.full((rows, cols), flat_levels(name)[0], np.int64)
    pairs = cols // 2
    cx = np.arange(pairs, dtype=np.int64)[None, :]
    if name == "checker":
        u = 1023 * ((r + cx) & 1)
        v = 1023 - u
    elif name == "edge_v":
        u = v = np.where(cx >= ((pairs // 2) | 1), 1023, 0) + 0 * r
    elif name == "edge_h":
        u = v = np.where(r >= ((rows // 2) | 1), 1023, 0) + 0 * cx
    elif name == "ramp":
        u = (2 * cx + r) & 1023
        v = 1023 - u
    else:
        _, fu, fv = flat_levels(name)
        u, v = np.full((rows, pairs), fu, np.int64), np.full((rows, pairs), fv, np.int64)
    pic = np.empty((rows, 2 * pairs), np.int64)
    pic[:, 0::2] = u
    pic[:, 1::2] = v
    return pic


def outside(name, rows, count, chroma):
    """rows x count samples of the pitch padding behind a picture of an even number of words per row"""
    lv = flat_levels(name)
    if lv is None:
        return np.full((rows, count), PAD, np.int64)
    if not chroma:
        return np.full((rows, count), 1023 - lv[0], np.int64)
    k = np.arange(count, dtype=np.int64)[None, :] + np.zeros((rows, 1), np.int64)
    return np.where(k & 1, 1023 - lv[2], 1023 - lv[1])


def make(name, rows, cols, pitch, chroma, rng):
    """one plane of uint16 words, rows x pitch; the picture is its first `cols` word columns"""
    assert pitch >= cols and cols % 2 == 0 and name in CLASSES, (name, cols, pitch)
    s = np.concatenate([samples(name, rows, cols, chroma), outside(name, rows, pitch - cols, chroma)], axis=1)
    return ((s << 6) | rng.integers(0, 64, s.shape)).astype(np.uint16)


def frame(name, w, h, pitch_y=None, pitch_uv=None, seed=0):
    """(y, uv) of a P010 frame of w x h, pitches in words"""
    rng = np.random.default_rng(seed)
    return make(name, h, w, pitch_y or w, False, rng), make(name, h // 2, w, pitch_uv or w, True, rng)
