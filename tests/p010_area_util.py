"""Shared by the tests of tsvpp_convert_letterbox_p010_area: a numpy restatement, in int64, of the resize that call's contract states (include/tsvpp.h) -- an exact
box filter per plane: row means in 1/64 sample steps, then column means -- in the place of p010_util.resize; the colour stage and the stored forms are
p010_util's, unchanged.  Contains no product code; the reference has no 10-bit path, so this model IS the expected value."""
import numpy as np

import p010_util as M

AREA = 3


def axis(N, n):
    """taps and weights of the n outputs of an axis of N samples: (n, T) index and weight arrays, weight 0 where an output has fewer than T taps"""
    j = np.arange(n, dtype=np.int64)
    first, last = j * N // n, ((j + 1) * N - 1) // n
    i = first[:, None] + np.arange((last - first).max() + 1)[None, :]
    o = np.minimum((i + 1) * n, ((j + 1) * N)[:, None]) - np.maximum(i * n, (j * N)[:, None])
    return np.minimum(i, N - 1), np.maximum(o, 0)


def box(S, w, h, exact=False):
    """plane S (H, W) of samples -> (h, w): the contract's two passes; `exact`: the rational mean in float64 instead"""
    H, W = S.shape
    S = S.astype(np.float64 if exact else np.int64)
    ix, ox = axis(W, w)
    hx = sum(S[:, ix[:, t]] * ox[:, t] for t in range(ix.shape[1]))
    r = hx / W if exact else (64 * hx + W // 2) // W
    iy, oy = axis(H, h)
    v = sum(r[iy[:, t]] * oy[:, t, None] for t in range(iy.shape[1]))
    return v / H if exact else (v + 32 * H) // (64 * H)


def virtual_frame(y, uv, w, h, rect, canvas, pad):
    """p010_util.virtual_frame with the box filter: the canvas before the colour stage"""
    cw, ch = canvas
    left, top, iw, ih = rect
    Ys, UVs = M.samples(y)[:h, :w], M.samples(uv)[:h // 2, :w]
    Y = np.full((ch, cw), pad[0], np.int64)
    U = np.full((ch // 2, cw // 2), pad[1], np.int64)
    V = np.full((ch // 2, cw // 2), pad[2], np.int64)
    Y[top:top + ih, left:left + iw] = box(Ys, iw, ih)
    for P, S in ((U, UVs[:, 0::2]), (V, UVs[:, 1::2])):
        P[top // 2:(top + ih) // 2, left // 2:(left + iw) // 2] = box(S, iw // 2, ih // 2)
    return Y, U, V


def want(fr, size, rect, canvas, flavour, pad):
    """the raw bytes of one canvas in a flavour of p010_cases.FLAVOURS"""
    import p010_cases as C
    return C.stored(M.channels(*virtual_frame(fr[0], fr[1], *size, rect, canvas, pad), C.FLAVOURS[flavour][0]), flavour)
