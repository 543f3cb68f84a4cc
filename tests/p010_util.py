"""Shared by the P010 letterbox tests: a numpy restatement of the contract of tsvpp_convert_letterbox_p010 (include/tsvpp.h) and nothing else.  float32
operations in the stated order, the fused steps through warp_util.fma32, integers elsewhere, the quotient as np.float32(np.float64(k) / 1023).  Contains no
product code; the reference has no 10-bit path, so this model IS the expected value."""
import numpy as np

from warp_util import fma32

NEAREST, BILINEAR = 0, 1
Y800, RGB24, BGR24 = 0, 1, 2
PLANAR, MERGED = 0, 1
F32 = np.float32
# tsvpp_default_coeffs: y_scale, v_to_r, u_to_b, v_to_g, u_to_g, round_bias, y_offset, c_offset
COEFFS = tuple(F32(v) for v in (1.163999557, 1.5959997177, 2.017999649, -0.812999725, -0.390999794, 0.5, 16.0, 128.0))


def samples(words):
    """s = word >> 6"""
    return (np.asarray(words).view(np.uint16) >> 6).astype(np.int64)


def _axis(idx, ratio, limit, taps, mode):
    """first tap, second tap, weight of output indices idx along one axis: `limit` is what the coordinate clamps to, `taps` the samples of the plane's axis"""
    idx = np.asarray(idx)
    if mode == NEAREST:
        p = (ratio * idx.astype(F32)).astype(np.int64)
        return p, p, np.zeros(idx.shape, F32)
    f = fma32(idx.astype(F32) + F32(0.5), ratio, F32(-0.5))
    pf = np.floor(f)
    w = (f - pf).astype(F32)
    p = pf.astype(np.int64)
    edge = (p < 0) | (p > limit - 1)
    p = np.clip(p, 0, limit - 1)
    w = np.where(edge, F32(0), w).astype(F32)
    return p, np.where(p + 1 >= taps, p, p + 1), w


def _blend(A, B, C, D, wx, wy):
    A, B, C, D = (t.astype(F32) for t in (A, B, C, D))
    omx, omy = F32(1) - wx, F32(1) - wy
    s = fma32(A * omx, omy, (B * wx) * omy)
    s = fma32(C * wy, omx, s)
    s = fma32(D, wx * wy, s)
    return s.astype(np.int64)  # truncated toward zero (s >= 0)


def resize(S, rows, cols, xr, yr, w, h, taps_x, taps_y, mode):
    """plane S (samples) at output indices rows x cols; the coordinate clamps are to the LUMA size (w, h) for both planes, as in the 8-bit call"""
    y, y2, wy = _axis(rows, yr, h, taps_y, mode)
    x, x2, wx = _axis(cols, xr, w, taps_x, mode)
    if mode == NEAREST:
        return S[np.ix_(y, x)]
    return _blend(S[np.ix_(y, x)], S[np.ix_(y, x2)], S[np.ix_(y2, x)], S[np.ix_(y2, x2)], wx[None, :], wy[:, None])


def virtual_frame(y, uv, w, h, rect, canvas, mode, pad):
    """the canvas before the colour stage: Y (ch, cw), U and V (ch / 2, cw / 2) as samples 0..1023.  y, uv: uint16 planes of any pitch (in words)"""
    cw, ch = canvas
    left, top, iw, ih = rect
    Ys, UVs = samples(y)[:h, :w], samples(uv)[:h // 2, :w]
    xr, yr = F32(w) / F32(iw), F32(h) / F32(ih)
    Y = np.full((ch, cw), pad[0], np.int64)
    U = np.full((ch // 2, cw // 2), pad[1], np.int64)
    V = np.full((ch // 2, cw // 2), pad[2], np.int64)
    Y[top:top + ih, left:left + iw] = resize(Ys, np.arange(ih), np.arange(iw), xr, yr, w, h, w, h, mode)
    for P, S in ((U, UVs[:, 0::2]), (V, UVs[:, 1::2])):
        P[top // 2:(top + ih) // 2, left // 2:(left + iw) // 2] = resize(S, np.arange(ih // 2), np.arange(iw // 2), xr, yr, w, h, w // 2, h // 2, mode)
    return Y, U, V


def channels(Y, U, V, fcc, g_term=0, k=COEFFS):
    """k per stored channel, (c, ch, cw) integers 0..1023"""
    if fcc == Y800:
        return Y[None]
    y_scale, v_to_r, u_to_b, v_to_g, u_to_g, bias, y_off, c_off = k
    u = np.repeat(np.repeat(U, 2, 0), 2, 1).astype(F32) - F32(4) * c_off
    v = np.repeat(np.repeat(V, 2, 0), 2, 1).astype(F32) - F32(4) * c_off
    yv = np.maximum(F32(0), Y.astype(F32) - F32(4) * y_off) * y_scale
    rv, bv = fma32(v, v_to_r, bias), fma32(u, u_to_b, bias)
    if g_term == 0:
        g = fma32(v, v_to_g, u * u_to_g)
    elif g_term == 1:
        g = v * v_to_g + u * u_to_g
    else:
        g = fma32(u, u_to_g, v * v_to_g)
    gv = g + bias
    out = [np.clip(np.trunc(yv + t), 0, 1023).astype(np.int64) for t in (rv, gv, bv)]
    return np.stack(out if fcc == RGB24 else out[::-1])


def quotient(k):
    return (k.astype(np.float64) / 1023).astype(F32)


def stored(k, planes, norm):
    """the plain flavours: k (c, ch, cw) -> raw bytes of the output"""
    v = quotient(k) if norm else np.minimum(255, (k + 2) >> 2).astype(np.uint8)
    if planes == MERGED and k.shape[0] == 3:
        v = v.transpose(1, 2, 0)
    return np.ascontiguousarray(v).ravel().view(np.uint8)


def expected(y, uv, w, h, rect, canvas, mode, fcc, planes, norm, pad, g_term=0):
    return stored(channels(*virtual_frame(y, uv, w, h, rect, canvas, mode, pad), fcc, g_term), planes, norm)
