"""Shared by the remap tests (tsvpp_convert_remap): a numpy restatement of the contract of include/tsvpp.h that makes the VIRTUAL NV12 frame of dst_w x dst_h -- the
samples before the colour back end -- and the expected output, which is the existing oracle's conversion without a resize of that virtual frame; and generators
for the map set the tests use.  From the clamped coordinate on everything is tests/warp_util.py's (axis, bilerp, outside); the chroma coordinate's fused
multiply-add is its fma32.  All arithmetic is np.float32, one rounding per operation.  Contains no product code.
Its judge is tests/sampler64.py: an independent float64 evaluation of the header's prose, whose bracket this model must stay inside (tests/test_sampler64_cpu.py)."""
import numpy as np

from warp_util import F32, axis, bilerp, fma32, outside

TILE = 32  # ROI_TILE_W = ROI_TILE_H

# (frame (width, height, pitch), dst, names out of map_set): what the GPU test sends through contexts of TSVPP_LDS_KB = default / 0 / 3 -- under the default budget
# every tile stages, under 3 KiB the translation, the constant and the far map do and the 30 degree warp and the barrel do not (tests/test_remap_cpu.py proves it
# from the footprints)
STAGING_CASE = ((322, 182, 384), (112, 112), ("barrel", "affine30", "translate", "constant", "far"))


def clamp(f, limit):
    """THE clamp: fmax first, so a NaN counts as -1"""
    return np.fmin(np.fmax(np.asarray(f, F32), F32(-1)), F32(limit)).astype(F32)


def chroma_coord(c):
    """one component (dst_h, dst_w) of a map -> the pair grid's (dst_h / 2, dst_w / 2): three additions in the contract's order, then one fma"""
    c = np.asarray(c, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        s = ((c[0::2, 0::2] + c[0::2, 1::2]) + (c[1::2, 0::2] + c[1::2, 1::2])).astype(F32)
        finite = np.isfinite(s)  # (fma32 is stated on numbers: an infinite or NaN sum stays what it is through the fma)
        return np.where(finite, fma32(np.where(finite, s, F32(0)), F32(0.125), F32(-0.25)), s).astype(F32)


def coords(xy, w, h):
    """the clamped coordinates of a map (dst_h, dst_w, 2) on a w x h frame: luma x, y (dst_h, dst_w) and chroma x, y (dst_h / 2, dst_w / 2)"""
    xy = np.asarray(xy, F32)
    return clamp(xy[..., 0], w), clamp(xy[..., 1], h), clamp(chroma_coord(xy[..., 0]), w // 2), clamp(chroma_coord(xy[..., 1]), h // 2)


def virtual_frame_from_map(y, uv, w, h, xy, border=None):
    """the dst_w x dst_h NV12 frame the map samples out of the w x h frame (y, uv: planes with any pitch) -> (Y (dst_h, dst_w), UV (dst_h / 2, dst_w)) uint8"""
    fx, fy, cfx, cfy = coords(xy, w, h)
    x, x2, wx, _ = axis(fx, w)
    yy, y2, wy, _ = axis(fy, h)
    Y = bilerp(y[yy, x], y[yy, x2], y[y2, x], y[y2, x2], wx, wy)
    if border is not None:
        Y = np.where(outside(fx, w) | outside(fy, h), border[0], Y)
    cw, ch = w // 2, h // 2
    x, x2, wx, _ = axis(cfx, cw)
    yy, y2, wy, _ = axis(cfy, ch)
    UV = np.empty((xy.shape[0] // 2, xy.shape[1]), np.uint8)
    for comp in (0, 1):
        c = bilerp(uv[yy, 2 * x + comp], uv[yy, 2 * x2 + comp], uv[y2, 2 * x + comp], uv[y2, 2 * x2 + comp], wx, wy)
        if border is not None:
            c = np.where(outside(cfx, cw) | outside(cfy, ch), border[1 + comp], c)
        UV[:, comp::2] = c
    return Y.astype(np.uint8), UV


def expected(oracle, y, uv, w, h, xy, fcc, planes, norm, border=None, virtual=None):
    """the output as raw bytes: the oracle's conversion without a resize of the virtual frame (`virtual`: that frame, if the caller has it already)"""
    Y, UV = virtual_frame_from_map(y, uv, w, h, xy, border) if virtual is None else virtual
    ref, _, _ = oracle.convert(Y, UV, fourcc=fcc, planes=planes, normalization=norm)
    return ref.ravel().view(np.uint8)


def expected_planar_f32(oracle, virtual, fcc):
    """the oracle's fp32 PLANAR result of a virtual frame: what tests/tensor_util.py's expected() starts from"""
    ref, _, _ = oracle.convert(virtual[0], virtual[1], fourcc=fcc, planes=0, normalization=True)
    return ref


def tap_boxes(xy, w, h, j0, j1, i0, i1):
    """(xlo, xhi, ylo, yhi, cxlo, cxhi, cylo, cyhi): the extremes of every tap that can reach the result of output columns [j0, j1] / rows [i0, i1] -- the first
    tap always, the second unless its weight was forced to zero at the low edge (it is multiplied by that zero)"""
    fx, fy, cfx, cfy = coords(xy, w, h)
    out = []
    for f, limit, rows, cols in ((fx, w, slice(i0, i1 + 1), slice(j0, j1 + 1)), (fy, h, slice(i0, i1 + 1), slice(j0, j1 + 1)),
                                 (cfx, w // 2, slice(i0 >> 1, (i1 >> 1) + 1), slice(j0 >> 1, (j1 >> 1) + 1)),
                                 (cfy, h // 2, slice(i0 >> 1, (i1 >> 1) + 1), slice(j0 >> 1, (j1 >> 1) + 1))):
        p, p2, _, low = axis(f[rows, cols], limit)
        p2 = np.where(low, p, p2)
        out += [int(min(p.min(), p2.min())), int(max(p.max(), p2.max()))]
    return tuple(out)


def tiles(dst_w, dst_h, vec):
    """(j_first, j_last, i_first, i_last) of every tile of an output: the plain tiling, or -- `vec`, 4 k + 2 >= 32 columns -- with the last tile column shifted to
    the right edge"""
    cols = [(j, min(j + TILE, dst_w) - 1) for j in range(0, dst_w, TILE)]
    if vec and dst_w % 4 and dst_w >= TILE:
        cols[-1] = (dst_w - TILE, dst_w - 1)
    return [(j0, j1, i, min(i + TILE, dst_h) - 1) for i in range(0, dst_h, TILE) for (j0, j1) in cols]


def chunks(span):
    return ((span + 14) >> 4) + 1


def lds_need(box, luma_only=False):
    """roi_lds_need restated: 16-byte chunks of the luma rows, then of the chroma rows"""
    xlo, xhi, ylo, yhi, cxlo, cxhi, cylo, cyhi = box
    return 16 * ((yhi - ylo + 1) * chunks(xhi - xlo + 1) + (0 if luma_only else (cyhi - cylo + 1) * chunks(2 * (cxhi - cxlo + 1))))


def stageable(box):
    return chunks(box[1] - box[0] + 1) <= 128 and chunks(2 * (box[5] - box[4] + 1)) <= 128


# ---- the map set ---------------------------------------------------------------------------------------------------------------------------------------

def grid(dst_w, dst_h):
    """(j, i) as float32 arrays (dst_h, dst_w)"""
    j, i = np.meshgrid(np.arange(dst_w, dtype=F32), np.arange(dst_h, dtype=F32))
    return j, i


def stack(x, y):
    return np.ascontiguousarray(np.stack((np.asarray(x, F32), np.asarray(y, F32)), axis=-1))


def identity(dst_w, dst_h):
    return stack(*grid(dst_w, dst_h))


def exact_ratio(dst_w, dst_h, r):
    """the BILINEAR coordinates of the exact power-of-two ratio r: (j + 0.5) r - 0.5, exact in float32"""
    j, i = grid(dst_w, dst_h)
    return stack(j * F32(r) + F32(0.5 * r - 0.5), i * F32(r) + F32(0.5 * r - 0.5))


def translation(dst_w, dst_h, dx, dy):
    j, i = grid(dst_w, dst_h)
    return stack(j + F32(dx), i + F32(dy))


def affine(dst_w, dst_h, w, h, degrees=30.0, scale=1.7):
    """the output rotated by `degrees` about the frame's centre at `scale` source pixels per output pixel, in float64, rounded once"""
    j, i = np.meshgrid(np.arange(dst_w, dtype=np.float64), np.arange(dst_h, dtype=np.float64))
    c, s = np.cos(np.radians(degrees)) * scale, np.sin(np.radians(degrees)) * scale
    u, v = j - (dst_w - 1) / 2, i - (dst_h - 1) / 2
    return stack(c * u - s * v + (w - 1) / 2, s * u + c * v + (h - 1) / 2)


def barrel(dst_w, dst_h, w, h, k1=-0.28, k2=0.07):
    """r' = r (1 + k1 r^2 + k2 r^4) about the centre, r normalised to the half diagonal; the output spans the frame"""
    j, i = np.meshgrid(np.arange(dst_w, dtype=np.float64), np.arange(dst_h, dtype=np.float64))
    u, v = (j + 0.5) / dst_w * 2 - 1, (i + 0.5) / dst_h * 2 - 1
    r2 = (u * u + v * v) / 2
    f = 1 + k1 * r2 + k2 * r2 * r2
    return stack((u * f + 1) * w / 2 - 0.5, (v * f + 1) * h / 2 - 0.5)


def transpose(dst_w, dst_h):
    j, i = grid(dst_w, dst_h)
    return stack(i, j)


def constant(dst_w, dst_h, x, y):
    return stack(np.full((dst_h, dst_w), x, F32), np.full((dst_h, dst_w), y, F32))


def split(dst_w, dst_h, w, h):
    """the left half of the output to the frame's top-left corner, the right half to its bottom-right: a tile's footprint is the whole frame"""
    j, i = grid(dst_w, dst_h)
    left = j < dst_w // 2
    return stack(np.where(left, F32(0.25), F32(w - 1.25)), np.where(left, F32(0.5), F32(h - 1.5)))


def far(dst_w, dst_h):
    j, i = grid(dst_w, dst_h)
    return stack(j + F32(5000), i - F32(3000))


def garbage(dst_w, dst_h, seed):
    """random bit patterns: NaNs, infinities of both signs and subnormals are planted, the rest is whatever 32 random bits are"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 1 << 32, (dst_h, dst_w, 2), dtype=np.uint64).astype(np.uint32)
    flat = bits.reshape(-1)
    special = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x7F800001, 0x80000000], np.uint32)
    where = rng.choice(flat.size, size=min(flat.size // 4, 8 * special.size), replace=False)
    flat[where] = np.resize(special, where.size)
    # an entry block whose x entries are +inf and -inf: their sum is the NaN the contract counts as -1
    bits[0, 0, 0], bits[0, 1, 0] = 0x7F800000, 0xFF800000
    return np.ascontiguousarray(bits.view(F32))


def padded(xy, extra=6):
    """the same map with a row stride of 2 * dst_w + extra floats and NaN in the padding: (the strided view, its backing array)"""
    dst_h, dst_w, _ = xy.shape
    back = np.full((dst_h, 2 * dst_w + extra), np.nan, F32)
    view = back[:, :2 * dst_w].reshape(dst_h, dst_w, 2)
    view[...] = xy
    return view, back


def map_set(w, h, dst_w, dst_h, seed=0):
    """name -> map (dst_h, dst_w, 2) float32 for a w x h frame: the set of the issue (the pitch-padded form is padded() of any of them)"""
    out = {}
    if (dst_w, dst_h) == (w, h):
        out["identity"] = identity(dst_w, dst_h)
    if 2 * dst_w <= w and 2 * dst_h <= h:
        out["exact2"] = exact_ratio(dst_w, dst_h, 2)
    dx, dy = 2 * max((w - dst_w) // 4, 0), 2 * max((h - dst_h) // 4, 0)
    out["translate"] = translation(dst_w, dst_h, dx, dy)
    out["affine30"] = affine(dst_w, dst_h, w, h)
    out["barrel"] = barrel(dst_w, dst_h, w, h)
    out["transpose"] = transpose(dst_w, dst_h)
    out["constant"] = constant(dst_w, dst_h, w / 3 + 0.3, h / 3 + 0.7)
    out["split"] = split(dst_w, dst_h, w, h)
    out["far"] = far(dst_w, dst_h)
    out["garbage"] = garbage(dst_w, dst_h, seed + 7 * w + dst_w)
    return out
