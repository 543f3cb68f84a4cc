"""Shared by the mesh tests (tsvpp_convert_mesh): a numpy restatement of the coordinate contract of include/tsvpp.h -- expand(), the dense map E(mesh) -- and
generators for the meshes the tests use.  From E(mesh) on the contract is the dense call's, so the expected output is tests/remap_util.py's of E(mesh).  All
arithmetic is np.float32, one rounding per operation; the fused multiply-adds are warp_util.fma32.  Contains no product code."""
import numpy as np

from warp_util import F32, fma32

U = 2.0 ** -24  # the unit roundoff of float32
# |E(mesh) - the real-valued bilinear interpolation| <= BOUND * max|control value of the cell| (DESIGN.md section 5 derives it from the six roundings)
BOUND = 12 * U + 32 * U * U

CELLS = [(4, 4), (16, 8), (8, 32), (256, 256)]


def log2(v):
    assert v > 0 and v & (v - 1) == 0
    return v.bit_length() - 1


def dims(dst_w, dst_h, cell):
    """(rows, cols) of the control grid"""
    return ((dst_h - 1) >> log2(cell[1])) + 2, ((dst_w - 1) >> log2(cell[0])) + 2


def fma(a, b, c):
    """fma32 for every bit pattern: where the exact a * b + c is no number (an operand is inf or NaN; finite float32 operands cannot overflow float64) the float64
    expression already is what IEEE-754 says -- the infinity or a NaN -- and fma32, which is stated on numbers, is not asked"""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    with np.errstate(invalid="ignore", over="ignore"):
        naive = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
        ok = np.isfinite(naive)
        zero = F32(0)
        r = fma32(np.where(ok, a, zero), np.where(ok, b, zero), np.where(ok, c, zero))
        return np.where(ok, r, naive.astype(F32)).astype(F32)


def expand(mesh, dst_w, dst_h, cell):
    """E(mesh): (dst_h, dst_w, 2) float32 from the control grid (rows, cols, 2) -- per component top = fma(tx, B - A, A), bot = fma(tx, D - C, C),
    f = fma(ty, bot - top, top) with tx = (j mod cw) / cw, ty = (i mod ch) / ch"""
    mesh = np.asarray(mesh, F32)
    cw, ch = cell
    assert mesh.shape == dims(dst_w, dst_h, cell) + (2,), (mesh.shape, dims(dst_w, dst_h, cell))
    j, i = np.arange(dst_w), np.arange(dst_h)
    c, r = (j >> log2(cw))[None, :], (i >> log2(ch))[:, None]
    tx = ((j & (cw - 1)).astype(F32) * F32(1.0 / cw))[None, :, None]
    ty = ((i & (ch - 1)).astype(F32) * F32(1.0 / ch))[:, None, None]
    A, B, C, D = mesh[r, c], mesh[r, c + 1], mesh[r + 1, c], mesh[r + 1, c + 1]
    with np.errstate(invalid="ignore", over="ignore"):
        top = fma(tx, (B - A).astype(F32), A)
        bot = fma(tx, (D - C).astype(F32), C)
        return np.ascontiguousarray(fma(ty, (bot - top).astype(F32), top))


def expand64(mesh, dst_w, dst_h, cell):
    """the real-valued bilinear interpolation of the control points in float64, and max |control value| of each pixel's cell: (value (dst_h, dst_w, 2), M)"""
    m = np.asarray(mesh, np.float64)
    cw, ch = cell
    j, i = np.arange(dst_w), np.arange(dst_h)
    c, r = (j >> log2(cw))[None, :], (i >> log2(ch))[:, None]
    tx, ty = ((j & (cw - 1)) / cw)[None, :, None], ((i & (ch - 1)) / ch)[:, None, None]
    A, B, C, D = m[r, c], m[r, c + 1], m[r + 1, c], m[r + 1, c + 1]
    top, bot = A + tx * (B - A), C + tx * (D - C)
    return top + ty * (bot - top), np.max(np.abs(np.stack((A, B, C, D))), axis=0)


def same_bits(a, b):
    """equal as bit patterns, a NaN standing for any NaN (its payload is no part of the contract: every NaN counts as -1)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


# ---- the mesh set ------------------------------------------------------------------------------------------------------------------------------------------

def positions(dst_w, dst_h, cell):
    """the output indices (J, I) of the control points, float64 (rows, cols): the last row and column may lie beyond the output"""
    rows, cols = dims(dst_w, dst_h, cell)
    return np.meshgrid(np.arange(cols, dtype=np.float64) * cell[0], np.arange(rows, dtype=np.float64) * cell[1])


def stack(x, y):
    return np.ascontiguousarray(np.stack((np.asarray(x, F32), np.asarray(y, F32)), axis=-1))


def identity(dst_w, dst_h, cell):
    return stack(*positions(dst_w, dst_h, cell))


def exact2(dst_w, dst_h, cell):
    """x = 2 j + 0.5, y = 2 i + 0.5: the BILINEAR coordinates of the exact ratio 2 : 1"""
    J, I = positions(dst_w, dst_h, cell)
    return stack(2 * J + 0.5, 2 * I + 0.5)


def translation(dst_w, dst_h, cell, dx, dy):
    J, I = positions(dst_w, dst_h, cell)
    return stack(J + dx, I + dy)


def affine(dst_w, dst_h, cell, w, h, degrees=30.0, scale=1.7):
    """remap_util.affine at the control positions: the output rotated about the frame's centre at `scale` source pixels per output pixel"""
    J, I = positions(dst_w, dst_h, cell)
    c, s = np.cos(np.radians(degrees)) * scale, np.sin(np.radians(degrees)) * scale
    u, v = J - (dst_w - 1) / 2, I - (dst_h - 1) / 2
    return stack(c * u - s * v + (w - 1) / 2, s * u + c * v + (h - 1) / 2)


def barrel(dst_w, dst_h, cell, w, h, k1=-0.28, k2=0.07):
    """remap_util.barrel at the control positions"""
    J, I = positions(dst_w, dst_h, cell)
    u, v = (J + 0.5) / dst_w * 2 - 1, (I + 0.5) / dst_h * 2 - 1
    r2 = (u * u + v * v) / 2
    f = 1 + k1 * r2 + k2 * r2 * r2
    return stack((u * f + 1) * w / 2 - 0.5, (v * f + 1) * h / 2 - 0.5)


def far(dst_w, dst_h, cell):
    J, I = positions(dst_w, dst_h, cell)
    return stack(J + 5000, I - 3000)


def garbage(dst_w, dst_h, cell, seed):
    """random bit patterns as control points: NaNs, infinities of both signs and subnormals are planted; the first cell holds +inf and -inf, whose difference is
    the NaN the contract counts as -1"""
    rows, cols = dims(dst_w, dst_h, cell)
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 1 << 32, (rows, cols, 2), dtype=np.uint64).astype(np.uint32)
    flat = bits.reshape(-1)
    special = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x7F800001, 0x80000000], np.uint32)
    where = rng.choice(flat.size, size=max(flat.size // 4, 1), replace=False)
    flat[where] = np.resize(special, where.size)
    bits[0, 0, 0], bits[0, 1, 0] = 0x7F800000, 0xFF800000
    return np.ascontiguousarray(bits.view(F32))


def padded(mesh, extra=6):
    """the same mesh with a row stride of 2 * cols + extra floats and NaN in the padding: (the strided view, its backing array)"""
    rows, cols, _ = mesh.shape
    back = np.full((rows, 2 * cols + extra), np.nan, F32)
    view = back[:, :2 * cols].reshape(rows, cols, 2)
    view[...] = mesh
    return view, back


def mesh_set(w, h, dst_w, dst_h, cell, seed=0):
    """name -> mesh for a w x h frame: the set of the GPU test"""
    return {"barrel": barrel(dst_w, dst_h, cell, w, h), "affine30": affine(dst_w, dst_h, cell, w, h), "far": far(dst_w, dst_h, cell),
            "garbage": garbage(dst_w, dst_h, cell, seed + 7 * w + dst_w + cell[0])}
