"""CPU: tsvpp_convert_mesh's host side and its coordinate model (tests/mesh_util.py) -- tsvpp_mesh_expand against the numpy restatement bit for bit, both against
a float64 interpolation within the bound derived from the six roundings, mesh_from_map / mesh_error, the ABI (symbols, struct sizes, every
status from tsvpp_describe_mesh without a context), the describe line, the Python argument forms and mesh_undistort."""
import ctypes
import os

import numpy as np
import pytest

import mesh_util as M
import remap_util as R
from warp_util import BGR24, BILINEAR, MERGED, PLANAR, RGB24, F32

OK, UNSUPPORTED, ERROR = 0, -2, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(64, 64), (70, 66), (30, 34)]
FRAME = (322, 182)
PF = ctypes.POINTER(ctypes.c_float)


@pytest.fixture(scope="module")
def native():
    from tensor_stream import _native
    _native.lib()
    return _native


def c_expand(native, mesh, dst, cell, pitch=0):
    out = np.full((dst[1], dst[0], 2), -77, F32)
    sts = native.lib().tsvpp_mesh_expand(mesh.ctypes.data_as(PF), pitch, dst[0], dst[1], M.log2(cell[0]), M.log2(cell[1]), out.ctypes.data_as(PF), 0)
    assert sts == OK
    return out


# ---- 1. the coordinate -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell", M.CELLS)
@pytest.mark.parametrize("dst", SIZES)
def test_expand_equals_the_restatement_bit_for_bit(native, dst, cell):
    """tsvpp_mesh_expand (the function the kernel calls) against mesh_util.expand on smooth meshes, the identity, the 2 : 1 mesh and seeded garbage with NaN, +-inf
    and subnormals; a NaN stands for any NaN"""
    w, h = FRAME
    meshes = dict(M.mesh_set(w, h, *dst, cell), identity=M.identity(*dst, cell), exact2=M.exact2(*dst, cell), garbage2=M.garbage(*dst, cell, 99))
    assert M.dims(*dst, cell) == (((dst[1] - 1) // cell[1]) + 2, ((dst[0] - 1) // cell[0]) + 2)
    for name, mesh in meshes.items():
        got, want = c_expand(native, mesh, dst, cell), M.expand(mesh, *dst, cell)
        assert M.same_bits(got, want), (name, dst, cell, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:4])
    g = M.expand(meshes["garbage"], *dst, cell)
    assert np.isnan(g).any() and (cell == (256, 256) or np.isfinite(g).any())  # (one cell of garbage is NaN throughout: its first two points are +inf and -inf)
    # at a control point f is the control value itself
    e = M.expand(meshes["barrel"], *dst, cell)
    rows, cols = M.dims(*dst, cell)
    inside = meshes["barrel"][:(dst[1] - 1) // cell[1] + 1, :(dst[0] - 1) // cell[0] + 1]
    assert np.array_equal(e[::cell[1], ::cell[0]].view(np.uint32), inside.view(np.uint32))
    # a padded pitch reads no padding
    view, back = M.padded(meshes["barrel"])
    assert M.same_bits(c_expand(native, back, dst, cell, pitch=back.strides[0]), e)


@pytest.mark.parametrize("cell", M.CELLS)
def test_identities_are_exact(native, cell):
    """the interpolation of the identity, the 2 : 1 and an even translation mesh is exact: E(mesh) is remap_util's dense map of the same name, bit for bit"""
    for dst in SIZES:
        assert np.array_equal(c_expand(native, M.identity(*dst, cell), dst, cell), R.identity(*dst))
        assert np.array_equal(c_expand(native, M.exact2(*dst, cell), dst, cell), R.exact_ratio(*dst, 2))
        assert np.array_equal(c_expand(native, M.translation(*dst, cell, 20, 6), dst, cell), R.translation(*dst, 20, 6))


@pytest.mark.parametrize("cell", M.CELLS)
@pytest.mark.parametrize("dst", SIZES)
def test_expand_within_the_derived_bound_of_float64(native, dst, cell):
    """for finite meshes E(mesh) lies within (12 u + 32 u^2) * max|control value of the cell| of the real-valued interpolation: six roundings, no tuning"""
    w, h = FRAME
    for name in ("barrel", "affine30", "far"):
        mesh = M.mesh_set(w, h, *dst, cell)[name]
        ref, big = M.expand64(mesh, *dst, cell)
        err = np.abs(c_expand(native, mesh, dst, cell).astype(np.float64) - ref)
        assert (err <= M.BOUND * big).all(), (name, dst, cell, float((err / big).max() / M.U))


@pytest.mark.parametrize("cell", M.CELLS)
@pytest.mark.parametrize("dst", SIZES)
def test_from_map_of_an_affine_map_gives_it_back(native, dst, cell):
    """an affine dense map whose entries are exact in float32 (dyadic coefficients): mesh_from_map samples it, extrapolates the last row and column exactly, and
    expand returns the map within the bound of the six roundings"""
    import tensor_stream as ts
    j, i = R.grid(*dst)
    xy = R.stack(F32(1.5) * j - F32(0.25) * i + F32(3.125), F32(0.375) * j + F32(1.25) * i - F32(7.5))
    mesh = ts.mesh_from_map(xy, cell)
    assert mesh.shape == M.dims(*dst, cell) + (2,) and mesh.dtype == np.float32
    J, I = M.positions(*dst, cell)
    assert np.array_equal(mesh, M.stack(1.5 * J - 0.25 * I + 3.125, 0.375 * J + 1.25 * I - 7.5))  # beyond the output too
    e = ts.mesh_expand(mesh, dst, cell)
    _, big = M.expand64(mesh, *dst, cell)
    assert (np.abs(e.astype(np.float64) - xy.astype(np.float64)) <= M.BOUND * big).all()
    assert ts.mesh_error(xy, mesh, cell) <= M.BOUND * float(big.max())


def test_mesh_error_shrinks_with_the_cell(native):
    """a bilinear interpolant's error is h^2 / 8 * max|f''| per axis: it falls with the cell, and by the factor 4 per halving once the cell is small"""
    import tensor_stream as ts
    w, h = FRAME
    xy = R.barrel(112, 112, w, h)
    errs = [ts.mesh_error(xy, ts.mesh_from_map(xy, (c, c)), (c, c)) for c in (64, 32, 16, 8, 4)]
    assert all(a > b for a, b in zip(errs, errs[1:])) and 3.5 < errs[-2] / errs[-1] < 4.5, errs
    # non-finite entries do not count
    bad = xy.copy()
    bad[5, 5] = np.nan, np.inf
    mesh = ts.mesh_from_map(xy, (16, 16))
    assert ts.mesh_error(bad, mesh, (16, 16)) == ts.mesh_error(xy, mesh, (16, 16))


def test_lds_need_is_the_dense_calls_on_the_expanded_mesh(native):
    import tensor_stream as ts
    w, h = FRAME
    for dst in ((112, 112), (70, 66)):
        for cell in ((16, 16), (4, 4)):
            mesh = M.barrel(*dst, cell, w, h)
            for luma_only in (False, True):
                assert ts.mesh_lds_hint(mesh, dst, cell, w, h, luma_only) == ts.remap_lds_hint(M.expand(mesh, *dst, cell), w, h, luma_only) > 0


# ---- 2. ABI and statuses ---------------------------------------------------------------------------------------------------------------------------------

def _params(native, dst=(64, 64), rt=BILINEAR, fcc=RGB24, planes=MERGED, norm=0, crop=(0, 0, 0, 0)):
    return native.Params(crop[0], crop[1], crop[2], crop[3], dst[0], dst[1], rt, fcc, planes, norm)


def _describe(native, p, frames, meshes, remaps, border=(-1, -1, -1), spec=None, n_frames=None, n_meshes=None, n=None, aligned=1):
    L = native.lib()
    buf = ctypes.create_string_buffer(512)
    fr = (native.NV12 * max(len(frames), 1))(*frames) if frames is not None else None
    ms = (native.Mesh * max(len(meshes), 1))(*meshes) if meshes is not None else None
    rs = (native.Remap * max(len(remaps), 1))(*remaps) if remaps is not None else None
    nf = len(frames) if n_frames is None else n_frames
    nm = len(meshes) if n_meshes is None else n_meshes
    nr = len(remaps) if n is None else n
    pp = ctypes.byref(p) if p is not None else None
    if spec is None:
        sts = L.tsvpp_describe_mesh(pp, nf, fr, nm, ms, nr, rs, border[0], border[1], border[2], aligned, buf, len(buf))
    else:
        sp = ctypes.byref(spec) if spec != "null" else None
        sts = L.tsvpp_describe_mesh_tensor(pp, sp, nf, fr, nm, ms, nr, rs, border[0], border[1], border[2], aligned, buf, len(buf))
    return sts, buf.value.decode()


def test_symbols_and_struct_sizes(native):
    assert ctypes.sizeof(native.Mesh) == 24 and native.TSVPP_MAX_MESHES == 32
    header = open(os.path.join(ROOT, "include", "tsvpp.h")).read()
    assert "#define TSVPP_MAX_MESHES 32" in header
    L = native.lib()
    for s in ("tsvpp_convert_mesh", "tsvpp_describe_mesh", "tsvpp_convert_mesh_tensor", "tsvpp_describe_mesh_tensor", "tsvpp_mesh_dims", "tsvpp_mesh_expand",
              "tsvpp_mesh_from_map", "tsvpp_mesh_error", "tsvpp_mesh_lds_need"):
        assert s in native.SYMBOLS
        getattr(L, s)
    cols, rows = ctypes.c_int(), ctypes.c_int()
    assert L.tsvpp_mesh_dims(70, 66, 4, 3, ctypes.byref(cols), ctypes.byref(rows)) == OK and (cols.value, rows.value) == (6, 10)
    assert L.tsvpp_mesh_dims(1920, 1080, 4, 4, ctypes.byref(cols), ctypes.byref(rows)) == OK and 8 * cols.value * rows.value == 66792  # "67 KB"
    assert L.tsvpp_mesh_dims(70, 66, 4, 3, None, ctypes.byref(rows)) == ERROR
    assert L.tsvpp_mesh_dims(71, 66, 4, 3, ctypes.byref(cols), ctypes.byref(rows)) == ERROR
    assert L.tsvpp_mesh_dims(70, 66, 1, 3, ctypes.byref(cols), ctypes.byref(rows)) == UNSUPPORTED
    assert L.tsvpp_mesh_dims(70, 66, 4, 9, ctypes.byref(cols), ctypes.byref(rows)) == UNSUPPORTED


def test_statuses_in_their_order_without_a_context(native):
    N = native
    fr = [N.NV12(None, None, 192, 192, 128, 72)]
    ms = [N.Mesh(None, 0, 4, 4, 0)]
    rs = [N.Remap(0, 0)]
    p = _params(N)
    assert _describe(N, p, fr, ms, rs)[0] == OK
    # TSVPP_ERROR
    assert _describe(N, None, fr, ms, rs)[0] == ERROR
    assert _describe(N, p, None, ms, rs, n_frames=1)[0] == ERROR
    assert _describe(N, p, fr, None, rs, n_meshes=1)[0] == ERROR
    assert _describe(N, p, fr, ms, None, n=1)[0] == ERROR
    assert N.lib().tsvpp_describe_mesh(ctypes.byref(p), 1, (N.NV12 * 1)(*fr), 1, (N.Mesh * 1)(*ms), 1, (N.Remap * 1)(*rs), -1, -1, -1, 1, None, 0) == ERROR
    for kw in (dict(n_frames=0), dict(n_meshes=0), dict(n=0)):
        assert _describe(N, p, fr, ms, rs, **kw)[0] == ERROR
    assert _describe(N, p, [N.NV12(None, None, 192, 192, 0, 72)], ms, rs)[0] == ERROR
    for bad in (N.Remap(1, 0), N.Remap(-1, 0), N.Remap(0, 1), N.Remap(0, -1)):
        assert _describe(N, p, fr, ms, [bad])[0] == ERROR
    assert _describe(N, _params(N, dst=(0, 64)), fr, ms, rs)[0] == ERROR
    assert _describe(N, _params(N, crop=(0, 0, 32, 32)), fr, ms, rs)[0] == ERROR
    for border in ((256, 128, 128), (-2, -2, -2), (-1, 128, 128), (0, 0, 300)):
        assert _describe(N, p, fr, ms, rs, border=border)[0] == ERROR, border
    # the pitch: 64 columns at cell 16 are 5 control points, 40 bytes
    assert _describe(N, p, fr, [N.Mesh(None, 40, 4, 4, 0)], rs)[0] == OK
    assert _describe(N, p, fr, [N.Mesh(None, 40 + 48, 4, 4, 4096)], rs)[0] == OK
    assert _describe(N, p, fr, [N.Mesh(None, 32, 4, 4, 0)], rs)[0] == ERROR
    assert _describe(N, p, fr, [N.Mesh(None, 44, 4, 4, 0)], rs)[0] == ERROR
    assert _describe(N, p, fr, [N.Mesh(None, -8, 4, 4, 0)], rs)[0] == ERROR
    assert _describe(N, p, fr, [N.Mesh(None, 0, 4, 4, -1)], rs)[0] == ERROR
    # ... and TSVPP_ERROR wins over TSVPP_UNSUPPORTED
    assert _describe(N, p, fr, [N.Mesh(None, 0, 1, 4, -1)], rs)[0] == ERROR
    assert _describe(N, _params(N, rt=2), fr, ms, rs, border=(256, 0, 0))[0] == ERROR
    # TSVPP_UNSUPPORTED
    for lw, lh in ((1, 4), (9, 4), (4, 1), (4, 9), (-1, 4), (4, 40)):
        assert _describe(N, p, fr, [N.Mesh(None, 0, lw, lh, 0)], rs)[0] == UNSUPPORTED, (lw, lh)
    for lw, lh in ((2, 2), (8, 8), (2, 8)):
        assert _describe(N, p, fr, [N.Mesh(None, 0, lw, lh, 0)], rs)[0] == OK
    for rt in (0, 2, 3):
        assert _describe(N, _params(N, rt=rt), fr, ms, rs)[0] == UNSUPPORTED
    assert _describe(N, _params(N, dst=(63, 64)), fr, ms, rs)[0] == UNSUPPORTED
    assert _describe(N, p, [N.NV12(None, None, 192, 192, 127, 72)], ms, rs)[0] == UNSUPPORTED
    assert _describe(N, _params(N, fcc=5), fr, ms, rs)[0] == UNSUPPORTED  # (a format outside the list)
    # the tensor form: the plan's status first, then the spec's
    spec = N.TensorSpec(1, (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1))
    pt = _params(N, fcc=BGR24, planes=PLANAR, norm=1)
    assert _describe(N, pt, fr, ms, rs, spec=spec)[0] == OK
    assert _describe(N, pt, fr, ms, rs, spec="null")[0] == ERROR
    assert _describe(N, pt, fr, [N.Mesh(None, 0, 9, 4, 0)], rs, spec="null")[0] == UNSUPPORTED
    assert _describe(N, _params(N, fcc=RGB24, planes=MERGED, norm=1), fr, ms, rs, spec=spec)[0] == UNSUPPORTED
    # the host-only functions refuse what they cannot read
    L = N.lib()
    a = np.zeros((80, 80, 2), F32)
    pa = a.ctypes.data_as(PF)
    assert L.tsvpp_mesh_expand(None, 0, 64, 64, 4, 4, pa, 0) == ERROR and L.tsvpp_mesh_expand(pa, 0, 64, 64, 4, 4, None, 0) == ERROR
    assert L.tsvpp_mesh_expand(pa, 36, 64, 64, 4, 4, pa, 0) == ERROR and L.tsvpp_mesh_expand(pa, 0, 64, 64, 4, 4, pa, 8 * 64 - 8) == ERROR
    assert L.tsvpp_mesh_expand(pa, 0, 64, 64, 4, 9, pa, 0) == UNSUPPORTED
    assert L.tsvpp_mesh_from_map(pa, 0, 64, 63, 4, 4, pa, 0) == ERROR and L.tsvpp_mesh_from_map(pa, 0, 64, 64, 1, 4, pa, 0) == UNSUPPORTED
    worst = ctypes.c_float()
    assert L.tsvpp_mesh_error(pa, 0, 64, 64, pa, 0, 4, 4, None) == ERROR and L.tsvpp_mesh_error(pa, 0, 64, 64, pa, 0, 4, 4, ctypes.byref(worst)) == OK
    assert L.tsvpp_mesh_lds_need(None, 0, 64, 64, 4, 4, 128, 72, 0) == ERROR and L.tsvpp_mesh_lds_need(pa, 0, 64, 64, 4, 4, 127, 72, 0) == ERROR
    assert L.tsvpp_mesh_lds_need(pa, 0, 64, 64, 4, 10, 128, 72, 0) == UNSUPPORTED


def test_describe_line(native, monkeypatch):
    import torch
    import tensor_stream as ts
    for k in ("TSVPP_LDS_KB", "TSVPP_FORCE_GATHER", "TSVPP_NT_STORES"):
        monkeypatch.delenv(k, raising=False)
    fp = ts.FrameParameters(width=70, height=66, resize_type=BILINEAR, pixel_format=BGR24, planes_pos=PLANAR, normalization=True)
    geo = [(128, 72, 192), (322, 182, 384)]
    d = ts.describe_mesh(fp, geo, [(0, 0), (0, 2048)], cell=[(16, 8), (32, 32)], remaps=[(k % 2, k % 2) for k in range(40)], border=(114, 128, 128))
    assert d["mode"] == "mesh_bilinear" and d["out"] == "f32_planar" and d["dst"] == "70x66"
    assert (d["remaps"], d["meshes"], d["cell"], d["frames"], d["launches"], d["limit"]) == (40, 2, "16x8", 2, 2, 32)
    assert d["kernel"] == "vpp_mesh<O_F32_PLANAR,vec,staged,border>" and "_kernel<" not in d["kernel"]  # (tests/dispatch_grid.py scrapes "vpp_..._kernel<" literals)
    assert d["lds"] == 40 * 1024 - 64 and d["grid"] == 9 * 32 and d["tiles"] == "3x3" and d["tail"] == 2 and d["border"] == "114,128,128"
    assert "staged" not in d
    e = ts.describe_remap(fp, geo, [(0, 0), (0, 2048)], remaps=[(k % 2, k % 2) for k in range(40)], border=(114, 128, 128))
    assert {k: v for k, v in d.items() if k not in ("mode", "meshes", "cell", "kernel")} == {k: v for k, v in e.items() if k not in ("mode", "maps", "kernel")}
    assert d["kernel"].replace("vpp_mesh", "vpp_remap") == e["kernel"]
    h = ts.describe_mesh(fp, geo, [(0, 2048)], cell=(16, 16), remaps=[(0, 0)], aligned_outputs=False)
    assert h["kernel"] == "vpp_mesh<O_F32_PLANAR,elem,staged,replicate>" and h["lds"] == 2048 and h["tail"] == 0
    t = ts.describe_mesh(fp, geo, [(0, 0)], cell=(4, 256), remaps=[(1, 0)], dtype=torch.float16, mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25))
    assert t["kernel"] == "vpp_mesh_tensor<PLANAR,EL_HALF,vec,staged,replicate>" and t["out"] == "f16_planar" and t["cell"] == "4x256"
    monkeypatch.setenv("TSVPP_LDS_KB", "0")
    assert ts.describe_mesh(fp, geo, [(0, 0)], cell=(16, 16), remaps=[(0, 0)])["kernel"] == "vpp_mesh<O_F32_PLANAR,vec,gather,replicate>"


def test_python_argument_forms_raise_before_the_c_call(native):
    import torch
    import tensor_stream as ts
    fp = ts.FrameParameters(width=64, height=64, resize_type=BILINEAR, pixel_format=RGB24, planes_pos=MERGED, normalization=False)
    geo = [(128, 72, 192)]
    good = torch.zeros((5, 5, 2), dtype=torch.float32)
    assert ts.describe_mesh(fp, geo, good, cell=(16, 16))["meshes"] == 1
    assert ts.describe_mesh(fp, geo, (good, 1024), cell=(16, 16))["lds"] == 1024
    wide = torch.zeros((5, 8, 2), dtype=torch.float32)[:, :5]
    assert ts.describe_mesh(fp, geo, wide, cell=(16, 16))["meshes"] == 1
    for bad in (good.double(), torch.zeros((5, 6, 2)), torch.zeros((5, 5)), torch.zeros((5, 2, 5)).permute(0, 2, 1), torch.zeros((5, 5, 4))[:, :, ::2]):
        with pytest.raises(ValueError):
            ts.describe_mesh(fp, geo, bad, cell=(16, 16))
    for cell in ((12, 16), (16, 0), (16,), 16, (16, -4), [(16, 16), (8, 8)]):
        with pytest.raises(ValueError):
            ts.describe_mesh(fp, geo, good, cell=cell)
    with pytest.raises(ValueError):
        ts.describe_mesh(fp, geo, [], cell=(16, 16))
    with pytest.raises(ValueError):
        ts.describe_mesh(fp, geo * 3, [good, good], cell=(16, 16))  # three frames and two meshes do not pair up
    with pytest.raises(RuntimeError, match="-2"):
        ts.describe_mesh(fp, geo, [(0, 0)], cell=(512, 16))  # a power of two the C call refuses
    with pytest.raises(ValueError):
        ts.mesh_expand(np.zeros((5, 6, 2), F32), (64, 64), (16, 16))
    with pytest.raises(ValueError):
        ts.mesh_from_map(np.zeros((64, 64, 2), np.float64), (16, 16))
    with pytest.raises(ValueError):
        ts.mesh_error(np.zeros((64, 64, 2), F32), np.zeros((4, 5, 2), F32), (16, 16))
    with pytest.raises(ValueError):
        ts.mesh_lds_hint(np.zeros((5, 5, 2), F32), (64, 64), (8, 8), 128, 72)
    assert ts.mesh_dims(70, 66, (16, 8)) == (10, 6)
    # tensors give tensors, arrays give arrays
    assert isinstance(ts.mesh_expand(good, (64, 64), (16, 16)), torch.Tensor) and isinstance(ts.mesh_from_map(np.zeros((64, 64, 2), F32), (16, 16)), np.ndarray)


def test_mesh_undistort(native):
    """zero distortion with K = new_K is exactly the identity mesh; with distortion it is OpenCV's forward model at the control positions (a float64 evaluation
    written the textbook way agrees to rounding); a new_K that zooms scales the mesh"""
    import tensor_stream as ts
    K = np.array([[811.3, 0, 963.137], [0, 808.9, 541.77], [0, 0, 1]])
    for cell in ((16, 16), (32, 8), (256, 4)):
        m = ts.mesh_undistort(K, (0, 0, 0, 0), K, (1920, 1080), cell)
        assert m.dtype == np.float32 and np.array_equal(m.view(np.uint32), M.identity(1920, 1080, cell).view(np.uint32)), cell
    dist = (-0.28, 0.07, 0.001, -0.002, 0.01, 0.02, -0.01, 0.003)
    newK = np.array([[700.0, 0, 320.0], [0, 710.0, 320.0], [0, 0, 1]])
    cell = (16, 16)
    for nd in (4, 5, 8):
        d = dist[:nd]
        m = ts.mesh_undistort(K, d, newK, (640, 640), cell)
        k1, k2, p1, p2, k3, k4, k5, k6 = tuple(d) + (0.0,) * (8 - nd)
        J, I = M.positions(640, 640, cell)
        x, y = (J - 320.0) / 700.0, (I - 320.0) / 710.0
        r2 = x * x + y * y
        rad = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
        xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        ref = np.stack((K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]), -1)
        assert m.shape == ref.shape and np.abs(m - ref).max() <= 2 ** -23 * np.abs(ref).max()  # one float32 rounding (2^-24) and float64 noise
    with pytest.raises(ValueError):
        ts.mesh_undistort(K, (0.1, 0.2, 0.3), K, (640, 640), cell)
    with pytest.raises(ValueError):
        ts.mesh_undistort(K[:2], (0, 0, 0, 0), K, (640, 640), cell)
