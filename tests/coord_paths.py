"""The four coordinate paths as tests/coord_suite.py's descriptors -- WARP, PERSP, REMAP, MESH -- with the item sets and requests their GPU tests use.
Warp and perspective send rows of coefficients, [(frame, m)], in the kernel arguments; remap and mesh send device tables and (frame, table) pairs, a
cs.Tables.  The adaptors here hide that from the shared cases."""
import ctypes
import math

import numpy as np
import pytest
import torch

import coord_suite as cs
import mesh_util as M
import persp_util as P
import remap_util as R
import warp_util as W
from coord_suite import GEO, to_device
from letterbox_util import bits


def f32(m):
    return tuple(float(np.float32(v)) for v in m)


def _two_per_frame(a, b, geo=GEO):
    return [(k, name) for k in range(len(geo)) for name in (a, b)]


# ---- rows of coefficients: warp and perspective

def matrices(w, h, dw, dh):
    """the matrix set of one frame: name -> m"""
    import tensor_stream as ts
    out = {
        "rot30": ts.warp_rotated_box(w / 2, h / 2, 1.7 * dw, 1.7 * dh, math.radians(30), dw, dh),
        "transpose": (0, 1, 0, 1, 0, 0),
        "mirror": (-1, 0, w, 0, 1, 0),
        "up_shear": (0.37, 0.1, 0.3 * w, 0.05, 0.37, 0.3 * h),
        "down4.6": (4.6, 0, w / 2 - 2.3 * dw, 0, 4.6, h / 2 - 2.3 * dh),
        "left": ts.warp_rotated_box(0, h / 2, w, h, 0.2, dw, dh),
        "right": ts.warp_rotated_box(w, h / 2, w, h, -0.3, dw, dh),
        "top": ts.warp_rotated_box(w / 2, 0, w, h, 2.0, dw, dh),
        "bottom": ts.warp_rotated_box(w / 2, h, w, h, -1.1, dw, dh),
        "far": (1, 0, 5000, 0, 1, -3000),
        "singular": (0, 0, w / 3, 0, 0, h / 3),
    }
    return {k: f32(m) for k, m in out.items()}


def homographies(w, h, dw, dh):
    """the homography set of one frame: name -> h.  Every one is in the domain (asserted): the horizon stays off the output"""
    def quad(pts, dx=0.0, dy=0.0):
        return P.from_quad([(x * w + dx, y * h + dy) for x, y in pts], dw, dh)
    mild = [(0.1, 0.1), (0.9, 0.15), (0.85, 0.9), (0.12, 0.85)]
    strong = [(0.42, 0.2), (0.58, 0.2), (0.98, 0.9), (0.02, 0.9)]  # the far edge is 6 x shorter than the near one
    c, s = math.cos(math.radians(30)), math.sin(math.radians(30))
    keyrot = [(0.5 + (x - 0.5) * c - (y - 0.5) * s * h / w, 0.5 + (x - 0.5) * s * w / h + (y - 0.5) * c) for x, y in [(0.3, 0.25), (0.7, 0.25), (0.85, 0.75), (0.15, 0.75)]]
    out = {
        "mild": quad(mild),
        "strong": quad(strong),
        "keyrot": quad(keyrot),
        "left": quad(mild, dx=-0.5 * w),
        "right": quad(mild, dx=0.5 * w),
        "top": quad(strong, dy=-0.5 * h),
        "bottom": quad(strong, dy=0.5 * h),
        "far": quad(mild, dx=5000, dy=-3000),
        "x4": tuple(4.0 * v for v in quad(mild)),
        "x3": tuple(3.0 * v for v in quad(keyrot)),  # h8 = 3: a scaling that rounds
        "affine": P.affine(matrices(w, h, dw, dh)["rot30"]),
    }
    out = {k: f32(v) for k, v in out.items()}
    for k, v in out.items():
        assert P.in_domain(v, dw, dh), (k, v)
    return out


def warp_full_set(dst):
    return [(k, m) for k, (w, h, _) in enumerate(GEO) for m in matrices(w, h, *dst).values()]


def persp_full_set(dst):
    return [(k, q) for k, (w, h, _) in enumerate(GEO) for q in homographies(w, h, *dst).values()]


def _rows(name, model, item_set, record, valid, staging, refusals, split, guard, gterm, capture):
    """the descriptor of a path whose request is [(frame, coefficients)].  item_set(w, h, dw, dh) -> {name: coefficients}; valid(w, h): the coefficients of a
    plain down-scale to 64 x 64; staging(pick), refusals(call, items): the path's own, below; the rest: item names of the shared cases"""
    def pick(picks, geo, dst):
        return [(k, item_set(geo[k][0], geo[k][1], *dst)[nm]) for k, nm in picks]

    def describe(fp, geo, items, **kw):
        import tensor_stream as ts
        return getattr(ts, "describe_" + name)(fp, list(geo), [(k,) + c for k, c in items], **kw)

    def records(N, items):
        return (1, (record(N) * 1)(record(N)(0, (ctypes.c_float * len(items[0][1]))(*items[0][1])))), lambda raw, ctx, outs: None

    return cs.Path(
        name=name, model=name, LIMIT=32, pick=pick, describe=describe, staging=lambda: staging(pick), refusals=refusals, records=records,
        call=lambda v, ys, uvs, items, fp, **kw: getattr(v, "convert_" + name)(ys, uvs, [(k,) + c for k, c in items], fp, **kw),
        output=lambda items, i, dst: (items[i][0], items[i][1], items[i][1], f"{name} {items[i][1]}"),
        virtual_frame=lambda y, uv, w, h, c, dst, border: model.virtual_frame(y, uv, w, h, c, dst[0], dst[1], border),
        expected=lambda oracle, c, dst, fcc, planes, norm, border, virtual: model.expected(oracle, None, None, 0, 0, c, dst, fcc, planes, norm, border, virtual=virtual),
        split_items=lambda geo: ((64, 64), pick([(k, split[k % 4]) for k in range(len(geo))], geo, (64, 64))),
        guard_items=lambda dst: pick(_two_per_frame(*guard), GEO, dst),
        gterm_items=lambda dst: pick(_two_per_frame(*gterm), GEO, dst),
        capture_dst=(64, 64), capture_items=lambda step, geo: pick(_two_per_frame(*capture, geo=geo), geo, (64, 64)),
        resident=lambda items: items, overwrite=lambda items, now: None,  # the coefficients travel in the kernel arguments: a replay cannot see new ones
        valid=lambda w, h: [(0, valid(w, h))], on_frame=lambda items, k: [(k, items[0][1])], broken=lambda items: [(3, items[0][1])])


def _warp_staging(pick):
    """the default budget stages every tile, 0 gathers every tile, 3 KiB stages some tiles and gathers others in one launch"""
    warps = pick([(2, nm) for nm in ("rot30", "up_shear", "down4.6", "left", "far")], GEO, (112, 112))

    def default(d):
        assert d["kernel"].endswith("staged,replicate>") and d["staged"] == len(warps) and d["lds"] > 3 * 1024

    def none(d):
        assert d["kernel"].endswith("gather,replicate>") and d["staged"] == 0 and d["lds"] == 0

    def mixed(d):  # "far" and "up_shear" tap little: they stage; the 30 degree warp at scale 1.7 does not fit 3 KiB
        assert d["kernel"].endswith("staged,replicate>") and 0 < d["staged"] < len(warps) and 0 < d["lds"] <= 3 * 1024
    return (112, 112), [(None, warps, default), ("0", warps, none), ("3", warps, mixed)]


def _warp_refusals(call, items):
    m = items[0][1]
    with pytest.raises(RuntimeError, match="-3"):
        call(border=(114, -1, 128))
    with pytest.raises(RuntimeError, match="-3"):
        call([(0, (float("nan"),) + m[1:])])
    with pytest.raises(RuntimeError, match="-3"):
        call([])
    with pytest.raises(RuntimeError, match="-2"):
        call([(0, (2.0 ** 25,) + m[1:])])


def _persp_staging(pick):
    """the default budget stages, 0 gathers every tile, 3 KiB stages some tiles and gathers others in one launch"""
    persps = pick([(2, nm) for nm in ("mild", "strong", "keyrot", "left", "far", "affine")], GEO, (112, 112))

    def default(d):
        assert d["kernel"].endswith("staged,replicate>") and d["staged"] >= 4 and d["lds"] > 3 * 1024

    def none(d):
        assert d["kernel"].endswith("gather,replicate>") and d["staged"] == 0 and d["lds"] == 0

    def mixed(d):  # "far" taps one pixel: it stages; the keystones do not fit 3 KiB
        assert d["kernel"].endswith("staged,replicate>") and 0 < d["staged"] < len(persps) and 0 < d["lds"] <= 3 * 1024
    return (112, 112), [(None, persps, default), ("0", persps, none), ("3", persps, mixed)]


def _persp_refusals(call, items):
    q = items[0][1]
    with pytest.raises(RuntimeError, match="-3"):
        call(border=(114, -1, 128))
    with pytest.raises(RuntimeError, match="-3"):
        call([(0, q[:7] + (float("nan"),) + q[8:])])
    with pytest.raises(RuntimeError, match="-3"):
        call([])
    with pytest.raises(RuntimeError, match="-2"):
        call([(0, (2.0 ** 25,) + q[1:])])
    with pytest.raises(RuntimeError, match="-2"):  # the horizon crosses the output
        call([(0, q[:6] + (-1 / 32, 0.0, 1.0))])


WARP = _rows("warp", W, matrices, lambda N: N.Warp, lambda w, h: W.scale_only(w, h, 64, 64), _warp_staging, _warp_refusals,
             split=["rot30", "up_shear", "left", "bottom"], guard=("rot30", "right"), gterm=("rot30", "top"), capture=("rot30", "left"))
PERSP = _rows("perspective", P, homographies, lambda N: N.Persp, lambda w, h: P.affine(W.scale_only(w, h, 64, 64)), _persp_staging, _persp_refusals,
              split=["mild", "strong", "left", "keyrot"], guard=("keyrot", "right"), gterm=("strong", "top"), capture=("strong", "left"))


# ---- device tables: remap and mesh

def padded_to_device(table):
    """a map or mesh with a row stride of 2 * columns + 6 floats and NaN in the padding, as a strided device view"""
    view, back = R.padded(table)
    t = torch.from_numpy(back).cuda()
    assert torch.isnan(t[:, 2 * table.shape[1]:]).all()
    return t[:, :2 * table.shape[1]].unflatten(1, (table.shape[1], 2))


def _device_tables(items):
    return [to_device(t) for _, t in items.tables] if items.dev is None else items.dev


def _by_kind(pick, kinds, geo, dst, **kw):
    """the capture case's order: every frame through its first kind, then every frame through its second"""
    return pick([(k, kinds[0]) for k in range(len(geo))] + [(k, kinds[1]) for k in range(len(geo))], geo, dst, **kw)


def _resident(items):
    items.dev = _device_tables(items)
    return items


def _overwrite(items, now):
    for t, (_, host) in zip(items.dev, now.tables):
        t.copy_(torch.from_numpy(host).cuda())


def _with(items, **fields):
    """`items` with other fields"""
    return cs.Tables(**{**vars(items), **fields})


def _table_refusals(call, items):
    """what remap and mesh refuse alike: a table index out of range and a negative hint; returns the valid device table"""
    t = items.dev[0]
    with pytest.raises(RuntimeError, match="-3"):
        call(_with(items, remaps=[(0, 1)]))
    with pytest.raises(RuntimeError, match="-3"):
        call(_with(items, dev=[(t, -5)]))
    return t


SHARED = ("transpose", "far")  # maps of the set that do not depend on the frame: one device map serves every frame


def remap_tables(tables, remaps, dev=None):
    return cs.Tables(tables=tables, remaps=remaps, dev=dev)


def remap_pick(picks, geo, dst):
    """the request of [(frame, name of one of its maps)]: a map "name@frame" per output"""
    return remap_tables([(f"{nm}@{k}", R.map_set(geo[k][0], geo[k][1], *dst)[nm]) for k, nm in picks], [(k, i) for i, (k, _) in enumerate(picks)])


def remap_full_set(dst):
    """every frame of GEO through its map set in one call, the frame-independent maps shared between the frames, and the barrel map of frame 2 a second time --
    the last map, which test_map_set_against_the_model sends pitch-padded"""
    maps, remaps, shared = [], [], {}
    for k, (w, h, _) in enumerate(GEO):
        for name, xy in R.map_set(w, h, *dst).items():
            if name in SHARED:
                if name not in shared:
                    shared[name] = len(maps)
                    maps.append((name, xy))
                remaps.append((k, shared[name]))
            else:
                remaps.append((k, len(maps)))
                maps.append((f"{name}@{k}", xy))
    remaps.append((2, len(maps)))
    maps.append(("barrel@2", R.map_set(GEO[2][0], GEO[2][1], *dst)["barrel"]))
    return remap_tables(maps, remaps)


def _remap_output(items, i, dst):
    k, m = items.remaps[i]
    name, xy = items.tables[m]
    return k, xy, name, f"map {name}"


def _remap_describe(fp, geo, items, **kw):
    import tensor_stream as ts
    return ts.describe_remap(fp, geo, [(0, 0)] * len(items.tables) if items.dev is None else items.dev, remaps=items.remaps, **kw)


def _remap_staging():
    """the default budget stages every tile of these maps, 0 gathers every tile, 3 KiB stages some tiles and gathers others in one launch
    (tests/test_remap_cpu.py proves all three from the footprints); and the default budget with the hints of remap_lds_hint"""
    import tensor_stream as ts
    geo, dst, names = R.STAGING_CASE
    assert geo == GEO[2]
    plain = _resident(remap_pick([(2, n) for n in names], GEO, dst))
    hints = [ts.remap_lds_hint(xy, geo[0], geo[1]) for _, xy in plain.tables]
    hinted = remap_tables(plain.tables, plain.remaps, list(zip(plain.dev, hints)))

    def staged(lds):
        def expect(d):
            assert d["kernel"].endswith("staged,replicate>") and d["lds"] == lds
        return expect

    def none(d):
        assert d["kernel"].endswith("gather,replicate>") and d["lds"] == 0

    def with_hints(d):  # the hints bring the launch's LDS below the default budget
        assert d["kernel"].endswith("staged,replicate>") and d["lds"] == max(hints) < 40 * 1024 - 64
    return dst, [(None, plain, staged(40 * 1024 - 64)), ("0", plain, none), ("3", plain, staged(3 * 1024 - 64)), (None, hinted, with_hints)]


def _remap_split(geo):
    """twelve maps -- four kinds for each of the three frame sizes -- shared by the outputs"""
    names = ["affine30", "barrel", "translate", "garbage"]
    sets = [R.map_set(w, h, 64, 64) for (w, h, _) in GEO[:3]]
    return (64, 64), _resident(remap_tables([(f"{nm}@{g}", sets[g][nm]) for g in range(3) for nm in names],
                                            [(k, (k % 3) * len(names) + k % len(names)) for k in range(len(geo))]))


def _remap_refusals(call, items):
    """... and, before the C call, a wrong device, dtype, shape or layout, and two maps for one frame"""
    xy = _table_refusals(call, items)
    for bad in (xy.cpu(), xy.double(), xy[:, :62], xy.permute(1, 0, 2)):
        with pytest.raises(ValueError):
            call(_with(items, dev=[bad]))
    with pytest.raises(ValueError):
        call(_with(items, dev=[xy, xy], remaps=None))


def _remap_records(N, items):
    xy = items.dev[0]
    ms = (N.Map * 1)(N.Map(None, 0, 0))

    def own(raw, ctx, outs):
        assert raw(ctx, outs) == -3       # a null map
        ms[0].xy = xy.data_ptr() + 4
        assert raw(ctx, outs) == -3       # ... one that is not 8-byte aligned
        ms[0].xy = xy.data_ptr()
    return (1, ms, 1, (N.Remap * 1)(N.Remap(0, 0))), own


_CAPTURE_MAPS = [("affine30", "barrel"), ("barrel", "garbage"), ("translate", "affine30")]  # the maps before capture, then what each replay overwrites them with

REMAP = cs.Path(
    name="remap", model="remap", LIMIT=32, pick=remap_pick, describe=_remap_describe, output=_remap_output,
    call=lambda v, ys, uvs, items, fp, **kw: v.convert_remap(ys, uvs, _device_tables(items), fp, remaps=items.remaps, **kw),
    virtual_frame=lambda y, uv, w, h, xy, dst, border: R.virtual_frame_from_map(y, uv, w, h, xy, border),
    expected=lambda oracle, xy, dst, fcc, planes, norm, border, virtual: R.expected(oracle, None, None, 0, 0, xy, fcc, planes, norm, border, virtual=virtual),
    staging=_remap_staging, split_items=_remap_split,
    guard_items=lambda dst: remap_pick(_two_per_frame("affine30", "garbage"), GEO, dst),
    gterm_items=lambda dst: remap_pick(_two_per_frame("barrel", "split"), GEO, dst),
    capture_dst=(64, 64), capture_items=lambda step, geo: _by_kind(remap_pick, _CAPTURE_MAPS[step], geo, (64, 64)),
    resident=_resident, overwrite=_overwrite,
    valid=lambda w, h: _resident(remap_tables([("shift", R.translation(64, 64, 4, 2))], [(0, 0)])),
    on_frame=lambda items, k: _with(items, remaps=[(k, 0)]), broken=lambda items: _with(items, remaps=[(0, 3)]),
    refusals=_remap_refusals, records=_remap_records)


def mesh_tables(tables, remaps, cell, dev=None, dense_call=False):
    """dense_call: the call also runs convert_remap on the uploaded E(mesh) and asserts the same bits"""
    return cs.Tables(tables=tables, remaps=remaps, dev=dev, cell=cell, dense_call=dense_call, dense={})


def mesh_pick(picks, geo, dst, cell=(16, 16), dense_call=False):
    """the request of [(frame, name of one of its meshes)]: a mesh "name@frame" per output"""
    return mesh_tables([(f"{nm}@{k}", M.mesh_set(geo[k][0], geo[k][1], *dst, cell)[nm]) for k, nm in picks], [(k, i) for i, (k, _) in enumerate(picks)], cell,
                       dense_call=dense_call)


MESH_NAMES = ("barrel", "affine30", "far", "garbage")


def mesh_full_set(dst, cell, dense_call=False):
    """every frame of GEO through its own mesh set and through the next frame's, the frame-independent mesh shared, and the barrel mesh of frame 2 a second time --
    the last mesh, which test_mesh_set_is_the_dense_call_on_the_expanded_mesh sends pitch-padded"""
    meshes, index = [], {}
    for k, (w, h, _) in enumerate(GEO):
        for name, mesh in M.mesh_set(w, h, *dst, cell).items():
            key = name if name == "far" else f"{name}@{k}"
            if key not in index:
                index[key] = len(meshes)
                meshes.append((key, mesh))
    remaps = []
    for k in range(len(GEO)):
        for own in (k, (k + 1) % len(GEO)):
            remaps += [(k, index[n if n == "far" else f"{n}@{own}"]) for n in MESH_NAMES]
    remaps.append((2, len(meshes)))
    meshes.append(("barrel@2", M.mesh_set(GEO[2][0], GEO[2][1], *dst, cell)["barrel"]))
    return mesh_tables(meshes, remaps, cell, dense_call=dense_call)


def _dense(items, m, dst):
    """E(mesh m), expanded once per request"""
    if m not in items.dense:
        items.dense[m] = M.expand(items.tables[m][1], *dst, items.cell)
    return items.dense[m]


def _mesh_call(v, ys, uvs, items, fp, **kw):
    got = v.convert_mesh(ys, uvs, _device_tables(items), fp, cell=items.cell, remaps=items.remaps, **kw)
    if items.dense_call:
        p = fp.parameters
        dst = (p.dst_width, p.dst_height)
        torch.cuda.synchronize()
        ref = v.convert_remap(ys, uvs, [to_device(_dense(items, m, dst)) for m in range(len(items.tables))], fp, remaps=items.remaps,
                              **{k: kw[k] for k in ("border", "width", "height")})
        torch.cuda.synchronize()
        for i in range(len(items.remaps)):
            assert np.array_equal(bits(got[i]), bits(ref[i])), ("differs from convert_remap of the expanded mesh", i, items.remaps[i], dst, items.cell, p.fourcc, p.planes,
                                                                p.normalization, kw["border"])
    return got


def _mesh_output(items, i, dst):
    k, m = items.remaps[i]
    name = items.tables[m][0]
    return k, _dense(items, m, dst), ("mesh", name, items.cell), f"mesh {name} cell {items.cell}"


def _mesh_describe(fp, geo, items, **kw):
    import tensor_stream as ts
    return ts.describe_mesh(fp, geo, [(0, 0)] * len(items.tables) if items.dev is None else items.dev, cell=items.cell, remaps=items.remaps, **kw)


def _mesh_staging():
    """the default budget, 0 (every tile gathers), 3 KiB (some tiles stage, the 30 degree warp and the barrel do not: the decisions are the dense call's on
    E(mesh), which tests/test_remap_cpu.py proves mixed for these warps) and the default budget with the hints of mesh_lds_hint"""
    import tensor_stream as ts
    geo, dst, _ = R.STAGING_CASE
    assert geo == GEO[2]
    w, h, _ = geo
    cell = (16, 16)
    meshes = [("barrel@2", M.barrel(*dst, cell, w, h)), ("affine30@2", M.affine(*dst, cell, w, h)), ("translate@2", M.translation(*dst, cell, 104, 34)),
              ("far", M.far(*dst, cell))]
    plain = _resident(mesh_tables(meshes, [(2, m) for m in range(len(meshes))], cell, dense_call=True))
    hints = [ts.mesh_lds_hint(m, dst, cell, w, h) for _, m in meshes]
    needs = [ts.remap_lds_hint(M.expand(m, *dst, cell), w, h) for _, m in meshes]
    assert hints == needs and min(needs) < 3 * 1024 - 64 < max(needs) < 40 * 1024 - 64  # 3 KiB: a mixed launch
    hinted = mesh_tables(meshes, plain.remaps, cell, list(zip(plain.dev, hints)), dense_call=True)

    def staged(lds):
        def expect(d):
            assert d["kernel"] == "vpp_mesh<O_F32_PLANAR,vec,staged,replicate>" and d["lds"] == lds
        return expect

    def none(d):
        assert d["kernel"] == "vpp_mesh<O_F32_PLANAR,vec,gather,replicate>" and d["lds"] == 0
    return dst, [(None, plain, staged(40 * 1024 - 64)), ("0", plain, none), ("3", plain, staged(3 * 1024 - 64)), (None, hinted, staged(max(hints)))]


def _mesh_split(geo):
    """the stabiliser's case: a mesh of its own per output"""
    dst, cell = (70, 66), (16, 16)
    n = len(geo)
    return dst, mesh_tables([(f"shake{k}", M.affine(*dst, cell, geo[k][0], geo[k][1], degrees=3.0 * k - 40, scale=0.8 + 0.01 * k)) for k in range(n)],
                            [(k, k) for k in range(n)], cell)


def _mesh_refusals(call, items):
    """... and a cell the library does not take; before the C call, a wrong device, dtype, shape or layout, two meshes for one frame, a cell that is no power of two"""
    mesh = _table_refusals(call, items)
    with pytest.raises(RuntimeError, match="-2"):
        call(_with(items, dev=[torch.zeros((2, 2, 2), device="cuda")], cell=(512, 512)))
    for bad in (mesh.cpu(), mesh.double(), mesh[:, :4], torch.zeros((5, 2, 5), device="cuda").permute(0, 2, 1)):
        with pytest.raises(ValueError):
            call(_with(items, dev=[bad]))
    with pytest.raises(ValueError):
        call(_with(items, dev=[mesh, mesh], remaps=None))
    with pytest.raises(ValueError):
        call(_with(items, cell=(16, 12)))


def _mesh_records(N, items):
    mesh = items.dev[0]
    ms = (N.Mesh * 1)(N.Mesh(None, 0, 4, 4, 0))

    def own(raw, ctx, outs):
        assert raw(ctx, outs) == -3       # a null mesh
        ms[0].xy = mesh.data_ptr() + 4
        assert raw(ctx, outs) == -3       # ... one that is not 8-byte aligned
        ms[0].xy = mesh.data_ptr()
        ms[0].log2_cw = 9
        assert raw(ctx, outs) == -2
        ms[0].log2_cw = 4
    return (1, ms, 1, (N.Remap * 1)(N.Remap(0, 0))), own


_CAPTURE_MESHES = [("affine30", "barrel"), ("barrel", "garbage"), ("far", "affine30")]  # the meshes before capture, then what each replay overwrites them with

MESH = cs.Path(
    name="mesh", model="remap", LIMIT=32, pick=mesh_pick, describe=_mesh_describe, output=_mesh_output, call=_mesh_call,
    virtual_frame=REMAP.virtual_frame, expected=REMAP.expected,  # of E(mesh): the mesh call is the dense call on it
    staging=_mesh_staging, split_items=_mesh_split,
    guard_items=lambda dst: mesh_pick(_two_per_frame("affine30", "garbage"), GEO, dst, cell=(16, 8)),
    gterm_items=None,  # tests/test_gpu_mesh.py writes its G-term case out: three variants, no second look at the default
    capture_dst=(70, 66), capture_items=lambda step, geo: _by_kind(mesh_pick, _CAPTURE_MESHES[step], geo, (70, 66), cell=(16, 8)),
    resident=_resident, overwrite=_overwrite,
    valid=lambda w, h: _resident(mesh_tables([("shift", M.translation(64, 64, (16, 16), 4, 2))], [(0, 0)], (16, 16))),
    on_frame=lambda items, k: _with(items, remaps=[(k, 0)]), broken=lambda items: _with(items, remaps=[(0, 3)]),
    refusals=_mesh_refusals, records=_mesh_records)
