"""The BICUBIC map calls as tests/coord_suite.py's descriptors: tests/coord_paths.py's REMAP and MESH with the model of tests/remap_bicubic_util.py, asking for
BICUBIC whatever the suite's parameters name.  Staging: the BILINEAR path's runs (TSVPP_LDS_KB default / 0 / 3, its smaller hint), then the BICUBIC hint."""
import dataclasses

import coord_paths as cp
import remap_bicubic_util as RB
import remap_util as R
from coord_bicubic_paths import bicubic


def _path(base, name, hint, **extra):
    """extra: keyword of the call -> attribute of the request (the mesh call's cell); hint(ts, table, dst, request) -> the BICUBIC hint of one table"""
    more = lambda items: {k: getattr(items, a) for k, a in extra.items()}  # noqa: E731

    def call(v, ys, uvs, items, fp, **kw):
        return getattr(v, f"convert_{name}_bicubic")(ys, uvs, cp._device_tables(items), bicubic(fp), remaps=items.remaps, **more(items), **kw)

    def describe(fp, geo, items, **kw):
        import tensor_stream as ts
        tables = [(0, 0)] * len(items.tables) if items.dev is None else items.dev
        return getattr(ts, f"describe_{name}_bicubic")(bicubic(fp), geo, tables, remaps=items.remaps, **more(items), **kw)

    def says(kb):  # the describe line of a run: this call's kernel, gathering under TSVPP_LDS_KB=0 and staged otherwise
        def expect(d):
            assert d["kernel"].startswith(f"vpp_{name}_bicubic<") and f",{'gather' if kb == '0' else 'staged'}," in d["kernel"] and (d["lds"] > 0) == (kb != "0"), d
        return expect

    def staging():
        import tensor_stream as ts
        dst, runs = base.staging()
        plain = runs[0][1]
        hinted = cp._with(plain, dev=[(t, hint(ts, table, dst, plain)) for t, (_, table) in zip(plain.dev, plain.tables)])
        return dst, [(kb, items, says(kb)) for kb, items, _ in runs] + [(None, hinted, says(None))]

    return dataclasses.replace(base, name=f"{name}_bicubic", model="remap_bicubic", call=call, describe=describe, staging=staging,
                               virtual_frame=lambda y, uv, w, h, xy, dst, border: RB.virtual_frame_from_map(y, uv, w, h, xy, border))


REMAP_BICUBIC = _path(cp.REMAP, "remap", lambda ts, xy, dst, items: ts.remap_lds_hint(xy, *R.STAGING_CASE[0][:2], bicubic=True))
MESH_BICUBIC = _path(cp.MESH, "mesh", lambda ts, mesh, dst, items: ts.mesh_lds_hint(mesh, dst, items.cell, *R.STAGING_CASE[0][:2], bicubic=True), cell="cell")
