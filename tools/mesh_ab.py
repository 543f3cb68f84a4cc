#!/usr/bin/env python
"""A/B: lens undistortion of n 1080p frames (pitch 2048) through a barrel warp given as a control grid -- tsvpp_convert_mesh against tsvpp_convert_remap of the
expanded mesh, which computes the same bits -- on one stream of one MI355X.

    python tools/mesh_ab.py [--out profiles/mesh_ab.txt] [--repeats 20] [--ns 1,4,8,32]

Protocol (tools/remap_ab.py's): every leg is timed with HIP events around blocks of back-to-back calls on ONE stream, frames and outputs rotating through pools of
more than 256 MiB each (the MI355X has a 256 MiB last-level cache); the legs' blocks alternate, per leg the median of `repeats` blocks, with the blocks' min .. max.  Before it is timed every
leg is parity-checked (first and last output of a call) against tests/mesh_util.py's E(mesh) through tests/remap_util.py's model and the CPU oracle, bit for bit.
  (a)    one tsvpp_convert_mesh call, one shared mesh at cell 16 x 16 carrying the hint of tsvpp_mesh_lds_need
  (d)    one tsvpp_convert_remap call on E(mesh) in device memory, carrying the same hint
  (a32)  (a) at cell 32 x 32 (a different warp by the interpolation error, so its own E(mesh) and parity)
  (an)   (a) with one distinct mesh per output: a stabiliser's call (the n meshes hold the same values in n allocations)
  (dn)   (d) with one distinct dense map per output: what that stabiliser sends today (n copies of E(mesh), 16.6 MB each at 1080p)
"bytes" = what a call must move per output: the mesh (a, a32, an) or the dense map (d), the source bounding boxes of its tiles (tsvpp_remap_footprint of E(mesh):
luma + chroma bytes) and the output; "roofline" = (a)'s bytes / time as a fraction of 8 TB/s.  Expectation: (a) is not slower than (d) by more than the spread
(max - min) of (d)'s own blocks, in any row."""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tensor-stream_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import mesh_util as MU  # noqa: E402  (the model of the mesh's coordinate contract, and the barrel mesh)
import remap_util as RU  # noqa: E402  (the model of everything behind the coordinate)
import tensor_stream as ts  # noqa: E402
import tensor_util as T  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tensor_stream import _native as N  # noqa: E402

W, H, PITCH = 1920, 1080, 2048
HBM = 8e12
BILINEAR, BGR24, PLANAR, MERGED = 1, 2, 0, 1
WORKLOADS = [("undistort 1080p -> 1920x1080", (1920, 1080)), ("undistort + resize 1080p -> 640x640", (640, 640))]
ELEMENTS = [("BGR24 planar fp32", PLANAR, True, 4), ("BGR24 merged uint8", MERGED, False, 1)]


def timed(fns, stream, repeats, iters, warm):
    """us per call of every leg: `repeats` rounds, each timing one block of `iters` calls of every leg in turn, so that whatever else the machine does falls on
    all legs alike; every block moves on through the frame and output pools, so no leg finds what the leg before it left in the last-level cache"""
    for fn in fns.values():
        for k in range(warm):
            fn(k)
    stream.synchronize()
    blocks = {leg: [] for leg in fns}
    k = warm
    for _ in range(repeats):
        for leg, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for i in range(iters):
                fn(k + i)
            e1.record(stream)
            e1.synchronize()
            blocks[leg].append(e0.elapsed_time(e1) * 1e3 / iters)
            k += iters
    return blocks


def footprint_bytes(L, xy, dst):
    """per output: the source bounding boxes of all tiles, both planes"""
    total = 0
    out8 = (ctypes.c_int32 * 8)()
    ptr = xy.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    for (j0, j1, i0, i1) in RU.tiles(dst[0], dst[1], True):
        assert L.tsvpp_remap_footprint(ptr, 0, dst[0], dst[1], W, H, j0, j1, i0, i1, out8) == 0
        f = list(out8)
        total += (f[1] - f[0] + 1) * (f[3] - f[2] + 1) + 2 * (f[5] - f[4] + 1) * (f[7] - f[6] + 1)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_ab.txt"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--ns", default="1,4,8,32")
    ap.add_argument("--frames", type=int, default=96)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/mesh_ab.py measures on the GPU: there is nothing to report without one"
    O.build()
    L = N.lib()
    vpp = ts.VideoProcessor(device=0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    raw = stream.cuda_stream
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    gx = torch.arange(PITCH, device=dev, dtype=torch.float32)[None, :]
    gy = torch.arange(H, device=dev, dtype=torch.float32)[:, None]
    base_y = (128 + 80 * torch.sin(gx / 37) * torch.cos(gy / 29) + torch.randint(0, 8, (H, PITCH), device=dev, generator=gen)).to(torch.uint8)
    base_uv = (128 + 60 * torch.cos(gx / 53) * torch.sin(gy[:H // 2] / 17) + torch.randint(0, 8, (H // 2, PITCH), device=dev, generator=gen)).to(torch.uint8)
    ys = [base_y + (37 * k) % 256 for k in range(a.frames)]
    uvs = [base_uv + (37 * k) % 256 for k in range(a.frames)]
    frames = [N.NV12(ys[k].data_ptr(), uvs[k].data_ptr(), PITCH, PITCH, W, H) for k in range(a.frames)]
    host_frames = {}

    def host_frame(k):
        if k not in host_frames:
            host_frames[k] = (ys[k].cpu().numpy(), uvs[k].cpu().numpy())
        return host_frames[k]

    lines = [f"# tools/mesh_ab.py: {torch.cuda.get_device_name(0)}, {L.tsvpp_version().decode()}, frame pool {a.frames} x 1080p at pitch {PITCH} "
             f"({a.frames * PITCH * H * 3 // 2 >> 20} MiB), output pools of more than 256 MiB, median of {a.repeats} blocks, one stream",
             "# (a) = 1 x tsvpp_convert_mesh, one shared barrel mesh (k1 = -0.28, k2 = 0.07) at cell 16 x 16 with its LDS hint   (d) = 1 x tsvpp_convert_remap of E(mesh), same hint",
             "# (a32) = (a) at cell 32 x 32   (an) = (a) with one distinct mesh per output (the stabiliser's call)   (dn) = (d) with one distinct dense map per output",
             "# us per call, [min .. max of the blocks]; MB = bytes a call must move per output (mesh or map + tile footprints + output); roofline = (a)'s bytes / time / 8 TB/s;",
             "# ok = (a) <= (d) + (max - min of (d)'s blocks)"]
    all_ok = True
    virtual = {}
    for wname, dst in WORKLOADS:
        mesh = {c: MU.barrel(dst[0], dst[1], (c, c), W, H) for c in (16, 32)}
        dense = {c: MU.expand(mesh[c], dst[0], dst[1], (c, c)) for c in (16, 32)}
        hint = {c: ts.mesh_lds_hint(mesh[c], dst, (c, c), W, H) for c in (16, 32)}
        assert hint[16] == ts.remap_lds_hint(dense[16], W, H)
        d_mesh = {c: torch.from_numpy(mesh[c]).to(dev) for c in (16, 32)}
        d_dense = torch.from_numpy(dense[16]).to(dev)
        foot = {c: footprint_bytes(L, dense[c], dst) for c in (16, 32)}
        err = ts.mesh_error(RU.barrel(dst[0], dst[1], W, H), mesh[16], (16, 16)), ts.mesh_error(RU.barrel(dst[0], dst[1], W, H), mesh[32], (32, 32))
        for ename, planes, norm, elem in ELEMENTS:
            p = ts.FrameParameters(width=dst[0], height=dst[1], resize_type=BILINEAR, pixel_format=BGR24, planes_pos=planes, normalization=norm).parameters
            out_bytes = 3 * dst[0] * dst[1] * elem
            mb = {"a": mesh[16].nbytes + foot[16] + out_bytes, "d": dense[16].nbytes + foot[16] + out_bytes, "a32": mesh[32].nbytes + foot[32] + out_bytes}
            lines += ["", f"## {wname}, {ename}   (hint {hint[16]} bytes; MB per output: (a) {mb['a'] / 1e6:.2f}, (d) {mb['d'] / 1e6:.2f}, (a32) {mb['a32'] / 1e6:.2f}; "
                          f"the mesh is within {err[0]:.4f} px of the dense barrel map at cell 16, {err[1]:.4f} px at cell 32)",
                      f"{'n':>3} | {'(a) us':>9} {'spread':>19} {'roofline':>8} | {'(d) us':>9} {'spread':>19} | {'(a32) us':>9} {'spread':>19} | {'(an) us':>9} {'spread':>19} | "
                      f"{'(dn) us':>9} {'spread':>19} | {'a / d':>6} {'a32 / a':>7} {'an / a':>6} {'an / dn':>7} | ok"]
            for n in [int(v) for v in a.ns.split(",")]:
                sets = max(2, (257 << 20) // (n * out_bytes) + 1)
                pool = [vpp._alloc(p, dst[0], dst[1], n) for _ in range(sets)]
                out_arrs = [(ctypes.c_void_p * n)(*[t[i].data_ptr() for i in range(n)]) for t in pool]
                calls = max(1, a.frames // n)
                frame_arrs = [(N.NV12 * n)(*[frames[(c * n + i) % a.frames] for i in range(n)]) for c in range(calls)]
                shared = (N.Remap * n)(*[N.Remap(i, 0) for i in range(n)])
                own = (N.Remap * n)(*[N.Remap(i, i) for i in range(n)])
                copies = [d_mesh[16].clone() for _ in range(n)]
                dense_copies = [d_dense.clone() for _ in range(n)]
                mdn = (N.Map * n)(*[N.Map(t.data_ptr(), 0, hint[16]) for t in dense_copies])
                m16 = (N.Mesh * 1)(N.Mesh(d_mesh[16].data_ptr(), 0, 4, 4, hint[16]))
                m32 = (N.Mesh * 1)(N.Mesh(d_mesh[32].data_ptr(), 0, 5, 5, hint[32]))
                mn = (N.Mesh * n)(*[N.Mesh(t.data_ptr(), 0, 4, 4, hint[16]) for t in copies])
                md = (N.Map * 1)(N.Map(d_dense.data_ptr(), 0, hint[16]))
                pref = ctypes.byref(p)

                def leg_mesh(meshes, n_meshes, remaps):
                    def fn(k):
                        if L.tsvpp_convert_mesh(vpp._ctx, n, frame_arrs[k % calls], n_meshes, meshes, n, remaps, pref, -1, -1, -1, out_arrs[k % sets], raw) != 0:
                            raise RuntimeError("tsvpp_convert_mesh failed")
                    return fn

                def leg_dense(maps, n_maps, remaps):
                    def fn(k):
                        if L.tsvpp_convert_remap(vpp._ctx, n, frame_arrs[k % calls], n_maps, maps, n, remaps, pref, -1, -1, -1, out_arrs[k % sets], raw) != 0:
                            raise RuntimeError("tsvpp_convert_remap failed")
                    return fn

                def expected(c, i):
                    """call 0: output i samples frame i of the pool through E(mesh) of cell c"""
                    key = (c, dst, i)
                    if key not in virtual:
                        y, uv = host_frame(i)
                        virtual[key] = RU.virtual_frame_from_map(y, uv, W, H, dense[c])
                    return O.convert(virtual[key][0], virtual[key][1], fourcc=BGR24, planes=planes, normalization=norm)[0].ravel().view(np.uint8)

                iters = max(2, 40 // n) if dst[0] > 1000 else max(4, 160 // n)
                with torch.cuda.stream(stream):
                    legs = (("a", leg_mesh(m16, 1, shared), 16), ("d", leg_dense(md, 1, shared), 16), ("a32", leg_mesh(m32, 1, shared), 32), ("an", leg_mesh(mn, n, own), 16),
                            ("dn", leg_dense(mdn, n, own), 16))
                    for leg, fn, c in legs:
                        for t_ in pool:
                            t_.zero_()
                        fn(0)
                        stream.synchronize()
                        for i in sorted({0, n - 1}):
                            if not np.array_equal(T.bits(pool[0][i]), expected(c, i)):
                                raise SystemExit(f"PARITY FAILURE: leg ({leg}) {wname} {ename} n={n} output {i}")
                    res = timed({leg: fn for leg, fn, _ in legs}, stream, a.repeats, iters, warm=max(3, iters // 2))
                m = {k: statistics.median(v) for k, v in res.items()}
                sp = lambda v: f"{min(v):9.2f}..{max(v):<8.2f}"  # noqa: E731
                ok = m["a"] <= m["d"] + (max(res["d"]) - min(res["d"]))
                all_ok = all_ok and ok
                lines.append(f"{n:>3} | {m['a']:9.2f} {sp(res['a'])} {n * mb['a'] / (m['a'] * 1e-6) / HBM:8.4f} | {m['d']:9.2f} {sp(res['d'])} | {m['a32']:9.2f} {sp(res['a32'])} | "
                             f"{m['an']:9.2f} {sp(res['an'])} | {m['dn']:9.2f} {sp(res['dn'])} | {m['a'] / m['d']:6.2f} {m['a32'] / m['a']:7.2f} {m['an'] / m['a']:6.2f} {m['an'] / m['dn']:7.2f} | "
                             f"{'yes' if ok else 'NO'}")
                print(lines[-1], flush=True)
                del pool, out_arrs, copies, dense_copies
                torch.cuda.empty_cache()
    lines += ["", "# parity: every leg bit-exact against tests/mesh_util.py's E(mesh) through tests/remap_util.py's model and the CPU oracle, first and last output of call 0, before timing",
              f"# expectation ((a) not slower than (d) beyond the spread of (d)'s blocks, in every row): {'met' if all_ok else 'NOT MET'}"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    vpp.Close()


if __name__ == "__main__":
    main()
