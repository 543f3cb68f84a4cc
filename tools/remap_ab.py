#!/usr/bin/env python3
"""A/B: lens undistortion of n 1080p frames (pitch 2048) through ONE shared barrel map -- the fused tsvpp_convert_remap against what a user does without it -- on
one stream, timed with HIP events.

    python tools/remap_ab.py [--out profiles/remap_ab.txt] [--repeats 20] [--ns 1,4,8,32]

Protocol (tools/warp_ab.py's): per (workload, element, n, leg) a warm-up, then `repeats` timed blocks between two events on the stream; the figure is the MEDIAN
block, the spread (min .. max of the blocks) is printed beside it.  Every iteration takes the next n frames of a pool of 96 distinct 1080p frames (318 MiB) and
the next output set of a pool of more than 256 MiB, so that neither the 256 MiB last-level cache nor L2 serves a second pass over the same bytes.  Every leg of
this library is parity-checked (first and last output of a call) against tests/remap_util.py's / tests/warp_util.py's model through the CPU oracle, bit for bit,
before it is timed.
Workloads: 1080p -> 1920 x 1080 (undistort) and 1080p -> 640 x 640 (undistort + resize in one map); BGR24 planar fp32, and fp16 with ImageNet mean / std.
  (a)    one tsvpp_convert_remap[_tensor] call, the map carrying the hint of tsvpp_remap_lds_need
  (a40)  the same without a hint: the launch asks for the whole LDS budget
  (ag)   the same in a context of TSVPP_LDS_KB=0: every tile gathers from global memory
  (b)    what a user does today: tsvpp_convert_batch of the n frames to fp32 planar, then torch grid_sample (bilinear, border padding, align_corners=False) with
         the equivalent normalised grid, built once outside the timing; (x - mean) * scale -> .half() for the fp16 rows.  NOT this library's arithmetic (it
         blends RGB, not NV12): the mean absolute difference to (a) is printed as a check of the geometry
  (w)    one tsvpp_convert_warp[_tensor] call with the scale-only matrix of the same sizes: the cost floor without a map
"bytes" of (a) = what it must move: the map (8 bytes per output pixel, counted once per OUTPUT although the n outputs share one map -- after the first output the
map is re-read from cache) + the source bounding boxes of its tiles (tsvpp_remap_footprint: luma + chroma bytes) + the outputs; "roofline" = bytes / time as a
fraction of 8 TB/s.  The one condition: (a) is faster than (b) in every row."""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tensor-stream_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import remap_util as RU  # noqa: E402  (the model of the remap's contract, and the barrel map)
import tensor_stream as ts  # noqa: E402
import tensor_util as T  # noqa: E402  (the expected bits of the tensor entry points)
import warp_util as WU  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tensor_stream import _native as N  # noqa: E402

W, H, PITCH = 1920, 1080, 2048
HBM = 8e12
BILINEAR, BGR24, PLANAR = 1, 2, 0
WORKLOADS = [("undistort 1080p -> 1920x1080", (1920, 1080)), ("undistort + resize 1080p -> 640x640", (640, 640))]
ELEMENTS = [("BGR24 planar fp32", None, None), ("BGR24 planar fp16, ImageNet mean / std", T.F16, T.IMAGENET)]


def timed(fn, stream, repeats, iters, warm):
    for k in range(warm):
        fn(k)
    stream.synchronize()
    blocks = []
    k = warm
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(iters):
            fn(k)
            k += 1
        e1.record(stream)
        e1.synchronize()
        blocks.append(e0.elapsed_time(e1) * 1e3 / iters)  # us per iteration
    return blocks


def must_move(L, xy, dst, elem):
    """bytes leg (a) must move per output: the map, per tile the source bounding box in both planes, the output"""
    total = 8 * dst[0] * dst[1] + 3 * dst[0] * dst[1] * elem
    out8 = (ctypes.c_int32 * 8)()
    ptr = xy.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    for (j0, j1, i0, i1) in RU.tiles(dst[0], dst[1], True):
        assert L.tsvpp_remap_footprint(ptr, 0, dst[0], dst[1], W, H, j0, j1, i0, i1, out8) == 0
        f = list(out8)
        total += (f[1] - f[0] + 1) * (f[3] - f[2] + 1) + 2 * (f[5] - f[4] + 1) * (f[7] - f[6] + 1)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remap_ab.txt"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--ns", default="1,4,8,32")
    ap.add_argument("--frames", type=int, default=96)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/remap_ab.py measures on the GPU: there is nothing to report without one"
    O.build()
    L = N.lib()
    vpp = ts.VideoProcessor(device=0)
    # the gathering context: TSVPP_LDS_KB is read when a context is created, and only under the knob gate
    saved = {k: os.environ.get(k) for k in ("TSVPP_DEBUG_KNOBS", "TSVPP_LDS_KB")}
    os.environ.update(TSVPP_DEBUG_KNOBS="1", TSVPP_LDS_KB="0")
    vpp_gather = ts.VideoProcessor(device=0)
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    raw = stream.cuda_stream
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    # a smooth picture with a little noise (leg (b)'s result can then be compared with (a)'s), distinct per frame of the pool
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

    p_full = ts.FrameParameters(pixel_format=BGR24, planes_pos=PLANAR, normalization=True).parameters
    lines = [f"# tools/remap_ab.py: {torch.cuda.get_device_name(0)}, {L.tsvpp_version().decode()}, frame pool {a.frames} x 1080p at pitch {PITCH} "
             f"({a.frames * PITCH * H * 3 // 2 >> 20} MiB), output pools of more than 256 MiB, median of {a.repeats} blocks, one stream",
             "# (a) = 1 x tsvpp_convert_remap, one shared barrel map (k1 = -0.28, k2 = 0.07) with its LDS hint   (a40) = without the hint   (ag) = TSVPP_LDS_KB=0: every tile gathers",
             "# (b) = tsvpp_convert_batch to fp32 planar + torch grid_sample (+ normalise + .half())   (w) = 1 x tsvpp_convert_warp, scale-only matrix: the floor without a map",
             "# us per call, [min .. max of the blocks]; roofline = bytes (a) must move (map once per output -- a shared map is re-read from cache -- + tile footprints + outputs) / time / 8 TB/s;",
             "# |b-a| = mean absolute difference of (b)'s result to (a)'s"]
    faster = True
    virtual = {}
    for wname, dst in WORKLOADS:
        xy = RU.barrel(dst[0], dst[1], W, H)
        d_xy = torch.from_numpy(xy).to(dev)
        hint = ts.remap_lds_hint(xy, W, H)
        moved1 = {4: must_move(L, xy, dst, 4), 2: must_move(L, xy, dst, 2)}
        m_scale = WU.scale_only(W, H, *dst)
        # the normalised grid of leg (b): the inverse of remap_from_grid, x = ((gx + 1) w - 1) / 2
        d64 = d_xy.double()
        grid1 = torch.stack(((2 * d64[..., 0] + 1) / W - 1, (2 * d64[..., 1] + 1) / H - 1), dim=-1).float()[None]
        p = ts.FrameParameters(width=dst[0], height=dst[1], resize_type=BILINEAR, pixel_format=BGR24, planes_pos=PLANAR, normalization=True).parameters
        for ename, dtype, spec_ms in ELEMENTS:
            tdt = torch.float32 if dtype is None else T.TORCH[dtype]
            elem = 4 if dtype is None else T.ESIZE[dtype]
            spec = None if dtype is None else ts.tensor_spec(dtype=tdt, mean=spec_ms[0], std=spec_ms[1])
            if spec is not None:
                t_mean = torch.tensor(list(spec.mean), dtype=torch.float32, device=dev).view(1, 3, 1, 1)
                t_scale = torch.tensor(list(spec.scale), dtype=torch.float32, device=dev).view(1, 3, 1, 1)
            lines += ["", f"## {wname}, {ename}   (hint {hint} bytes; {moved1[elem] / 1e6:.2f} MB per output)",
                      f"{'n':>3} | {'(a) us':>9} {'spread':>19} {'roofline':>8} | {'(a40) us':>9} {'spread':>19} | {'(ag) us':>9} {'spread':>19} | {'(b) us':>9} {'spread':>19} | "
                      f"{'(w) us':>9} {'spread':>19} | {'b / a':>6} {'a / w':>6} {'a / ag':>6} {'a / a40':>7} | {'|b-a|':>7}"]
            for n in [int(v) for v in a.ns.split(",")]:
                out_bytes = 3 * dst[0] * dst[1] * elem
                sets = max(2, (257 << 20) // (n * out_bytes) + 1)
                pool = [vpp._alloc(p, dst[0], dst[1], n, None if dtype is None else tdt) for _ in range(sets)]
                out_arrs = [(ctypes.c_void_p * n)(*[t[i].data_ptr() for i in range(n)]) for t in pool]
                full_sets = max(2, (257 << 20) // (n * 3 * W * H * 4) + 1)
                full = [torch.empty((n, 3, H, W), dtype=torch.float32, device=dev) for _ in range(full_sets)]
                full_arrs = [(ctypes.c_void_p * n)(*[t[i].data_ptr() for i in range(n)]) for t in full]
                calls = max(1, a.frames // n)
                frame_arrs = [(N.NV12 * n)(*[frames[(c * n + i) % a.frames] for i in range(n)]) for c in range(calls)]
                remaps = (N.Remap * n)(*[N.Remap(i, 0) for i in range(n)])
                warps = (N.Warp * n)(*[N.Warp(i, (ctypes.c_float * 6)(*m_scale)) for i in range(n)])
                map_hint = (N.Map * 1)(N.Map(d_xy.data_ptr(), 0, hint))
                map_plain = (N.Map * 1)(N.Map(d_xy.data_ptr(), 0, 0))
                pref, sref, pfull = ctypes.byref(p), None if spec is None else ctypes.byref(spec), ctypes.byref(p_full)
                grid = grid1.expand(n, -1, -1, -1)
                last_b = [None]

                def leg_remap(ctx, maps):
                    if spec is None:
                        def fn(k):
                            if L.tsvpp_convert_remap(ctx, n, frame_arrs[k % calls], 1, maps, n, remaps, pref, -1, -1, -1, out_arrs[k % sets], raw) != 0:
                                raise RuntimeError("tsvpp_convert_remap failed")
                    else:
                        def fn(k):
                            if L.tsvpp_convert_remap_tensor(ctx, n, frame_arrs[k % calls], 1, maps, n, remaps, pref, sref, -1, -1, -1, out_arrs[k % sets], raw) != 0:
                                raise RuntimeError("tsvpp_convert_remap_tensor failed")
                    return fn

                def leg_w(k):
                    if spec is None:
                        sts = L.tsvpp_convert_warp(vpp._ctx, n, frame_arrs[k % calls], n, warps, pref, -1, -1, -1, out_arrs[k % sets], raw)
                    else:
                        sts = L.tsvpp_convert_warp_tensor(vpp._ctx, n, frame_arrs[k % calls], n, warps, pref, sref, -1, -1, -1, out_arrs[k % sets], raw)
                    if sts != 0:
                        raise RuntimeError("tsvpp_convert_warp failed")

                def leg_b(k):
                    buf = full[k % full_sets]
                    if L.tsvpp_convert_batch(vpp._ctx, n, frame_arrs[k % calls], pfull, full_arrs[k % full_sets], raw) != 0:
                        raise RuntimeError("tsvpp_convert_batch failed")
                    x = F.grid_sample(buf, grid, mode="bilinear", padding_mode="border", align_corners=False)
                    last_b[0] = x if spec is None else x.sub(t_mean).mul(t_scale).half()

                def expected(leg, i):
                    """call 0: output i samples frame i of the pool"""
                    key = ("w" if leg == "w" else "a", dst, i)
                    if key not in virtual:
                        y, uv = host_frame(i)
                        virtual[key] = WU.virtual_frame(y, uv, W, H, m_scale, *dst) if leg == "w" else RU.virtual_frame_from_map(y, uv, W, H, xy)
                    q = O.convert(virtual[key][0], virtual[key][1], fourcc=BGR24, planes=PLANAR, normalization=True)[0]
                    return q.ravel().view(np.uint8) if dtype is None else T.expected(q, 3, spec_ms, dtype)

                res, diff_ba = {}, float("nan")
                iters = max(2, 40 // n) if dst[0] > 1000 else max(4, 160 // n)
                with torch.cuda.stream(stream):
                    legs = (("a", leg_remap(vpp._ctx, map_hint)), ("a40", leg_remap(vpp._ctx, map_plain)), ("ag", leg_remap(vpp_gather._ctx, map_plain)), ("b", leg_b), ("w", leg_w))
                    for leg, fn in legs:
                        # parity first, on call 0 and output set 0
                        for t_ in pool:
                            t_.zero_()
                        fn(0)
                        stream.synchronize()
                        if leg == "b":
                            legs[0][1](0)
                            stream.synchronize()
                            diff_ba = float((last_b[0].float() - pool[0].float()).abs().mean())
                        else:
                            for i in sorted({0, n - 1}):
                                if not np.array_equal(T.bits(pool[0][i]), expected(leg, i)):
                                    raise SystemExit(f"PARITY FAILURE: leg ({leg}) {wname} {ename} n={n} output {i}")
                        res[leg] = timed(fn, stream, a.repeats, iters, warm=max(3, iters // 2))
                m = {k: statistics.median(v) for k, v in res.items()}
                sp = lambda v: f"{min(v):9.2f}..{max(v):<8.2f}"  # noqa: E731
                lines.append(f"{n:>3} | {m['a']:9.2f} {sp(res['a'])} {n * moved1[elem] / (m['a'] * 1e-6) / HBM:8.4f} | {m['a40']:9.2f} {sp(res['a40'])} | {m['ag']:9.2f} {sp(res['ag'])} | "
                             f"{m['b']:9.2f} {sp(res['b'])} | {m['w']:9.2f} {sp(res['w'])} | {m['b'] / m['a']:6.2f} {m['a'] / m['w']:6.2f} {m['a'] / m['ag']:6.2f} {m['a'] / m['a40']:7.2f} | "
                             f"{diff_ba:7.4f}")
                print(lines[-1], flush=True)
                faster = faster and m["a"] < m["b"]
                del pool, out_arrs, full, full_arrs, last_b
                torch.cuda.empty_cache()
    lines += ["", "# parity: (a), (a40), (ag) bit-exact against tests/remap_util.py's model and (w) against tests/warp_util.py's, through the CPU oracle, first and last output of call 0, before "
              "timing; (b) is torch's arithmetic",
              f"# condition ((a) faster than (b) in every row): {'met' if faster else 'NOT MET'}"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    vpp.Close()
    vpp_gather.Close()


if __name__ == "__main__":
    main()
