#!/usr/bin/env python3
"""A/B: n quadrilaterals of a 1080p frame (pitch 2048) rectified to 112 x 112 -- the fused tsvpp_convert_perspective against what a user does without it -- on one
stream, timed with HIP events.

    python tools/persp_ab.py [--out profiles/persp_ab.txt] [--repeats 20] [--iters 50] [--ns 1,4,16,32]
    python tools/persp_ab.py --bicubic       tsvpp_convert_perspective_bicubic: the legs of tools/coord_bicubic_ab.py, appended to profiles/warp_bicubic_ab.txt

Protocol (tools/warp_ab.py's): per (configuration, n, leg) a warm-up, then `repeats` timed blocks of `iters` iterations each between two events on the stream; the
figure is the MEDIAN block, the spread (min .. max of the blocks) is printed beside it.  Every iteration takes the next frame of a pool of 96 distinct 1080p
frames (318 MiB) and the next output set of a pool, so that neither the 256 MiB last-level cache nor L2 serves a second pass over the same bytes.  Every leg is
parity-checked before it is timed.  Quads: seeded boxes with sides 64 .. 512 inside the frame, every corner moved by up to 15 % of the sides.
  (a)   one tsvpp_convert_perspective[_tensor] call on the quads                     parity: tests/persp_util.py's model + the CPU oracle, bit for bit
  (a0)  the same call with the affine part only: (h0 .. h5, 0, 0, 1)                 parity: the same
  (w)   one tsvpp_convert_warp[_tensor] call on those affine matrices (h0 .. h5)     parity: tests/warp_util.py's model + the CPU oracle, bit for bit; (a0) and
                                                                                     (w) have identical footprints and identical outputs
  (b)   what a user does today: one tsvpp_convert of the frame to fp32 planar, then a projective grid built on the device (bmm of the n homographies with the
        output's pixel centres, a divide, the normalisation) + grid_sample (bilinear, border padding, align_corners=False), plus ((x - mean) * scale).half()
        for the fp16 configuration, all on the same stream                           parity: NOT this library's arithmetic (it blends RGB, not NV12) -- the mean
                                                                                     absolute difference to (a) is printed as a check of the geometry
"bytes" of (a) = what it must move: the interval boxes of its tiles (tsvpp_persp_footprint: luma + chroma bytes) + the outputs; "roofline" = bytes / time as a
fraction of 8 TB/s.  a0 / w = the cost of the reciprocal and the denominator on identical footprints, to be read against (w)'s block spread; a / a0 = the cost
of the looser boxes.  "planning" = the host side alone, without a device: tsvpp_describe_perspective and tsvpp_describe_warp of the same requests, us per call."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tensor-stream_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import persp_util as PU  # noqa: E402  (the model of the perspective contract)
import tensor_stream as ts  # noqa: E402
import tensor_util as T  # noqa: E402  (the expected bits of the tensor entry points)
import warp_util as WU  # noqa: E402  (the model of the warp's contract)
from oracle import oracle as O  # noqa: E402
from tensor_stream import _native as N  # noqa: E402

W, H, PITCH = 1920, 1080, 2048
HBM = 8e12
DST = (112, 112)
BILINEAR, BGR24, PLANAR = 1, 2, 0
# (name, dtype or None, (mean, std))
CONFIGS = [("112x112 BGR24 planar fp32", None, None), ("112x112 BGR24 planar fp16, ImageNet mean / std", T.F16, T.IMAGENET)]


def quads_for(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        bw, bh = 2 * int(rng.integers(32, 257)), 2 * int(rng.integers(32, 257))  # sides 64 .. 512
        l, t = 2 * int(rng.integers(0, (W - bw) // 2)), 2 * int(rng.integers(0, (H - bh) // 2))
        j = rng.uniform(-0.15, 0.15, (4, 2)) * (bw, bh)
        quad = [(l + j[0][0], t + j[0][1]), (l + bw + j[1][0], t + j[1][1]), (l + bw + j[2][0], t + bh + j[2][1]), (l + j[3][0], t + bh + j[3][1])]
        h = ts.perspective_from_quad(quad, *DST)
        if PU.in_domain(h, *DST):
            out.append(h)
    return out


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
    return blocks, k - 1


def must_move(L, hs, elem):
    """bytes leg (a) must move: per tile the interval box in both planes, plus the outputs"""
    total = 0
    out8 = (ctypes.c_int32 * 8)()
    for h in hs:
        q = N.Persp(0, (ctypes.c_float * 9)(*h))
        for i0 in range(0, DST[1], 32):
            for j0 in range(0, DST[0], 32):
                if L.tsvpp_persp_footprint(ctypes.byref(q), W, H, j0, min(j0 + 32, DST[0]) - 1, i0, min(i0 + 32, DST[1]) - 1, out8) != 0:
                    raise RuntimeError("tsvpp_persp_footprint failed")
                f = list(out8)
                total += (f[1] - f[0] + 1) * (f[3] - f[2] + 1) + 2 * (f[5] - f[4] + 1) * (f[7] - f[6] + 1)
        total += 3 * DST[0] * DST[1] * elem
    return total


def planning(fn, calls=300):
    fn()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) * 1e6 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/persp_ab.txt; with --bicubic: profiles/warp_bicubic_ab.txt")
    ap.add_argument("--bicubic", action="store_true", help="the BICUBIC call against Convert + grid_sample(bicubic) and against the BILINEAR call (tools/coord_bicubic_ab.py)")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--ns", default="1,4,16,32")
    ap.add_argument("--frames", type=int, default=96)
    a = ap.parse_args()
    if a.bicubic:
        import coord_bicubic_ab
        return coord_bicubic_ab.run("persp", a)
    a.out = a.out or os.path.join(ROOT, "profiles", "persp_ab.txt")
    assert torch.cuda.is_available(), "tools/persp_ab.py measures on the GPU: there is nothing to report without one"
    O.build()
    L = N.lib()
    vpp = ts.VideoProcessor(device=0)
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
    frame_arrs = [(N.NV12 * 1)(frames[k]) for k in range(a.frames)]
    frame_refs = [ctypes.byref(f) for f in frames]
    geo = (N.NV12 * 1)(N.NV12(None, None, PITCH, PITCH, W, H))
    p = ts.FrameParameters(width=DST[0], height=DST[1], resize_type=BILINEAR, pixel_format=BGR24, planes_pos=PLANAR, normalization=True).parameters
    p_full = ts.FrameParameters(pixel_format=BGR24, planes_pos=PLANAR, normalization=True).parameters
    full = [torch.empty((1, 3, H, W), dtype=torch.float32, device=dev) for _ in range(11)]  # 274 MiB of full-frame fp32 for leg (b)
    # the output's pixel centres, homogeneous: (3, dh * dw), built once as a user would
    jj, ii = torch.meshgrid(torch.arange(DST[0], device=dev, dtype=torch.float32) + 0.5, torch.arange(DST[1], device=dev, dtype=torch.float32) + 0.5, indexing="xy")
    centres = torch.stack([jj.reshape(-1), ii.reshape(-1), torch.ones(DST[0] * DST[1], device=dev)])
    half = torch.tensor([W / 2, H / 2], dtype=torch.float32, device=dev).view(1, 2, 1)
    lines = [f"# tools/persp_ab.py: {torch.cuda.get_device_name(0)}, {L.tsvpp_version().decode()}, frame pool {a.frames} x 1080p at pitch {PITCH} "
             f"({a.frames * PITCH * H * 3 // 2 >> 20} MiB), median of {a.repeats} blocks of {a.iters} iterations, one stream",
             "# (a) = 1 x tsvpp_convert_perspective on seeded quads   (a0) = the same with the affine part only (h0..h5, 0, 0, 1)   (w) = 1 x tsvpp_convert_warp on those affine "
             "matrices   (b) = tsvpp_convert of the frame to fp32 planar + a projective grid built on the device + grid_sample (+ normalise + .half())",
             "# us per call, [min .. max of the blocks]; roofline = bytes (a) must move / time / 8 TB/s; w-spread = max - min of (w)'s blocks, us; |b-a| = mean absolute difference "
             "of (b)'s result to (a)'s; plan = host planning alone (describe call, no device), us: perspective quads / perspective affine / warp"]
    faster = True
    for name, dtype, spec_ms in CONFIGS:
        tdt = torch.float32 if dtype is None else T.TORCH[dtype]
        elem = 4 if dtype is None else T.ESIZE[dtype]
        spec = None if dtype is None else ts.tensor_spec(dtype=tdt, mean=spec_ms[0], std=spec_ms[1])
        if spec is not None:
            t_mean = torch.tensor(list(spec.mean), dtype=torch.float32, device=dev).view(1, 3, 1, 1)
            t_scale = torch.tensor(list(spec.scale), dtype=torch.float32, device=dev).view(1, 3, 1, 1)
        lines += ["", f"## {name}",
                  f"{'n':>3} | {'(a) us':>8} {'spread':>15} {'roofline':>8} | {'(a0) us':>8} {'spread':>15} | {'(w) us':>8} {'spread':>15} {'w-spread':>8} | {'(b) us':>8} {'spread':>15} | "
                  f"{'b / a':>6} {'a0 / w':>6} {'a / a0':>6} | {'|b-a|':>7} | {'plan a / a0 / w':>22}"]
        for n in [int(v) for v in a.ns.split(",")]:
            hs = quads_for(n, seed=200 + n)
            aff = [h[:6] for h in hs]
            hs0 = [m + (0.0, 0.0, 1.0) for m in aff]
            out_bytes = 3 * DST[0] * DST[1] * elem
            sets = max(2, min(64, (300 << 20) // (n * out_bytes) + 1))
            pool = [vpp._alloc(p, DST[0], DST[1], n, None if dtype is None else tdt) for _ in range(sets)]
            out_arrs = [(ctypes.c_void_p * n)(*[t[i].data_ptr() for i in range(n)]) for t in pool]
            q_full = (N.Persp * n)(*[N.Persp(0, (ctypes.c_float * 9)(*h)) for h in hs])
            q_aff = (N.Persp * n)(*[N.Persp(0, (ctypes.c_float * 9)(*h)) for h in hs0])
            w_aff = (N.Warp * n)(*[N.Warp(0, (ctypes.c_float * 6)(*m)) for m in aff])
            hmat = torch.tensor(hs, dtype=torch.float32, device=dev).view(n, 3, 3)
            ctx, pref, sref = vpp._ctx, ctypes.byref(p), None if spec is None else ctypes.byref(spec)
            pfull = ctypes.byref(p_full)
            last_b = [None]

            def leg_persp(qs):
                if spec is None:
                    def fn(k):
                        if L.tsvpp_convert_perspective(ctx, 1, frame_arrs[k % a.frames], n, qs, pref, -1, -1, -1, out_arrs[k % sets], raw) != 0:
                            raise RuntimeError("tsvpp_convert_perspective failed")
                else:
                    def fn(k):
                        if L.tsvpp_convert_perspective_tensor(ctx, 1, frame_arrs[k % a.frames], n, qs, pref, sref, -1, -1, -1, out_arrs[k % sets], raw) != 0:
                            raise RuntimeError("tsvpp_convert_perspective_tensor failed")
                return fn

            def leg_w(k):
                if spec is None:
                    sts = L.tsvpp_convert_warp(ctx, 1, frame_arrs[k % a.frames], n, w_aff, pref, -1, -1, -1, out_arrs[k % sets], raw)
                else:
                    sts = L.tsvpp_convert_warp_tensor(ctx, 1, frame_arrs[k % a.frames], n, w_aff, pref, sref, -1, -1, -1, out_arrs[k % sets], raw)
                if sts != 0:
                    raise RuntimeError("tsvpp_convert_warp failed")

            def leg_b(k):
                buf = full[k % len(full)]
                if L.tsvpp_convert(ctx, frame_refs[k % a.frames], pfull, buf.data_ptr(), raw) != 0:
                    raise RuntimeError("tsvpp_convert failed")
                pts = torch.matmul(hmat, centres)                       # (n, 3, dh * dw): numerators and denominator
                grid = (pts[:, :2] / pts[:, 2:3] / half - 1.0).permute(0, 2, 1).reshape(n, DST[1], DST[0], 2)
                x = F.grid_sample(buf.expand(n, -1, -1, -1), grid, mode="bilinear", padding_mode="border", align_corners=False)
                last_b[0] = x if spec is None else ((x - t_mean) * t_scale).half()

            def expected(leg, k, i):
                y, uv = ys[k % a.frames].cpu().numpy(), uvs[k % a.frames].cpu().numpy()
                if leg == "w":
                    q = WU.expected(O, y, uv, W, H, aff[i], DST, BGR24, PLANAR, True).view(np.float32)
                else:
                    q = PU.expected(O, y, uv, W, H, (hs if leg == "a" else hs0)[i], DST, BGR24, PLANAR, True).view(np.float32)
                return q.ravel().view(np.uint8) if dtype is None else T.expected(q, 3, spec_ms, dtype)

            res, diff_ba = {}, float("nan")
            with torch.cuda.stream(stream):
                for leg, fn in (("a", leg_persp(q_full)), ("a0", leg_persp(q_aff)), ("w", leg_w), ("b", leg_b)):
                    # parity first, on frame 1 and output set 1
                    for t_ in pool:
                        t_.zero_()
                    fn(1)
                    stream.synchronize()
                    if leg == "b":
                        leg_persp(q_full)(1)
                        stream.synchronize()
                        diff_ba = float((last_b[0].float() - pool[1 % sets].float()).abs().mean())
                    else:
                        for i in range(n):
                            if not np.array_equal(T.bits(pool[1 % sets][i]), expected(leg, 1, i)):
                                raise SystemExit(f"PARITY FAILURE: leg ({leg}) {name} n={n} output {i} {hs[i]}")
                    res[leg], _ = timed(fn, stream, a.repeats, a.iters, warm=max(10, a.iters // 2))
            buf = ctypes.create_string_buffer(512)
            if spec is None:
                plan = [planning(lambda: L.tsvpp_describe_perspective(pref, 1, geo, n, q_full, -1, -1, -1, 1, buf, len(buf))),
                        planning(lambda: L.tsvpp_describe_perspective(pref, 1, geo, n, q_aff, -1, -1, -1, 1, buf, len(buf))),
                        planning(lambda: L.tsvpp_describe_warp(pref, 1, geo, n, w_aff, -1, -1, -1, 1, buf, len(buf)))]
            else:
                plan = [planning(lambda: L.tsvpp_describe_perspective_tensor(pref, sref, 1, geo, n, q_full, -1, -1, -1, 1, buf, len(buf))),
                        planning(lambda: L.tsvpp_describe_perspective_tensor(pref, sref, 1, geo, n, q_aff, -1, -1, -1, 1, buf, len(buf))),
                        planning(lambda: L.tsvpp_describe_warp_tensor(pref, sref, 1, geo, n, w_aff, -1, -1, -1, 1, buf, len(buf)))]
            m = {k: statistics.median(v) for k, v in res.items()}
            sp = lambda v: f"{min(v):7.2f}..{max(v):<6.2f}"
            moved = must_move(L, hs, elem)
            lines.append(f"{n:>3} | {m['a']:8.2f} {sp(res['a'])} {moved / (m['a'] * 1e-6) / HBM:8.4f} | {m['a0']:8.2f} {sp(res['a0'])} | {m['w']:8.2f} {sp(res['w'])} "
                         f"{max(res['w']) - min(res['w']):8.2f} | {m['b']:8.2f} {sp(res['b'])} | {m['b'] / m['a']:6.2f} {m['a0'] / m['w']:6.2f} {m['a'] / m['a0']:6.2f} | {diff_ba:7.4f} | "
                         f"{plan[0]:6.1f} / {plan[1]:6.1f} / {plan[2]:6.1f}")
            print(lines[-1], flush=True)
            faster = faster and m["a"] < m["b"]
            del pool, out_arrs
            torch.cuda.empty_cache()
    lines += ["", "# parity: (a), (a0) bit-exact against tests/persp_util.py's model, (w) against tests/warp_util.py's, through the CPU oracle, on frame 1 before timing; (b) is torch's arithmetic",
              f"# condition ((a) faster than (b) at every n): {'met' if faster else 'NOT MET'}"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    vpp.Close()


if __name__ == "__main__":
    main()
