"""The --bicubic mode of tools/warp_ab.py and tools/persp_ab.py: n rotated boxes (warp) or quadrilaterals (persp) of a 1080p frame (pitch 2048) to 112 x 112,
sampled BICUBIC -- the fused tsvpp_convert_warp_bicubic / tsvpp_convert_perspective_bicubic against what a caller does without them -- on one stream, timed with
HIP events.  Both tools write their section into profiles/warp_bicubic_ab.txt (warp_ab.py starts the file, persp_ab.py appends to it).

Protocol (tools/warp_ab.py's): per (configuration, n, leg) a warm-up, then `repeats` timed blocks of `iters` iterations each between two events on the stream; the
figure is the MEDIAN block, the spread (min .. max of the blocks) beside it.  Every iteration takes the next frame of a pool of 96 distinct 1080p frames
(318 MiB) and the next output set of a pool (> 256 MiB with the full-frame buffers of leg (b)), so that neither the last-level cache nor L2 serves a second pass.
Every leg is parity-checked before it is timed.
  (a)  one call of the new entry point                                              parity: tests/warp_bicubic_util.py's model + the CPU oracle, bit for bit
  (b)  what a caller does today: one tsvpp_convert of the frame to fp32 planar, then grid_sample(mode="bicubic", padding_mode="border", align_corners=False)
       with the grid built on the device from the same matrices, plus ((x - mean) * scale).half() for the fp16 configuration, all on the same stream
                                                                                    parity: NOT this library's arithmetic (a = -0.75 on RGB, no integer
                                                                                    rounding between the passes) -- the mean absolute difference to (a) is printed
  (c)  the BILINEAR call (tsvpp_convert_warp / _perspective) on the same items      parity: tests/warp_util.py / persp_util.py's model, bit for bit
"bytes" of (a) = what it must move: the footprint boxes of its tiles (tsvpp_*_bicubic_footprint: luma + chroma bytes) + the outputs; "roofline" = bytes / time as
a fraction of 8 TB/s.  "plan" = the host's planning time: the describe call of the same request, which touches no device, mean of 200 calls."""
import ctypes
import math
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

import persp_util as PU  # noqa: E402
import tensor_stream as ts  # noqa: E402
import tensor_util as T  # noqa: E402
import warp_bicubic_util as BU  # noqa: E402
import warp_util as WU  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tensor_stream import _native as N  # noqa: E402

W, H, PITCH = 1920, 1080, 2048
HBM = 8e12
DST = (112, 112)
BILINEAR, BICUBIC, BGR24, PLANAR = 1, 2, 2, 0
CONFIGS = [("112x112 BGR24 planar fp32", None, None), ("112x112 BGR24 planar fp16, ImageNet mean / std", T.F16, T.IMAGENET)]


def items_for(kind, n, seed):
    """warp: seeded boxes, sides 64 .. 512, inside the frame, each rotated about its centre by a seeded angle; persp: the same boxes with jittered corners"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        bw, bh = 2 * int(rng.integers(32, 257)), 2 * int(rng.integers(32, 257))
        l, t = 2 * int(rng.integers(0, (W - bw) // 2)), 2 * int(rng.integers(0, (H - bh) // 2))
        if kind == "warp":
            out.append(tuple(float(np.float32(v)) for v in ts.warp_rotated_box(l + bw / 2, t + bh / 2, bw, bh, float(rng.uniform(0, 2 * math.pi)), *DST)))
        else:
            j = lambda s: float(rng.uniform(-0.12, 0.12)) * s
            quad = [(l + j(bw), t + j(bh)), (l + bw + j(bw), t + j(bh)), (l + bw + j(bw), t + bh + j(bh)), (l + j(bw), t + bh + j(bh))]
            q = PU.from_quad(quad, *DST)
            assert q is not None and PU.in_domain(q, *DST)
            out.append(q)
    return out


def timed(fn, stream, repeats, iters, warm):
    for k in range(warm):
        fn(k)
    stream.synchronize()
    blocks, k = [], warm
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(iters):
            fn(k)
            k += 1
        e1.record(stream)
        e1.synchronize()
        blocks.append(e0.elapsed_time(e1) * 1e3 / iters)
    return blocks


def device_grid(hs, dev):
    """grid_sample's grid (n, dh, dw, 2), normalised for align_corners=False, from the homographies (n, 9) -- built on the device, per call"""
    dw, dh = DST
    u = (torch.arange(dw, device=dev, dtype=torch.float32) + 0.5).view(1, 1, dw)
    v = (torch.arange(dh, device=dev, dtype=torch.float32) + 0.5).view(1, dh, 1)
    h = hs.view(-1, 9, 1, 1)
    nw = h[:, 6] * u + h[:, 7] * v + h[:, 8]
    X = (h[:, 0] * u + h[:, 1] * v + h[:, 2]) / nw
    Y = (h[:, 3] * u + h[:, 4] * v + h[:, 5]) / nw
    return torch.stack((2 * X / W - 1, 2 * Y / H - 1), dim=-1)


def run(kind, a):
    assert torch.cuda.is_available(), "the A/B measures on the GPU: there is nothing to report without one"
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
    frame_arrs = [(N.NV12 * 1)(frames[k]) for k in range(a.frames)]
    frame_refs = [ctypes.byref(f) for f in frames]
    p_cubic = ts.FrameParameters(width=DST[0], height=DST[1], resize_type=BICUBIC, pixel_format=BGR24, planes_pos=PLANAR, normalization=True).parameters
    p_lin = ts.FrameParameters(width=DST[0], height=DST[1], resize_type=BILINEAR, pixel_format=BGR24, planes_pos=PLANAR, normalization=True).parameters
    p_full = ts.FrameParameters(pixel_format=BGR24, planes_pos=PLANAR, normalization=True).parameters
    full = [torch.empty((1, 3, H, W), dtype=torch.float32, device=dev) for _ in range(11)]  # 274 MiB of full-frame fp32 for leg (b)
    Rec = N.Warp if kind == "warp" else N.Persp
    K = 6 if kind == "warp" else 9
    name = "warp" if kind == "warp" else "perspective"
    e_cubic, e_desc = getattr(L, f"tsvpp_convert_{name}_bicubic"), getattr(L, f"tsvpp_describe_{name}_bicubic")
    e_lin, e_lin_t, e_foot = getattr(L, f"tsvpp_convert_{name}"), getattr(L, f"tsvpp_convert_{name}_tensor"), getattr(L, f"tsvpp_{'warp' if kind == 'warp' else 'persp'}_bicubic_footprint")
    model_lin = WU if kind == "warp" else PU
    lines = [f"# tools/{'warp' if kind == 'warp' else 'persp'}_ab.py --bicubic: {torch.cuda.get_device_name(0)}, {L.tsvpp_version().decode()}, frame pool {a.frames} x 1080p at pitch {PITCH} "
             f"({a.frames * PITCH * H * 3 // 2 >> 20} MiB), median of {a.repeats} blocks of {a.iters} iterations, one stream",
             f"# (a) = 1 x tsvpp_convert_{name}_bicubic   (b) = tsvpp_convert of the frame to fp32 planar + grid_sample(mode=bicubic), the grid built on the device "
             f"(+ normalise + .half())   (c) = 1 x tsvpp_convert_{name} (BILINEAR) on the same items",
             "# us per call, [min .. max of the blocks]; roofline = bytes (a) must move / time / 8 TB/s; plan = host time of the describe call, us; |b-a| = mean absolute difference of (b)'s result to (a)'s"]
    faster = True
    for cname, dtype, spec_ms in CONFIGS:
        tdt = torch.float32 if dtype is None else T.TORCH[dtype]
        elem = 4 if dtype is None else T.ESIZE[dtype]
        spec = None if dtype is None else ts.tensor_spec(dtype=tdt, mean=spec_ms[0], std=spec_ms[1])
        if spec is not None:
            t_mean = torch.tensor(list(spec.mean), dtype=torch.float32, device=dev).view(1, 3, 1, 1)
            t_scale = torch.tensor(list(spec.scale), dtype=torch.float32, device=dev).view(1, 3, 1, 1)
        lines += ["", f"## {cname}",
                  f"{'n':>3} | {'(a) us':>8} {'spread':>15} {'roofline':>8} {'plan':>6} | {'(b) us':>8} {'spread':>15} | {'(c) us':>8} {'spread':>15} | {'b / a':>6} {'a / c':>6} | {'|b-a|':>7}"]
        for n in [int(v) for v in a.ns.split(",")]:
            items = items_for(kind, n, seed=100 + n)
            out_bytes = 3 * DST[0] * DST[1] * elem
            sets = max(2, min(64, (300 << 20) // (n * out_bytes) + 1))
            pool = [vpp._alloc(p_cubic, DST[0], DST[1], n, None if dtype is None else tdt) for _ in range(sets)]
            out_arrs = [(ctypes.c_void_p * n)(*[t[i].data_ptr() for i in range(n)]) for t in pool]
            recs = (Rec * n)(*[Rec(0, (ctypes.c_float * K)(*c)) for c in items])
            hs = torch.tensor([list(c) + [0.0, 0.0, 1.0] if kind == "warp" else list(c) for c in items], dtype=torch.float32, device=dev)
            ctx, pc, pl, sref, pfull = vpp._ctx, ctypes.byref(p_cubic), ctypes.byref(p_lin), None if spec is None else ctypes.byref(spec), ctypes.byref(p_full)
            last_b = [None]

            def leg_a(k):
                if e_cubic(ctx, 1, frame_arrs[k % a.frames], n, recs, pc, sref, -1, -1, -1, out_arrs[k % sets], raw) != 0:
                    raise RuntimeError("the BICUBIC call failed")

            def leg_c(k):
                sts = (e_lin(ctx, 1, frame_arrs[k % a.frames], n, recs, pl, -1, -1, -1, out_arrs[k % sets], raw) if spec is None else
                       e_lin_t(ctx, 1, frame_arrs[k % a.frames], n, recs, pl, sref, -1, -1, -1, out_arrs[k % sets], raw))
                if sts != 0:
                    raise RuntimeError("the BILINEAR call failed")

            def leg_b(k):
                buf = full[k % len(full)]
                if L.tsvpp_convert(ctx, frame_refs[k % a.frames], pfull, buf.data_ptr(), raw) != 0:
                    raise RuntimeError("tsvpp_convert failed")
                x = F.grid_sample(buf.expand(n, -1, -1, -1), device_grid(hs, dev), mode="bicubic", padding_mode="border", align_corners=False)
                last_b[0] = x if spec is None else ((x - t_mean) * t_scale).half()

            def expected(leg, k, i):
                y, uv = ys[k % a.frames].cpu().numpy(), uvs[k % a.frames].cpu().numpy()
                q = (BU if leg == "a" else model_lin).expected(O, y, uv, W, H, items[i], DST, BGR24, PLANAR, True).view(np.float32)
                return q.ravel().view(np.uint8) if dtype is None else T.expected(q, 3, spec_ms, dtype)

            res, diff_ba = {}, float("nan")
            with torch.cuda.stream(stream):
                for leg, fn in (("a", leg_a), ("b", leg_b), ("c", leg_c)):
                    for t_ in pool:
                        t_.zero_()
                    fn(1)
                    stream.synchronize()
                    if leg == "b":
                        leg_a(1)
                        stream.synchronize()
                        diff_ba = float((last_b[0].float() - pool[1 % sets].float()).abs().mean())
                    else:
                        for i in range(n):
                            if not np.array_equal(T.bits(pool[1 % sets][i]), expected(leg, 1, i)):
                                raise SystemExit(f"PARITY FAILURE: leg ({leg}) {cname} n={n} item {i} {items[i]}")
                    res[leg] = timed(fn, stream, a.repeats, a.iters, warm=max(10, a.iters // 2))
            # the host's planning time: the describe call of the same request
            buf = ctypes.create_string_buffer(512)
            geo = (N.NV12 * 1)(N.NV12(None, None, PITCH, PITCH, W, H))
            t0 = time.perf_counter()
            for _ in range(200):
                e_desc(pc, sref, 1, geo, n, recs, -1, -1, -1, 1, buf, len(buf))
            plan = (time.perf_counter() - t0) / 200 * 1e6
            moved, out8 = 0, (ctypes.c_int32 * 8)()
            for i in range(n):
                for i0 in range(0, DST[1], 32):
                    for j0 in range(0, DST[0], 32):
                        e_foot(ctypes.byref(recs[i]), W, H, j0, min(j0 + 32, DST[0]) - 1, i0, min(i0 + 32, DST[1]) - 1, out8)
                        f = list(out8)
                        moved += (f[1] - f[0] + 1) * (f[3] - f[2] + 1) + 2 * (f[5] - f[4] + 1) * (f[7] - f[6] + 1)
                moved += out_bytes
            m = {k: statistics.median(v) for k, v in res.items()}
            sp = lambda v: f"{min(v):7.2f}..{max(v):<6.2f}"
            lines.append(f"{n:>3} | {m['a']:8.2f} {sp(res['a'])} {moved / (m['a'] * 1e-6) / HBM:8.4f} {plan:6.2f} | {m['b']:8.2f} {sp(res['b'])} | {m['c']:8.2f} {sp(res['c'])} | "
                         f"{m['b'] / m['a']:6.2f} {m['a'] / m['c']:6.2f} | {diff_ba:7.4f}")
            print(lines[-1], flush=True)
            faster = faster and m["a"] < m["b"]
            del pool, out_arrs
            torch.cuda.empty_cache()
    lines += ["", "# parity: (a) bit-exact against tests/warp_bicubic_util.py's model through the CPU oracle, (c) against the BILINEAR model, on frame 1 before timing; (b) is torch's arithmetic",
              f"# condition ((a) faster than (b) at every n, fp32 and fp16): {'met' if faster else 'NOT MET'}", ""]
    text = "\n".join(lines) + "\n"
    out = a.out if a.out else os.path.join(ROOT, "profiles", "warp_bicubic_ab.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w" if kind == "warp" else "a") as f:
        f.write(text)
    print(text)
    vpp.Close()
