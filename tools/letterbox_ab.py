#!/usr/bin/env python3
"""A/B: n 1080p frames (pitch 2048) letterboxed into 640 x 640 canvases -- (loop) the three steps the library offered before tsvpp_convert_letterbox: one
tsvpp_convert_batch to 640 x 360 into a temporary, a fill of the canvases, a strided copy of the temporary into them -- against (fused) ONE
tsvpp_convert_letterbox -- on one stream, timed with HIP events.

    python tools/letterbox_ab.py [--out profiles/letterbox_ab.txt] [--repeats 20] [--iters 30] [--ns 1,8,32]
    python tools/letterbox_ab.py --dtype f16 [--mean a,b,c] [--std a,b,c]     the tensor legs: tsvpp_convert_letterbox_tensor (see tensor_main; appends to profiles/tensor_ab.txt)
    python tools/letterbox_ab.py --area [--out profiles/letterbox_area_ab.txt]  tsvpp_convert_letterbox_area against the loop it replaces and the BILINEAR letterbox (see area_main)

Method: per (configuration, n, leg) a warm-up, then `repeats` timed blocks of `iters` iterations each between two events on the stream; the figure is the MEDIAN
block, the spread (min .. max of the blocks) is printed beside it.  Every iteration takes the next n frames of a pool of 96 distinct frames (316 MB) and the next
canvas set of a pool of more than 256 MiB, so that neither the 256 MiB last-level cache nor L2 serves a second pass over the same bytes.  Before a number is
printed both legs are parity-checked against the CPU oracle on the last canvas set they wrote (every canvas, bit for bit: pad from the oracle's conversion of a
constant frame, the inner block from the oracle's resize of the frame to 640 x 360).  The fill and the copy of (loop) are torch's (one kernel each); the pad is gray
114, whose three channels are equal, so one fill serves every layout.
"bytes" = what a frame moves at the least: its source planes (1920 x 1080 x 1.5) + its canvas; "roofline" = bytes / time as a fraction of 8 TB/s."""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tensor-stream_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import tensor_stream as ts  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tensor_stream import _native as N  # noqa: E402

W, H, PITCH = 1920, 1080, 2048
CW, CH = 640, 640
PAD = (114, 128, 128)
HBM = 8e12
CONFIGS = [("640x640 BILINEAR BGR24 planar fp32", 1, 2, 0, True),
           ("640x640 BILINEAR RGB24 merged uint8", 1, 1, 1, False)]


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


def expected(y, uv, rect, rt, fcc, planes, norm):
    """the canvas of one frame from the oracle alone, as bytes"""
    left, top, iw, ih = rect
    pref = O.convert(np.full((2, 2), PAD[0], np.uint8), np.array([[PAD[1], PAD[2]]], np.uint8), fourcc=fcc, planes=planes, normalization=norm)[0]
    inner = O.convert(y[:, :W], uv[:, :W], dst=(iw, ih), resize_type=rt, fourcc=fcc, planes=planes, normalization=norm, nthreads=8)[0]
    if planes == 0:
        out = np.empty((3, CH, CW), pref.dtype)
        out[:] = pref.reshape(3, 2, 2)[:, 0, 0][:, None, None]
        out[:, top:top + ih, left:left + iw] = inner.reshape(3, ih, iw)
    else:
        out = np.empty((CH, CW, 3), pref.dtype)
        out[:] = pref.reshape(2, 2, 3)[0, 0]
        out[top:top + ih, left:left + iw, :] = inner.reshape(ih, iw, 3)
    return out.ravel().view(np.uint8)


def tensor_main(a):
    """The tensor legs at the first configuration of CONFIGS (1080p at pitch 2048 into 640 x 640 BILINEAR BGR24 planar), same protocol (one stream, frames and
    canvases rotating through more than 256 MiB, median of the blocks with their spread):
      (a) one tsvpp_convert_letterbox_tensor call with --dtype / --mean / --std: the fused call
      (b) one tsvpp_convert_letterbox call (fp32) followed by ((x - mean) * scale).to(dtype) in torch on the same stream: what a caller does without (a)
      (c) the tsvpp_convert_letterbox call of (b) alone: the yardstick
    Every leg is parity-checked, bit for bit, against tests/tensor_util.py on the last canvas set it wrote.  bytes per frame: the source planes (1920 x 1080 x 1.5)
    + the canvases a leg writes (+ for (b): the fp32 canvas read back)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tensor_util as T  # the expected bits of the tensor entry points: only these legs need the tests directory
    O.build()
    L = N.lib()
    vpp = ts.VideoProcessor(device=0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    raw = stream.cuda_stream
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    base_y = torch.randint(0, 256, (H, PITCH), dtype=torch.uint8, device=dev, generator=gen)
    base_uv = torch.randint(0, 256, (H // 2, PITCH), dtype=torch.uint8, device=dev, generator=gen)
    ys = [base_y + (37 * k) % 256 for k in range(a.frames)]
    uvs = [base_uv + (37 * k) % 256 for k in range(a.frames)]
    frames = [N.NV12(ys[k].data_ptr(), uvs[k].data_ptr(), PITCH, PITCH, W, H) for k in range(a.frames)]
    rect = ts.letterbox_rect(W, H, CW, CH)
    name, rt, fcc, planes, norm = CONFIGS[0]
    mean, std = [float(v) for v in a.mean.split(",")], [float(v) for v in a.std.split(",")]
    tdt = T.TORCH[a.dtype]
    spec = ts.tensor_spec(dtype=tdt, mean=mean, std=std)
    t_mean = torch.tensor(list(spec.mean), dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    t_scale = torch.tensor(list(spec.scale), dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    p = ts.FrameParameters(width=CW, height=CH, resize_type=rt, pixel_format=fcc, planes_pos=planes, normalization=norm).parameters
    b32, bel, src = 3 * CW * CH * 4, 3 * CW * CH * T.ESIZE[a.dtype], W * H * 3 // 2
    moved = {"a": src + bel, "b": src + 2 * b32 + bel, "c": src + b32}
    lines = ["", f"# tools/letterbox_ab.py --dtype {a.dtype} --mean {a.mean} --std {a.std}: {torch.cuda.get_device_name(0)}, {L.tsvpp_version().decode()}, frame pool "
             f"{a.frames} x 1080p pitch {PITCH} ({a.frames * PITCH * H * 3 // 2 >> 20} MiB), median of {a.repeats} blocks of {a.iters} iterations, one stream",
             f"# {name.replace('fp32', a.dtype)}: (a) = 1 x tsvpp_convert_letterbox_tensor   (b) = 1 x tsvpp_convert_letterbox (fp32) + ((x - mean) * scale).to({a.dtype}) in torch   "
             "(c) = the fp32 call of (b) alone", "# us per call, [min .. max of the blocks]; roofline = moved bytes / time / 8 TB/s",
             f"{'n':>3} | {'(a) us':>8} {'spread':>17} {'roofline':>8} | {'(b) us':>8} {'spread':>17} {'roofline':>8} | {'(c) us':>8} {'spread':>17} {'roofline':>8} | {'a / c':>6} {'b / a':>6}"]
    for n in [int(v) for v in a.ns.split(",")]:
        sets, sets_el = max(2, (300 << 20) // (n * b32) + 1), max(2, (300 << 20) // (n * bel) + 1)
        pool32 = [vpp._alloc(p, CW, CH, n) for _ in range(sets)]
        pool_el = [vpp._alloc(p, CW, CH, n, tdt) for _ in range(sets_el)]
        groups = max(1, a.frames // n)
        frame_arrs = [(N.NV12 * n)(*[frames[(g * n + i) % a.frames] for i in range(n)]) for g in range(groups)]
        arr32 = [(ctypes.c_void_p * n)(*[t[i].data_ptr() for i in range(n)]) for t in pool32]
        arr_el = [(ctypes.c_void_p * n)(*[t[i].data_ptr() for i in range(n)]) for t in pool_el]
        ctx, pref, sref, lb, lb_t = vpp._ctx, ctypes.byref(p), ctypes.byref(spec), L.tsvpp_convert_letterbox, L.tsvpp_convert_letterbox_tensor
        last_b = [None]

        def leg_a(k):
            if lb_t(ctx, n, frame_arrs[k % groups], pref, sref, None, PAD[0], PAD[1], PAD[2], arr_el[k % sets_el], raw) != 0:
                raise RuntimeError("tsvpp_convert_letterbox_tensor failed")

        def leg_c(k):
            if lb(ctx, n, frame_arrs[k % groups], pref, None, PAD[0], PAD[1], PAD[2], arr32[k % sets], raw) != 0:
                raise RuntimeError("tsvpp_convert_letterbox failed")

        def leg_b(k):
            leg_c(k)
            last_b[0] = ((pool32[k % sets] - t_mean) * t_scale).to(tdt)

        res = {}
        with torch.cuda.stream(stream):
            for leg, fn in (("a", leg_a), ("b", leg_b), ("c", leg_c)):
                for t in pool32 + pool_el:
                    t.zero_()
                torch.cuda.synchronize()
                blocks, last = timed(fn, stream, a.repeats, a.iters, warm=max(5, a.iters // 2))
                res[leg] = blocks
                got = {"a": pool_el[last % sets_el], "b": last_b[0], "c": pool32[last % sets]}[leg]
                want_spec, want_dt = ((mean, std), a.dtype) if leg != "c" else (T.IDENTITY, T.F32)
                for i in range(n):
                    f = ((last % groups) * n + i) % a.frames
                    q = expected(ys[f].cpu().numpy(), uvs[f].cpu().numpy(), rect, rt, fcc, planes, norm).view(np.float32)
                    if not np.array_equal(T.bits(got[i]), T.expected(q, 3, want_spec, want_dt)):
                        raise SystemExit(f"PARITY FAILURE: leg ({leg}) n={n} canvas {i}")
        m = {k: statistics.median(v) for k, v in res.items()}
        sp = lambda v: f"{min(v):8.2f}..{max(v):<7.2f}"
        lines.append(f"{n:>3} | " + " | ".join(f"{m[k]:8.2f} {sp(res[k])} {n * moved[k] / (m[k] * 1e-6) / HBM:8.4f}" for k in "abc") + f" | {m['a'] / m['c']:6.2f} {m['b'] / m['a']:6.2f}")
        print(lines[-1], flush=True)
        if n == max(int(v) for v in a.ns.split(",")):
            ok = m["a"] - m["c"] <= max(res["c"]) - min(res["c"])
            tail = f"# expectation at n = {n}: (a) not slower than (c) by more than the spread of (c)'s blocks ({max(res['c']) - min(res['c']):.2f} us): (a) - (c) = {m['a'] - m['c']:+.2f} us: {'met' if ok else 'NOT MET'}"
        del pool32, pool_el
        torch.cuda.empty_cache()
    lines += ["# parity: every leg bit-exact against tests/tensor_util.py (the CPU oracle's fp32 canvas, the float32 affine step, round to nearest even) on the last canvas set of every row", tail]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:  # (appends: tools/rois_ab.py --dtype fills the same file)
        f.write(text)
    print(text)
    vpp.Close()


AREA_GEOS = [("1080p -> 640x640 (P = 1)", 1920, 1080, 2048, (640, 640)), ("1080p -> 608x608 (P = 57)", 1920, 1080, 2048, (608, 608)),
             ("1366x768 -> 640x640 (P = 320 on x)", 1366, 768, 2048, (640, 640))]
AREA_FLAVOURS = [("BGR24 planar fp32", 2, 0, True, None), ("RGB24 merged uint8", 1, 1, False, None), ("BGR24 planar fp16, ImageNet mean / std", 2, 0, True, "f16")]
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def expected_geo(y, uv, w, rect, canvas, rt, fcc, planes, norm):
    """expected() for any frame width and canvas: the fp32 / uint8 canvas of one frame from the oracle alone, as an array of the canvas's shape"""
    left, top, iw, ih = rect
    cw, ch = canvas
    pref = O.convert(np.full((2, 2), PAD[0], np.uint8), np.array([[PAD[1], PAD[2]]], np.uint8), fourcc=fcc, planes=planes, normalization=norm)[0]
    inner = O.convert(y[:, :w], uv[:, :w], dst=(iw, ih), resize_type=rt, fourcc=fcc, planes=planes, normalization=norm, nthreads=8)[0]
    if planes == 0:
        out = np.empty((3, ch, cw), pref.dtype)
        out[:] = pref.reshape(3, 2, 2)[:, 0, 0][:, None, None]
        out[:, top:top + ih, left:left + iw] = inner.reshape(3, ih, iw)
    else:
        out = np.empty((ch, cw, 3), pref.dtype)
        out[:] = pref.reshape(2, 2, 3)[0, 0]
        out[top:top + ih, left:left + iw, :] = inner.reshape(ih, iw, 3)
    return out


def area_main(a):
    """tsvpp_convert_letterbox_area, same protocol (one stream, frames and canvases rotating through more than 256 MiB, median of the blocks with their spread, every
    leg parity-checked, bit for bit, against the CPU oracle on the last canvas set it wrote before its figure is printed):
      (a)  one tsvpp_convert_letterbox_area call: the fused call
      (b)  the loop it replaces: tsvpp_convert_batch(AREA) to the inner size into a temporary -- its weight tables already built --, a fill of the canvases, a strided
           copy of the temporary into them (the fp16 flavour: the fill is a broadcast copy of the per-channel pad, the copy goes through ((x - mean) * scale).to(f16))
      (b0) one iteration of (b) as the FIRST call of a fresh context, which allocates and synchronously copies the tables: wall clock around the call and a stream
           synchronisation, median of `repeats` fresh contexts (not a steady-state figure)
      (c)  the BILINEAR letterbox call on the same geometry (tsvpp_convert_letterbox / tsvpp_convert_letterbox_tensor)
    at three geometries, all from pitch 2048, n = 1, 8, 32, in three flavours."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tensor_util as T
    import time
    O.build()
    L = N.lib()
    vpp = ts.VideoProcessor(device=0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    raw = stream.cuda_stream
    ns = [int(v) for v in a.ns.split(",")]
    lines = [f"# tools/letterbox_ab.py --area: {torch.cuda.get_device_name(0)}, {L.tsvpp_version().decode()}, median of {a.repeats} blocks of {a.iters} iterations, one stream, "
             "frames and canvases rotating through more than 256 MiB each",
             "# (a) = 1 x tsvpp_convert_letterbox_area   (b) = tsvpp_convert_batch(AREA) to the inner size, tables built + fill + strided copy   (b0) = (b) as the first call of a "
             "fresh context (wall clock, builds the tables)   (c) = the BILINEAR letterbox call",
             "# us per call, [min .. max of the blocks]"]
    verdicts = []
    for gname, w, h, pitch, canvas in AREA_GEOS:
        cw, ch = canvas
        nframes = max(a.frames, -(-(280 << 20) // (pitch * h * 3 // 2)))
        nframes = (nframes + 31) // 32 * 32
        gen = torch.Generator(device=dev)
        gen.manual_seed(7)
        base_y = torch.randint(0, 256, (h, pitch), dtype=torch.uint8, device=dev, generator=gen)
        base_uv = torch.randint(0, 256, (h // 2, pitch), dtype=torch.uint8, device=dev, generator=gen)
        ys = [base_y + (37 * k) % 256 for k in range(nframes)]
        uvs = [base_uv + (37 * k) % 256 for k in range(nframes)]
        frames = [N.NV12(ys[k].data_ptr(), uvs[k].data_ptr(), pitch, pitch, w, h) for k in range(nframes)]
        rect = ts.letterbox_rect(w, h, cw, ch)
        left, top, iw, ih = rect
        host = {}  # frame index -> planes on the host

        def planes_of(f):
            if f not in host:
                host[f] = (ys[f].cpu().numpy(), uvs[f].cpu().numpy())
            return host[f]

        for fname, fcc, planes, norm, dtype in AREA_FLAVOURS:
            mk = lambda ww, hh, rt: ts.FrameParameters(width=ww, height=hh, resize_type=rt, pixel_format=fcc, planes_pos=planes, normalization=norm).parameters
            p_area, p_bil, p_inner = mk(cw, ch, 3), mk(cw, ch, 1), mk(iw, ih, 3)
            spec = ts.tensor_spec(dtype=T.TORCH[dtype], mean=IMAGENET[0], std=IMAGENET[1]) if dtype else None
            tdt = T.TORCH[dtype] if dtype else (torch.float32 if norm else torch.uint8)
            esz = T.ESIZE[dtype] if dtype else (4 if norm else 1)
            canvas_bytes = 3 * cw * ch * esz
            d = ts.describe_letterbox_area(ts.FrameParameters(width=cw, height=ch, resize_type=3, pixel_format=fcc, planes_pos=planes, normalization=norm), (w, h, pitch),
                                           **(dict(dtype=tdt, mean=IMAGENET[0], std=IMAGENET[1]) if dtype else {}))
            lines += ["", f"## {gname}, {fname}: inner {iw}x{ih}+{left}+{top}, kernel={d['kernel']} taps={d['taps']} chain={d['chain']} lds={d['lds']}",
                      f"{'n':>3} | {'(a) us':>9} {'spread':>19} | {'(b) us':>9} {'spread':>19} | {'(b0) us':>9} {'spread':>19} | {'(c) us':>9} {'spread':>19} | {'b / a':>6} {'a / c':>6}"]
            pad_q = expected_pad(fcc, planes, norm)
            if dtype:  # the pad after the affine step, per stored channel, exact bits from tensor_util
                pad_bits = T.expected(np.full((3, 1), pad_q, np.float32), 3, IMAGENET, dtype)
                pad_t = torch.from_numpy(pad_bits.view(np.uint16).astype(np.int16)).to(dev).view(torch.float16).view(3, 1, 1)
                t_mean = torch.tensor(list(spec.mean), dtype=torch.float32, device=dev).view(1, 3, 1, 1)
                t_scale = torch.tensor(list(spec.scale), dtype=torch.float32, device=dev).view(1, 3, 1, 1)
            ref_cache = {}

            def reference(f, rt):
                if (f, rt) not in ref_cache:
                    y, uv = planes_of(f)
                    q = expected_geo(y, uv, w, rect, canvas, rt, fcc, planes, norm)
                    ref_cache[(f, rt)] = T.expected(q, 3, IMAGENET, dtype) if dtype else q.ravel().view(np.uint8)
                return ref_cache[(f, rt)]

            for n in ns:
                sets = max(2, (300 << 20) // (n * canvas_bytes) + 1)
                pool = [vpp._alloc(p_area, cw, ch, n, tdt if dtype else None) for _ in range(sets)]
                tmp = vpp._alloc(p_inner, iw, ih, n)
                groups = max(1, nframes // n)
                frame_arrs = [(N.NV12 * n)(*[frames[(g * n + i) % nframes] for i in range(n)]) for g in range(groups)]
                out_arrs = [(ctypes.c_void_p * n)(*[pool[s][i].data_ptr() for i in range(n)]) for s in range(sets)]
                tmp_arr = (ctypes.c_void_p * n)(*[tmp[i].data_ptr() for i in range(n)])
                inner_views = [(t[:, :, top:top + ih, left:left + iw] if planes == 0 else t[:, top:top + ih, left:left + iw, :]) for t in pool]
                pa, pb, pi = ctypes.byref(p_area), ctypes.byref(p_bil), ctypes.byref(p_inner)
                sref = ctypes.byref(spec) if dtype else None

                def leg_a(k, ctx=vpp._ctx):
                    if L.tsvpp_convert_letterbox_area(ctx, n, frame_arrs[k % groups], pa, sref, None, PAD[0], PAD[1], PAD[2], out_arrs[k % sets], raw) != 0:
                        raise RuntimeError("tsvpp_convert_letterbox_area failed")

                def leg_b(k, ctx=vpp._ctx):
                    if L.tsvpp_convert_batch(ctx, n, frame_arrs[k % groups], pi, tmp_arr, raw) != 0:
                        raise RuntimeError("tsvpp_convert_batch failed")
                    if dtype:
                        pool[k % sets].copy_(pad_t.expand_as(pool[k % sets][0]))
                        inner_views[k % sets].copy_(((tmp - t_mean) * t_scale).to(tdt))
                    else:
                        pool[k % sets].fill_(float(pad_q))
                        inner_views[k % sets].copy_(tmp)

                def leg_c(k, ctx=vpp._ctx):
                    if dtype:
                        sts = L.tsvpp_convert_letterbox_tensor(ctx, n, frame_arrs[k % groups], pb, sref, None, PAD[0], PAD[1], PAD[2], out_arrs[k % sets], raw)
                    else:
                        sts = L.tsvpp_convert_letterbox(ctx, n, frame_arrs[k % groups], pb, None, PAD[0], PAD[1], PAD[2], out_arrs[k % sets], raw)
                    if sts != 0:
                        raise RuntimeError("the BILINEAR letterbox call failed")

                def parity(leg, last, rt):
                    got = pool[last % sets]
                    for i in range(n):
                        f = ((last % groups) * n + i) % nframes
                        if not np.array_equal(T.bits(got[i]), reference(f, rt)):
                            raise SystemExit(f"PARITY FAILURE: leg ({leg}) {gname} {fname} n={n} canvas {i}")

                res = {}
                with torch.cuda.stream(stream):
                    for leg, fn, rt in (("a", leg_a, 3), ("b", leg_b, 3), ("c", leg_c, 1)):
                        for t in pool:
                            t.zero_()
                        fn(0)  # parity first, on canvas set 0, then the timing (and parity once more on the last set written)
                        stream.synchronize()
                        parity(leg, 0, rt)
                        blocks, last = timed(fn, stream, a.repeats, a.iters, warm=max(5, a.iters // 2))
                        parity(leg, last, rt)
                        res[leg] = blocks
                    # (b0): the first call of a fresh context
                    b0 = []
                    for _ in range(a.repeats):
                        fresh = ts.VideoProcessor(device=0, max_consumers=1)
                        try:
                            stream.synchronize()
                            t0 = time.perf_counter()
                            leg_b(1, fresh._ctx)
                            stream.synchronize()
                            b0.append((time.perf_counter() - t0) * 1e6)
                        finally:
                            fresh.Close()
                    parity("b0", 1, 3)
                    res["b0"] = b0
                m = {k: statistics.median(v) for k, v in res.items()}
                sp = lambda v: f"{min(v):9.2f}..{max(v):<9.2f}"
                lines.append(f"{n:>3} | " + " | ".join(f"{m[k]:9.2f} {sp(res[k])}" for k in ("a", "b", "b0", "c")) + f" | {m['b'] / m['a']:6.2f} {m['a'] / m['c']:6.2f}")
                print(lines[-1], flush=True)
                if canvas == (640, 640) and w == 1920 and n >= 8:
                    spread = max(res["b"]) - min(res["b"])
                    verdicts.append((m["a"] - m["b"] <= spread, f"{fname}, n = {n}: (a) - (b) = {m['a'] - m['b']:+.2f} us, spread of (b) {spread:.2f} us"))
                del pool, tmp, inner_views
                torch.cuda.empty_cache()
        del ys, uvs, base_y, base_uv
        torch.cuda.empty_cache()
    lines += ["", "# parity: every leg bit-exact against the CPU oracle (fp16: tests/tensor_util.py on the oracle's fp32 canvas) on the first and on the last canvas set it wrote",
              "# condition (1080p -> 640x640: (a) not slower than (b) at n = 8 and n = 32 by more than the spread of (b)'s own blocks):"]
    lines += [f"#   {'met    ' if ok else 'NOT MET'}  {text}" for ok, text in verdicts]
    lines.append(f"# condition as a whole: {'met' if all(ok for ok, _ in verdicts) else 'NOT MET'}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    vpp.Close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--ns", default="1,8,32")
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--dtype", choices=("f32", "f16", "bf16"), default=None, help="the tensor legs (tsvpp_convert_letterbox_tensor); default output profiles/tensor_ab.txt, appended to")
    ap.add_argument("--mean", default="0.485,0.456,0.406", help="per stored channel (with --dtype)")
    ap.add_argument("--std", default="0.229,0.224,0.225", help="per stored channel (with --dtype); the library is handed float32(1) / float32(std)")
    ap.add_argument("--area", action="store_true", help="tsvpp_convert_letterbox_area against the loop it replaces and the BILINEAR call; default output profiles/letterbox_area_ab.txt")
    a = ap.parse_args()
    assert a.repeats >= 1 and a.iters >= 1
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "letterbox_area_ab.txt" if a.area else "tensor_ab.txt" if a.dtype else "letterbox_ab.txt")
    if a.area:
        return area_main(a)
    if a.dtype:
        return tensor_main(a)
    O.build()
    L = N.lib()
    vpp = ts.VideoProcessor(device=0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    raw = stream.cuda_stream
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    base_y = torch.randint(0, 256, (H, PITCH), dtype=torch.uint8, device=dev, generator=gen)
    base_uv = torch.randint(0, 256, (H // 2, PITCH), dtype=torch.uint8, device=dev, generator=gen)
    ys = [base_y + (37 * k) % 256 for k in range(a.frames)]  # distinct frames: every byte + 37 k (mod 256)
    uvs = [base_uv + (37 * k) % 256 for k in range(a.frames)]
    frames = [N.NV12(ys[k].data_ptr(), uvs[k].data_ptr(), PITCH, PITCH, W, H) for k in range(a.frames)]
    rect = ts.letterbox_rect(W, H, CW, CH)
    left, top, iw, ih = rect
    assert rect == (0, 140, 640, 360)
    lines = [f"# tools/letterbox_ab.py: {torch.cuda.get_device_name(0)}, {L.tsvpp_version().decode()}, frame pool {a.frames} x 1080p pitch {PITCH} "
             f"({a.frames * PITCH * H * 3 // 2 >> 20} MiB), median of {a.repeats} blocks of {a.iters} iterations, one stream",
             f"# (loop) = tsvpp_convert_batch to {iw}x{ih} into a temporary + fill of the canvases + strided copy   (fused) = 1 x tsvpp_convert_letterbox   "
             "spread = min .. max of the blocks   roofline = (source planes + canvas) / time / 8 TB/s"]
    ok = True
    for name, rt, fcc, planes, norm in CONFIGS:
        mk = lambda w, h: ts.FrameParameters(width=w, height=h, resize_type=rt, pixel_format=fcc, planes_pos=planes, normalization=norm).parameters
        p_canvas, p_inner = mk(CW, CH), mk(iw, ih)
        esz = 4 if norm else 1
        canvas_bytes = 3 * CW * CH * esz
        moved_frame = W * H * 3 // 2 + canvas_bytes
        pad_value = float(expected_pad(fcc, planes, norm))
        lines += ["", f"## {name}",
                  f"{'n':>3} | {'(loop) us':>10} {'us/frame':>8} {'spread':>17} {'roofline':>8} | {'(fused) us':>10} {'us/frame':>8} {'spread':>17} {'roofline':>8} | {'loop/fused':>10}"]
        for n in [int(v) for v in a.ns.split(",")]:
            sets = max(2, (300 << 20) // (n * canvas_bytes) + 1)
            pool = [vpp._alloc(p_canvas, CW, CH, n) for _ in range(sets)]
            tmp = vpp._alloc(p_inner, iw, ih, n)
            groups = max(1, a.frames // n)  # iteration k converts frames [g n, g n + n), g = k mod groups
            frame_arrs = [(N.NV12 * n)(*[frames[(g * n + i) % a.frames] for i in range(n)]) for g in range(groups)]
            out_arrs = [(ctypes.c_void_p * n)(*[pool[s][i].data_ptr() for i in range(n)]) for s in range(sets)]
            tmp_arr = (ctypes.c_void_p * n)(*[tmp[i].data_ptr() for i in range(n)])
            inner_views = [(t[:, :, top:top + ih, left:left + iw] if planes == 0 else t[:, top:top + ih, left:left + iw, :]) for t in pool]
            ctx, rc, ri = vpp._ctx, ctypes.byref(p_canvas), ctypes.byref(p_inner)
            batch, fused = L.tsvpp_convert_batch, L.tsvpp_convert_letterbox

            def leg_loop(k):
                if batch(ctx, n, frame_arrs[k % groups], ri, tmp_arr, raw) != 0:
                    raise RuntimeError("tsvpp_convert_batch failed")
                pool[k % sets].fill_(pad_value)
                inner_views[k % sets].copy_(tmp)

            def leg_fused(k):
                if fused(ctx, n, frame_arrs[k % groups], rc, None, PAD[0], PAD[1], PAD[2], out_arrs[k % sets], raw) != 0:
                    raise RuntimeError("tsvpp_convert_letterbox failed")

            res = {}
            with torch.cuda.stream(stream):
                for leg, fn in (("loop", leg_loop), ("fused", leg_fused)):
                    for t in pool:
                        t.zero_()
                    torch.cuda.synchronize()
                    blocks, last = timed(fn, stream, a.repeats, a.iters, warm=max(5, a.iters // 2))
                    got = pool[last % sets]
                    for i in range(n):
                        f = ((last % groups) * n + i) % a.frames
                        ref = expected(ys[f].cpu().numpy(), uvs[f].cpu().numpy(), rect, rt, fcc, planes, norm)
                        if not np.array_equal(got[i].contiguous().cpu().numpy().ravel().view(np.uint8), ref):
                            raise SystemExit(f"PARITY FAILURE: leg ({leg}) {name} n={n} canvas {i}")
                    res[leg] = blocks
            ml, mf = statistics.median(res["loop"]), statistics.median(res["fused"])
            cols = []
            for m, blocks in ((ml, res["loop"]), (mf, res["fused"])):
                cols.append(f"{m:10.2f} {m / n:8.2f} {min(blocks):8.2f}..{max(blocks):<7.2f} {n * moved_frame / (m * 1e-6) / HBM:8.4f}")
            lines.append(f"{n:>3} | {cols[0]} | {cols[1]} | {ml / mf:10.2f}")
            print(lines[-1], flush=True)
            if n >= 8 and not mf <= ml:
                ok = False
            del pool, tmp, inner_views
            torch.cuda.empty_cache()
    lines += ["", "# parity: both legs bit-exact against the CPU oracle on the last canvas set of every row",
              f"# condition (the fused call not slower than the loop at n = 8 and n = 32): {'met' if ok else 'NOT MET'}"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    vpp.Close()


def expected_pad(fcc, planes, norm):
    """the pad of PAD in this flavour: one value, because gray's channels are equal"""
    px = O.convert(np.full((2, 2), PAD[0], np.uint8), np.array([[PAD[1], PAD[2]]], np.uint8), fourcc=fcc, planes=planes, normalization=norm)[0]
    assert np.all(px == px[0])
    return px[0]


if __name__ == "__main__":
    main()
