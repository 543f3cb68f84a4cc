#!/usr/bin/env python3
"""A/B: n boxes of a 1080p frame to one NN-input size -- (a) n tsvpp_convert calls with crop set (one launch per box: all the library offered
before tsvpp_convert_rois) against (b) ONE tsvpp_convert_rois -- on one stream, timed with HIP events.

    python tools/rois_ab.py [--out profiles/rois_ab.txt] [--repeats 20] [--iters 50] [--ns 1,4,16,32,64]
    python tools/rois_ab.py --area [--out profiles/rois_area_ab.txt]      the AREA leg: tsvpp_convert_rois_area (see area_main)
    python tools/rois_ab.py --dtype f16 [--mean a,b,c] [--std a,b,c]      the tensor legs: tsvpp_convert_rois_tensor (see tensor_main; appends to profiles/tensor_ab.txt)

Method: per (configuration, n, leg) a warm-up, then `repeats` timed blocks of `iters` iterations each between two events on the stream; the figure is the
MEDIAN block, the spread (min .. max of the blocks) is printed beside it.  Every iteration takes the next frame of a pool of 96 distinct 1080p frames
(298 MB) and the next output set of a pool, so that neither the 256 MiB last-level cache nor L2 serves a second pass over the same bytes.  Before a
number is printed both legs are parity-checked against the CPU oracle on the last output set they wrote (every box, bit for bit).
Both legs are driven through ctypes with pre-built argument objects; leg (a) pays the interpreter's call overhead n times per iteration, leg (b) once
(a C++ caller pays ~0.5 us less per call): the per-call cost of (a) is therefore an upper bound, the one of (b) is not.
"bytes" = what a box moves at the least: its output + the source rows and columns it taps (1.5 bytes per box pixel, all of them at these ratios);
"roofline" = bytes / time as a fraction of 8 TB/s."""
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

W, H = 1920, 1080
HBM = 8e12
CONFIGS = [("224x224 BILINEAR BGR24 planar fp32", (224, 224), 1, 2, 0, True),
           ("112x112 BILINEAR RGB24 merged uint8", (112, 112), 1, 1, 1, False)]


def boxes_for(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        bw, bh = 2 * int(rng.integers(32, 257)), 2 * int(rng.integers(32, 257))  # sides 64 .. 512
        l, t = int(rng.integers(0, W - bw)), int(rng.integers(0, H - bh))        # strictly inside: Convert's crop stage accepts every one
        out.append((l, t, l + bw, t + bh))
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


AREA_CONFIGS = [("224x224 AREA BGR24 planar fp32", (224, 224), 2, 0, True),
                ("112x112 AREA RGB24 merged uint8", (112, 112), 1, 1, False)]


def area_main(a):
    """The AREA leg, same protocol (seeded boxes with sides 64 .. 512, one stream, frames and outputs rotating through more than 256 MiB, median of the blocks):
      (roi)  one tsvpp_convert_rois_area call
      (warm) one tsvpp_convert(crop = box, AREA) per box in the context that has already built every box's tables
      (cold) the same loop in a FRESH context per timed block: the first pass pays the table builds (one block of `iters` iterations, so the build cost is spread
             over `iters` passes; the per-box figure of the first pass alone is printed beside it as `first`)
      (bil)  one tsvpp_convert_rois BILINEAR call on the same boxes, for scale.
    (roi) and (warm) are parity-checked against each other and against the CPU oracle on the last output set they wrote."""
    O.build()
    L = N.lib()
    vpp = ts.VideoProcessor(device=0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    raw = stream.cuda_stream
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    base_y = torch.randint(0, 256, (H, W), dtype=torch.uint8, device=dev, generator=gen)
    base_uv = torch.randint(0, 256, (H // 2, W), dtype=torch.uint8, device=dev, generator=gen)
    ys = [base_y + (37 * k) % 256 for k in range(a.frames)]
    uvs = [base_uv + (37 * k) % 256 for k in range(a.frames)]
    frames = [N.NV12(ys[k].data_ptr(), uvs[k].data_ptr(), W, W, W, H) for k in range(a.frames)]
    lines = [f"# tools/rois_ab.py --area: {torch.cuda.get_device_name(0)}, {L.tsvpp_version().decode()}, frame pool {a.frames} x 1080p "
             f"({a.frames * W * H * 3 // 2 >> 20} MiB), median of {a.repeats} blocks of {a.iters} iterations, one stream",
             "# (roi) = 1 x tsvpp_convert_rois_area   (warm) / (cold) = n x tsvpp_convert(crop = box, AREA), tables built / a fresh context per block   "
             "(bil) = 1 x tsvpp_convert_rois BILINEAR", "# us per call, [min .. max of the blocks]; roofline = moved bytes / time / 8 TB/s of (roi); first = us per box of a fresh context's first pass"]
    ok = True
    for name, dst, fcc, planes, norm in AREA_CONFIGS:
        mk = lambda rt, crop=(0, 0, 0, 0): ts.FrameParameters(width=dst[0], height=dst[1], crop_coords=crop, resize_type=rt, pixel_format=fcc, planes_pos=planes,
                                                              normalization=norm).parameters
        p_area, p_bil = mk(3), mk(1)
        out_bytes = 3 * dst[0] * dst[1] * (4 if norm else 1)
        lines += ["", f"## {name}",
                  f"{'n':>3} | {'(roi) us':>9} {'spread':>15} {'roofline':>8} | {'(warm) us':>9} {'spread':>15} | {'(cold) us':>9} {'first/box':>9} | {'(bil) us':>8} | {'warm/roi':>8} {'roi/bil':>7}"]
        for n in [int(v) for v in a.ns.split(",")]:
            boxes = boxes_for(n, seed=100 + n)
            sets = max(2, min(64, (300 << 20) // (n * out_bytes) + 1))
            pool = [vpp._alloc(p_area, dst[0], dst[1], n) for _ in range(sets)]
            moved = sum(out_bytes + (b[2] - b[0]) * (b[3] - b[1]) * 3 // 2 for b in boxes)
            crops = [mk(3, b) for b in boxes]
            crop_refs = [ctypes.byref(c) for c in crops]
            frame_refs = [ctypes.byref(f) for f in frames]
            out_ptrs = [[pool[s][i].data_ptr() for i in range(n)] for s in range(sets)]
            conv = L.tsvpp_convert
            recs = (N.Roi * n)(*[N.Roi(0, *b) for b in boxes])
            out_arrs = [(ctypes.c_void_p * n)(*out_ptrs[s]) for s in range(sets)]
            frame_arrs = [(N.NV12 * 1)(frames[k]) for k in range(a.frames)]
            ra, rb, roi_area, roi_bil = ctypes.byref(p_area), ctypes.byref(p_bil), L.tsvpp_convert_rois_area, L.tsvpp_convert_rois

            def loop_in(ctx):
                def fn(k):
                    fr, ptrs = frame_refs[k % a.frames], out_ptrs[k % sets]
                    for i in range(n):
                        if conv(ctx, fr, crop_refs[i], ptrs[i], raw) != 0:
                            raise RuntimeError("tsvpp_convert failed")
                return fn

            def leg_roi(k):
                if roi_area(vpp._ctx, 1, frame_arrs[k % a.frames], n, recs, ra, out_arrs[k % sets], raw) != 0:
                    raise RuntimeError("tsvpp_convert_rois_area failed")

            def leg_bil(k):
                if roi_bil(vpp._ctx, 1, frame_arrs[k % a.frames], n, recs, rb, out_arrs[k % sets], raw) != 0:
                    raise RuntimeError("tsvpp_convert_rois failed")

            res, last_bits = {}, {}
            for leg, fn in (("roi", leg_roi), ("warm", loop_in(vpp._ctx)), ("bil", leg_bil)):
                for t in pool:
                    t.zero_()
                torch.cuda.synchronize()
                blocks, last = timed(fn, stream, a.repeats, a.iters, warm=max(10, a.iters // 2))
                res[leg] = blocks
                if leg == "bil":
                    continue
                y, uv = ys[last % a.frames].cpu().numpy(), uvs[last % a.frames].cpu().numpy()
                got = pool[last % sets]
                for i, (l, t, r, b) in enumerate(boxes):
                    ref = O.convert(y[t:b, l:r], uv[t // 2:t // 2 + (b - t) // 2, l:r], dst=dst, resize_type=3, fourcc=fcc, planes=planes, normalization=norm, nthreads=8)[0]
                    if not np.array_equal(got[i].contiguous().cpu().numpy().ravel().view(np.uint8), ref.view(np.uint8).ravel()):
                        raise SystemExit(f"PARITY FAILURE: leg ({leg}) {name} n={n} box {i} {(l, t, r, b)}")
                # ... and the two legs against each other, on one frame and one output set
                fn(0)
                torch.cuda.synchronize()
                last_bits[leg] = [pool[0][i].contiguous().cpu().numpy().ravel().view(np.uint8).copy() for i in range(n)]
            if not all(np.array_equal(x, y) for x, y in zip(last_bits["roi"], last_bits["warm"])):
                raise SystemExit(f"PARITY FAILURE: (roi) against (warm) {name} n={n}")
            # cold: a fresh context per block; the block's first pass builds every box's tables
            cold, first = [], []
            for _ in range(min(a.repeats, 5)):
                fresh = ts.VideoProcessor(device=0)
                fn = loop_in(fresh._ctx)
                torch.cuda.synchronize()
                e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                e0.record(stream)
                fn(0)
                e1.record(stream)
                for k in range(1, a.iters):
                    fn(k)
                e2.record(stream)
                e2.synchronize()
                first.append(e0.elapsed_time(e1) * 1e3 / n)
                cold.append(e0.elapsed_time(e2) * 1e3 / a.iters)
                fresh.Close()
            m = {k: statistics.median(v) for k, v in res.items()}
            sp = lambda v: f"{min(v):7.2f}..{max(v):<6.2f}"
            lines.append(f"{n:>3} | {m['roi']:9.2f} {sp(res['roi'])} {moved / (m['roi'] * 1e-6) / HBM:8.4f} | {m['warm']:9.2f} {sp(res['warm'])} | "
                         f"{statistics.median(cold):9.2f} {statistics.median(first):9.2f} | {m['bil']:8.2f} | {m['warm'] / m['roi']:8.2f} {m['roi'] / m['bil']:7.2f}")
            print(lines[-1], flush=True)
            if n >= 16 and not m["roi"] < m["warm"]:
                ok = False
            del pool
            torch.cuda.empty_cache()
    lines += ["", "# parity: (roi) and (warm) bit-exact against the CPU oracle on the last output set of every row, and against each other",
              f"# condition (the ROI call faster than the warm loop at n = 16, 32, 64): {'met' if ok else 'NOT MET'}"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    vpp.Close()


def tensor_main(a):
    """The tensor legs at the first configuration of CONFIGS (seeded 64-512 pixel boxes to 224 x 224 BILINEAR BGR24 planar), same protocol (one stream, frames and
    outputs rotating through more than 256 MiB, median of the blocks with their spread):
      (a) one tsvpp_convert_rois_tensor call with --dtype / --mean / --std: the fused call
      (b) one tsvpp_convert_rois call (fp32) followed by ((x - mean) * scale).to(dtype) in torch on the same stream: what a caller does without (a)
      (c) the tsvpp_convert_rois call of (b) alone: the yardstick
    Every leg is parity-checked, bit for bit, against tests/tensor_util.py on the last output set it wrote.  bytes: source taps (1.5 per box pixel) + the outputs
    a leg writes (+ for (b): the fp32 output read back)."""
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
    base_y = torch.randint(0, 256, (H, W), dtype=torch.uint8, device=dev, generator=gen)
    base_uv = torch.randint(0, 256, (H // 2, W), dtype=torch.uint8, device=dev, generator=gen)
    ys = [base_y + (37 * k) % 256 for k in range(a.frames)]
    uvs = [base_uv + (37 * k) % 256 for k in range(a.frames)]
    frames = [N.NV12(ys[k].data_ptr(), uvs[k].data_ptr(), W, W, W, H) for k in range(a.frames)]
    name, dst, rt, fcc, planes, norm = CONFIGS[0]
    mean, std = [float(v) for v in a.mean.split(",")], [float(v) for v in a.std.split(",")]
    tdt = T.TORCH[a.dtype]
    spec = ts.tensor_spec(dtype=tdt, mean=mean, std=std)
    t_mean = torch.tensor(list(spec.mean), dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    t_scale = torch.tensor(list(spec.scale), dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    p = ts.FrameParameters(width=dst[0], height=dst[1], resize_type=rt, pixel_format=fcc, planes_pos=planes, normalization=norm).parameters
    b32, bel = 3 * dst[0] * dst[1] * 4, 3 * dst[0] * dst[1] * T.ESIZE[a.dtype]
    lines = ["", f"# tools/rois_ab.py --dtype {a.dtype} --mean {a.mean} --std {a.std}: {torch.cuda.get_device_name(0)}, {L.tsvpp_version().decode()}, frame pool "
             f"{a.frames} x 1080p ({a.frames * W * H * 3 // 2 >> 20} MiB), median of {a.repeats} blocks of {a.iters} iterations, one stream",
             f"# {name.replace('fp32', a.dtype)}: (a) = 1 x tsvpp_convert_rois_tensor   (b) = 1 x tsvpp_convert_rois (fp32) + ((x - mean) * scale).to({a.dtype}) in torch   "
             "(c) = the fp32 call of (b) alone", "# us per call, [min .. max of the blocks]; roofline = moved bytes / time / 8 TB/s",
             f"{'n':>3} | {'(a) us':>8} {'spread':>15} {'roofline':>8} | {'(b) us':>8} {'spread':>15} {'roofline':>8} | {'(c) us':>8} {'spread':>15} {'roofline':>8} | {'a / c':>6} {'b / a':>6}"]
    ok = True
    for n in [int(v) for v in a.ns.split(",")]:
        boxes = boxes_for(n, seed=100 + n)
        sets = max(2, min(64, (300 << 20) // (n * b32) + 1))
        sets_el = max(2, min(64, (300 << 20) // (n * bel) + 1))
        pool32 = [vpp._alloc(p, dst[0], dst[1], n) for _ in range(sets)]
        pool_el = [vpp._alloc(p, dst[0], dst[1], n, tdt) for _ in range(sets_el)]
        src = sum((b[2] - b[0]) * (b[3] - b[1]) * 3 // 2 for b in boxes)
        moved = {"a": src + n * bel, "b": src + n * (2 * b32 + bel), "c": src + n * b32}
        recs = (N.Roi * n)(*[N.Roi(0, *b) for b in boxes])
        arr32 = [(ctypes.c_void_p * n)(*[t[i].data_ptr() for i in range(n)]) for t in pool32]
        arr_el = [(ctypes.c_void_p * n)(*[t[i].data_ptr() for i in range(n)]) for t in pool_el]
        frame_arrs = [(N.NV12 * 1)(frames[k]) for k in range(a.frames)]
        ctx, pref, sref, rois, rois_t = vpp._ctx, ctypes.byref(p), ctypes.byref(spec), L.tsvpp_convert_rois, L.tsvpp_convert_rois_tensor
        last_b = [None]

        def leg_a(k):
            if rois_t(ctx, 1, frame_arrs[k % a.frames], n, recs, pref, sref, arr_el[k % sets_el], raw) != 0:
                raise RuntimeError("tsvpp_convert_rois_tensor failed")

        def leg_c(k):
            if rois(ctx, 1, frame_arrs[k % a.frames], n, recs, pref, arr32[k % sets], raw) != 0:
                raise RuntimeError("tsvpp_convert_rois failed")

        def leg_b(k):
            leg_c(k)
            last_b[0] = ((pool32[k % sets] - t_mean) * t_scale).to(tdt)

        res = {}
        with torch.cuda.stream(stream):
            for leg, fn in (("a", leg_a), ("b", leg_b), ("c", leg_c)):
                for t in pool32 + pool_el:
                    t.zero_()
                torch.cuda.synchronize()
                blocks, last = timed(fn, stream, a.repeats, a.iters, warm=max(10, a.iters // 2))
                res[leg] = blocks
                y, uv = ys[last % a.frames].cpu().numpy(), uvs[last % a.frames].cpu().numpy()
                got = {"a": pool_el[last % sets_el], "b": last_b[0], "c": pool32[last % sets]}[leg]
                want_spec, want_dt = ((mean, std), a.dtype) if leg != "c" else (T.IDENTITY, T.F32)
                for i, (l, t, r, b) in enumerate(boxes):
                    q = O.convert(y[t:b, l:r], uv[t // 2:t // 2 + (b - t) // 2, l:r], dst=dst, resize_type=rt, fourcc=fcc, planes=planes, normalization=norm, nthreads=8)[0]
                    if not np.array_equal(T.bits(got[i]), T.expected(q, 3, want_spec, want_dt)):
                        raise SystemExit(f"PARITY FAILURE: leg ({leg}) n={n} box {i} {(l, t, r, b)}")
        m = {k: statistics.median(v) for k, v in res.items()}
        sp = lambda v: f"{min(v):7.2f}..{max(v):<6.2f}"
        lines.append(f"{n:>3} | " + " | ".join(f"{m[k]:8.2f} {sp(res[k])} {moved[k] / (m[k] * 1e-6) / HBM:8.4f}" for k in "abc") + f" | {m['a'] / m['c']:6.2f} {m['b'] / m['a']:6.2f}")
        print(lines[-1], flush=True)
        if n == max(int(v) for v in a.ns.split(",")):
            ok = m["a"] - m["c"] <= max(res["c"]) - min(res["c"])
            tail = f"# expectation at n = {n}: (a) not slower than (c) by more than the spread of (c)'s blocks ({max(res['c']) - min(res['c']):.2f} us): (a) - (c) = {m['a'] - m['c']:+.2f} us: {'met' if ok else 'NOT MET'}"
        del pool32, pool_el
        torch.cuda.empty_cache()
    lines += ["# parity: every leg bit-exact against tests/tensor_util.py (the CPU oracle's fp32 result, the float32 affine step, round to nearest even) on the last output set of every row", tail]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:  # (appends: tools/letterbox_ab.py --dtype fills the same file)
        f.write(text)
    print(text)
    vpp.Close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--area", action="store_true", help="the AREA leg (tsvpp_convert_rois_area); default output profiles/rois_area_ab.txt")
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--ns", default="1,4,16,32,64")
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--dtype", choices=("f32", "f16", "bf16"), default=None, help="the tensor legs (tsvpp_convert_rois_tensor); default output profiles/tensor_ab.txt, appended to")
    ap.add_argument("--mean", default="0.485,0.456,0.406", help="per stored channel (with --dtype)")
    ap.add_argument("--std", default="0.229,0.224,0.225", help="per stored channel (with --dtype); the library is handed float32(1) / float32(std)")
    a = ap.parse_args()
    assert a.repeats >= 1 and a.iters >= 1
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "tensor_ab.txt" if a.dtype else ("rois_area_ab.txt" if a.area else "rois_ab.txt"))
    if a.dtype:
        return tensor_main(a)
    if a.area:
        return area_main(a)
    O.build()
    L = N.lib()
    vpp = ts.VideoProcessor(device=0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    raw = stream.cuda_stream
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    base_y = torch.randint(0, 256, (H, W), dtype=torch.uint8, device=dev, generator=gen)
    base_uv = torch.randint(0, 256, (H // 2, W), dtype=torch.uint8, device=dev, generator=gen)
    ys = [base_y + (37 * k) % 256 for k in range(a.frames)]  # distinct frames: every byte + 37 k (mod 256)
    uvs = [base_uv + (37 * k) % 256 for k in range(a.frames)]
    frames = [N.NV12(ys[k].data_ptr(), uvs[k].data_ptr(), W, W, W, H) for k in range(a.frames)]
    lines = [f"# tools/rois_ab.py: {torch.cuda.get_device_name(0)}, {L.tsvpp_version().decode()}, frame pool {a.frames} x 1080p "
             f"({a.frames * W * H * 3 // 2 >> 20} MiB), median of {a.repeats} blocks of {a.iters} iterations, one stream",
             "# (a) = n x tsvpp_convert(crop = box)   (b) = 1 x tsvpp_convert_rois   spread = min .. max of the blocks   roofline = moved bytes / time / 8 TB/s"]
    for name, dst, rt, fcc, planes, norm in CONFIGS:
        fp = ts.FrameParameters(width=dst[0], height=dst[1], resize_type=rt, pixel_format=fcc, planes_pos=planes, normalization=norm)
        p = fp.parameters
        out_bytes = 3 * dst[0] * dst[1] * (4 if norm else 1)
        lines.append("")
        lines.append(f"## {name}")
        lines.append(f"{'n':>3} | {'(a) us/call':>11} {'us/box':>7} {'spread':>15} {'roofline':>8} | {'(b) us/call':>11} {'us/box':>7} {'spread':>15} {'roofline':>8} | {'a / b':>6}")
        for n in [int(v) for v in a.ns.split(",")]:
            boxes = boxes_for(n, seed=100 + n)
            sets = max(2, min(64, (300 << 20) // (n * out_bytes) + 1))
            pool = [vpp._alloc(p, dst[0], dst[1], n) for _ in range(sets)]
            moved = sum(out_bytes + (b[2] - b[0]) * (b[3] - b[1]) * 3 // 2 for b in boxes)
            # leg (a): one parameter block per box (crop = the box), one call per box
            crops = [ts.FrameParameters(width=dst[0], height=dst[1], crop_coords=b, resize_type=rt, pixel_format=fcc, planes_pos=planes,
                                        normalization=norm).parameters for b in boxes]
            crop_refs = [ctypes.byref(c) for c in crops]
            frame_refs = [ctypes.byref(f) for f in frames]
            out_ptrs = [[pool[s][i].data_ptr() for i in range(n)] for s in range(sets)]
            ctx, conv = vpp._ctx, L.tsvpp_convert

            def leg_a(k):
                fr, ptrs = frame_refs[k % a.frames], out_ptrs[k % sets]
                for i in range(n):
                    if conv(ctx, fr, crop_refs[i], ptrs[i], raw) != 0:
                        raise RuntimeError("tsvpp_convert failed")

            # leg (b): one call
            recs = (N.Roi * n)(*[N.Roi(0, *b) for b in boxes])
            out_arrs = [(ctypes.c_void_p * n)(*out_ptrs[s]) for s in range(sets)]
            frame_arrs = [(N.NV12 * 1)(frames[k]) for k in range(a.frames)]
            pref, rois = ctypes.byref(p), L.tsvpp_convert_rois

            def leg_b(k):
                if rois(ctx, 1, frame_arrs[k % a.frames], n, recs, pref, out_arrs[k % sets], raw) != 0:
                    raise RuntimeError("tsvpp_convert_rois failed")

            res = {}
            for leg, fn in (("a", leg_a), ("b", leg_b)):
                for t in pool:
                    t.zero_()
                torch.cuda.synchronize()
                blocks, last = timed(fn, stream, a.repeats, a.iters, warm=max(10, a.iters // 2))
                # parity of the last output set this leg wrote, every box, against the oracle on the sliced planes
                y, uv = ys[last % a.frames].cpu().numpy(), uvs[last % a.frames].cpu().numpy()
                got = pool[last % sets]
                for i, (l, t, r, b) in enumerate(boxes):
                    ref = O.convert(y[t:b, l:r], uv[t // 2:t // 2 + (b - t) // 2, l:r], dst=dst, resize_type=rt, fourcc=fcc, planes=planes, normalization=norm,
                                    nthreads=8)[0]
                    if not np.array_equal(got[i].contiguous().cpu().numpy().ravel().view(np.uint8), ref.view(np.uint8).ravel()):
                        raise SystemExit(f"PARITY FAILURE: leg ({leg}) {name} n={n} box {i} {(l, t, r, b)}")
                res[leg] = blocks
            ma, mb = statistics.median(res["a"]), statistics.median(res["b"])
            cols = []
            for m, blocks in ((ma, res["a"]), (mb, res["b"])):
                cols.append(f"{m:11.2f} {m / n:7.2f} {min(blocks):7.2f}..{max(blocks):<6.2f} {moved / (m * 1e-6) / HBM:8.4f}")
            lines.append(f"{n:>3} | {cols[0]} | {cols[1]} | {ma / mb:6.2f}")
            print(lines[-1], flush=True)
            del pool
            torch.cuda.empty_cache()
    lines.append("")
    lines.append("# parity: both legs bit-exact against the CPU oracle on the last output set of every row")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    vpp.Close()


if __name__ == "__main__":
    main()
