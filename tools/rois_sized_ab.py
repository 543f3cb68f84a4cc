#!/usr/bin/env python3
"""A/B: boxes of a 1080p frame that each go to their OWN output size -- ONE tsvpp_convert_rois_sized call against what the library offered before it -- on one
stream, timed with HIP events, in the protocol of tools/rois_ab.py.

    python tools/rois_sized_ab.py [--out profiles/rois_sized_ab.txt] [--repeats 20] [--iters 50]

Scenarios (BILINEAR; BGR24 planar fp32 and RGB24 merged uint8 each):
  text lines   n = 16 / 48 seeded boxes of 32-640 x 16-96 pixels to height 32 and the width of their aspect (ts.sizes_for_height, multiple 8, at most 640)
                 (s) one tsvpp_convert_rois_sized      (g) one tsvpp_convert_rois per DISTINCT size      (p) one tsvpp_convert_rois of every box to the widest size
                 -- (p) computes and writes the padding its caller throws away; its result is another one, it is checked against the oracle at that size
  pyramid      the whole frame to ts.pyramid_sizes(1920, 1080, 5)[1:]
                 (s) one tsvpp_convert_rois_sized      (c) one tsvpp_convert per level (the fused resize kernels of the flagship path, one launch each)
  cascade      16 faces to 112 x 112, 8 plates to 96 x 32, 8 persons to 128 x 256
                 (s) one tsvpp_convert_rois_sized      (g) one tsvpp_convert_rois per head

Method: per (scenario, leg) a warm-up, then `repeats` timed blocks of `iters` iterations between two events on the stream; the figure is the MEDIAN block, the
spread (min .. max of the blocks) beside it.  Every iteration takes the next frame of a pool of 96 distinct 1080p frames (298 MB) and the next output set of a
pool (up to 64 sets), so neither the 256 MiB last-level cache nor L2 serves a second pass over the same bytes.  Before a number is printed every leg is
parity-checked on the last output set it wrote: bit for bit against the CPU oracle on the box's sliced planes (the two largest pyramid levels: against the other
leg).  All legs go through ctypes with pre-built argument objects: a leg of k calls pays the interpreter's call overhead k times (a C++ caller ~0.5 us less each)."""
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
BILINEAR = 1
CONFIGS = [("BILINEAR BGR24 planar fp32", 2, 0, True), ("BILINEAR RGB24 merged uint8", 1, 1, False)]


def seeded(n, seed, w_range, h_range):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        bw, bh = 2 * int(rng.integers(w_range[0] // 2, w_range[1] // 2 + 1)), 2 * int(rng.integers(h_range[0] // 2, h_range[1] // 2 + 1))
        l, t = int(rng.integers(0, W - bw + 1)), int(rng.integers(0, H - bh + 1))
        out.append((l, t, l + bw, t + bh))
    return out


def scenarios():
    for n in (16, 48):
        boxes = seeded(n, 500 + n, (32, 640), (16, 96))
        yield f"text lines n={n}", boxes, ts.sizes_for_height(boxes, 32, max_width=640, multiple=8), "text"
    sizes = ts.pyramid_sizes(W, H, 5)[1:]
    yield "pyramid 960x540 .. 120x66", [(0, 0, W, H)] * len(sizes), sizes, "pyramid"
    boxes = seeded(16, 601, (64, 400), (64, 400)) + seeded(8, 602, (120, 360), (40, 120)) + seeded(8, 603, (100, 300), (200, 600))
    yield "cascade 16 x 112x112 + 8 x 96x32 + 8 x 128x256", boxes, [(112, 112)] * 16 + [(96, 32)] * 8 + [(128, 256)] * 8, "cascade"


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
        blocks.append(e0.elapsed_time(e1) * 1e3 / iters)  # us per iteration
    return blocks, k - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rois_sized_ab.txt"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--frames", type=int, default=96)
    a = ap.parse_args()
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
    frame_arrs = [(N.NV12 * 1)(frames[k]) for k in range(a.frames)]
    frame_refs = [ctypes.byref(f) for f in frames]
    ctx = vpp._ctx
    lines = [f"# tools/rois_sized_ab.py: {torch.cuda.get_device_name(0)}, {L.tsvpp_version().decode()}, frame pool {a.frames} x 1080p "
             f"({a.frames * W * H * 3 // 2 >> 20} MiB), median of {a.repeats} blocks of {a.iters} iterations, one stream",
             "# (s) = 1 x tsvpp_convert_rois_sized   (g) = 1 x tsvpp_convert_rois per distinct size   (p) = 1 x tsvpp_convert_rois, every box to the widest size   "
             "(c) = 1 x tsvpp_convert per level", "# us per iteration, [min .. max of the blocks]; calls = library calls per iteration; launches from the describe line"]

    for cname, fcc, planes, norm in CONFIGS:
        esz, ch = (4 if norm else 1), 3
        mk = lambda dst=(0, 0): ts.FrameParameters(width=dst[0], height=dst[1], resize_type=BILINEAR, pixel_format=fcc, planes_pos=planes, normalization=norm).parameters
        lines += ["", f"## {cname}", f"{'scenario':<80} {'leg':>4} {'calls':>5} {'us':>9} {'spread':>17} {'vs (s)':>7}"]
        for sname, boxes, sizes, kind in scenarios():
            n = len(boxes)
            nbytes = [ch * w * h * esz for w, h in sizes]
            offs, total = [], 0
            for nb in nbytes:
                offs.append(total)
                total += (nb + 255) // 256 * 256
            widest = (max(w for w, _ in sizes), max(h for _, h in sizes))
            pad_bytes = ch * widest[0] * widest[1] * esz
            pad_stride = (pad_bytes + 255) // 256 * 256
            per_set = max(total, n * pad_stride if kind == "text" else 0)
            sets = max(2, min(64, (300 << 20) // per_set + 1))
            pool = [torch.zeros(per_set, dtype=torch.uint8, device=dev) for _ in range(sets)]
            d = ts.describe_rois_sized(ts.FrameParameters(resize_type=BILINEAR, pixel_format=fcc, planes_pos=planes, normalization=norm), (W, H), boxes, sizes)

            # (s): one call
            recs = (N.RoiSized * n)(*[N.RoiSized(0, *b, *s) for b, s in zip(boxes, sizes)])
            out_s = [(ctypes.c_void_p * n)(*[t.data_ptr() + o for o in offs]) for t in pool]
            p0 = mk()
            r0, f_sized = ctypes.byref(p0), L.tsvpp_convert_rois_sized

            def leg_s(k):
                if f_sized(ctx, 1, frame_arrs[k % a.frames], n, recs, r0, out_s[k % sets], raw) != 0:
                    raise RuntimeError("tsvpp_convert_rois_sized failed")

            legs = [("s", leg_s, 1)]
            # (g): one tsvpp_convert_rois per distinct size, into the same slots
            groups = {}
            for i, s in enumerate(sizes):
                groups.setdefault(s, []).append(i)
            g_args = []
            for s, idx in groups.items():
                pg = mk(s)
                g_args.append((len(idx), (N.Roi * len(idx))(*[N.Roi(0, *boxes[i]) for i in idx]), pg, ctypes.byref(pg),
                               [(ctypes.c_void_p * len(idx))(*[t.data_ptr() + offs[i] for i in idx]) for t in pool]))
            f_rois = L.tsvpp_convert_rois

            def leg_g(k):
                fr = frame_arrs[k % a.frames]
                for cnt, rr, _, pref, outs in g_args:
                    if f_rois(ctx, 1, fr, cnt, rr, pref, outs[k % sets], raw) != 0:
                        raise RuntimeError("tsvpp_convert_rois failed")

            if kind in ("text", "cascade"):
                legs.append(("g", leg_g, len(g_args)))
            if kind == "text":  # (p): everything to the widest size
                pp = mk(widest)
                rp = ctypes.byref(pp)
                recs_p = (N.Roi * n)(*[N.Roi(0, *b) for b in boxes])
                out_p = [(ctypes.c_void_p * n)(*[t.data_ptr() + i * pad_stride for i in range(n)]) for t in pool]

                def leg_p(k):
                    if f_rois(ctx, 1, frame_arrs[k % a.frames], n, recs_p, rp, out_p[k % sets], raw) != 0:
                        raise RuntimeError("tsvpp_convert_rois failed")

                legs.append(("p", leg_p, 1))
            if kind == "pyramid":  # (c): one Convert per level
                c_par = [mk(s) for s in sizes]
                c_refs = [ctypes.byref(c) for c in c_par]
                f_conv = L.tsvpp_convert

                def leg_c(k):
                    t = pool[k % sets].data_ptr()
                    for i in range(n):
                        if f_conv(ctx, frame_refs[k % a.frames], c_refs[i], t + offs[i], raw) != 0:
                            raise RuntimeError("tsvpp_convert failed")

                legs.append(("c", leg_c, n))

            res, bits = {}, {}
            for leg, fn, calls in legs:
                for t in pool:
                    t.zero_()
                torch.cuda.synchronize()
                blocks, last = timed(fn, stream, a.repeats, a.iters, warm=max(10, a.iters // 2))
                res[leg] = (blocks, calls)
                y, uv = ys[last % a.frames].cpu().numpy(), uvs[last % a.frames].cpu().numpy()
                got = pool[last % sets].cpu().numpy()
                for i, ((l, t, r, b), s) in enumerate(zip(boxes, sizes)):
                    dst, off, nb = (widest, i * pad_stride, pad_bytes) if leg == "p" else (s, offs[i], nbytes[i])
                    if kind == "pyramid" and i < 2:
                        continue  # the two largest levels: leg against leg, below
                    ref = O.convert(y[t:b, l:r], uv[t // 2:t // 2 + (b - t) // 2, l:r], dst=dst, resize_type=BILINEAR, fourcc=fcc, planes=planes, normalization=norm, nthreads=8)[0]
                    if not np.array_equal(got[off:off + nb], ref.view(np.uint8).ravel()):
                        raise SystemExit(f"PARITY FAILURE: leg ({leg}) {cname} {sname} box {i} {(l, t, r, b)} -> {dst}")
                fn(0)  # ... and leg against leg on one frame and one output set
                torch.cuda.synchronize()
                bits[leg] = pool[0][:total].cpu().numpy().copy()
            for leg in bits:
                if leg not in ("s", "p") and not np.array_equal(bits[leg], bits["s"]):
                    raise SystemExit(f"PARITY FAILURE: leg ({leg}) against (s) {cname} {sname}")
            ms = statistics.median(res["s"][0])
            for leg, (blocks, calls) in res.items():
                m = statistics.median(blocks)
                label = f"{sname} [{d['sizes']} sizes, {d['launches']} launch{'es' if d['launches'] != 1 else ''}, grid {d['grid']}]" if leg == "s" else ""
                lines.append(f"{label:<80} {'(' + leg + ')':>4} {calls:>5} {m:9.2f} {min(blocks):8.2f}..{max(blocks):<7.2f} {m / ms:7.2f}")
                print(lines[-1], flush=True)
            del pool
            torch.cuda.empty_cache()
    lines += ["", "# parity: every leg bit-exact against the CPU oracle on the last output set it wrote ((p): at the widest size; the 960 x 540 and 480 x 270 pyramid levels: "
              "(c) against (s)), and (g) / (c) against (s) on one frame"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    vpp.Close()


if __name__ == "__main__":
    main()
