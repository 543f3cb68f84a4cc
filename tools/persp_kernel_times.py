#!/usr/bin/env python3
"""Kernel durations of the legs (a), (a0), (w) of tools/persp_ab.py (fp32, 112 x 112 BGR planar, the same seeded quads), from a kernel trace: what the event-timed
figures of that tool cannot show once the host's planning is longer than the kernel.

    rocprofv3 --output-format csv --kernel-trace -d DIR -o kt -- python tools/persp_kernel_times.py run
    python tools/persp_kernel_times.py parse DIR

`run` issues, per n = 1 / 4 / 16 / 32 and per leg in the order (a), (a0), (w), 100 calls through the Python facade over a rotating pool of 96 frames and > 256 MiB
of outputs; `parse` reads the trace, orders the vpp_persp / vpp_warp dispatches by start time and prints the median, minimum and maximum of each group of 100.
A traced duration includes the tracer's own cost per dispatch (about a microsecond on dispatches this short): compare legs, do not add to other records."""
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tensor-stream_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

NS, LEGS, CALLS, FRAMES = (1, 4, 16, 32), ("a", "a0", "w"), 100, 96


def run():
    import torch
    import persp_ab as A
    import tensor_stream as ts
    dev = torch.device("cuda", 0)
    vpp = ts.VideoProcessor(device=0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    base_y = torch.randint(0, 256, (A.H, A.PITCH), device=dev, generator=gen, dtype=torch.uint8)
    base_uv = torch.randint(0, 256, (A.H // 2, A.PITCH), device=dev, generator=gen, dtype=torch.uint8)
    ys = [base_y + k for k in range(FRAMES)]
    uvs = [base_uv + k for k in range(FRAMES)]
    fp = ts.FrameParameters(width=A.DST[0], height=A.DST[1], resize_type=A.BILINEAR, pixel_format=A.BGR24, planes_pos=A.PLANAR, normalization=True)
    for n in NS:
        hs = A.quads_for(n, seed=200 + n)
        aff = [h[:6] for h in hs]
        hs0 = [m + (0.0, 0.0, 1.0) for m in aff]
        sets = max(2, min(64, (300 << 20) // (n * 3 * A.DST[0] * A.DST[1] * 4) + 1))
        pool = [vpp._alloc(fp.parameters, A.DST[0], A.DST[1], n) for _ in range(sets)]
        for fn, arg in ((vpp.convert_perspective, hs), (vpp.convert_perspective, hs0), (vpp.convert_warp, aff)):
            for k in range(CALLS):
                fn(ys[k % FRAMES], uvs[k % FRAMES], arg, fp, out=pool[k % sets], width=A.W, height=A.H)
            torch.cuda.synchronize()
        del pool
    vpp.Close()


def parse(directory):
    rows = []
    for f in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "vpp_persp" in r["Kernel_Name"] or "vpp_warp" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"].split("(")[0]))
    rows.sort()
    assert len(rows) == len(NS) * len(LEGS) * CALLS, f"{len(rows)} dispatches in the trace, {len(NS) * len(LEGS) * CALLS} expected"
    print(f"# tools/persp_kernel_times.py: kernel durations from a kernel trace, {CALLS} dispatches per row, us")
    for i, (n, leg) in enumerate((n, leg) for n in NS for leg in LEGS):
        g = rows[i * CALLS:(i + 1) * CALLS]
        d = [x[1] / 1e3 for x in g]
        names = sorted({x[2] for x in g})
        assert len(names) == 1 and ("vpp_warp" in names[0]) == (leg == "w"), (n, leg, names)
        print(f"n={n:>2} ({leg:>2})  median {statistics.median(d):6.2f}  min {min(d):6.2f}  max {max(d):6.2f}  {names[0]}")


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 3 and sys.argv[1] == "parse":
        parse(sys.argv[2])
    else:
        sys.exit(__doc__)
