#!/usr/bin/env python3
"""bench.py -- throughput of the fused VPP hot path on MI355X.

A "step" is one pass of the hot path over one batch of synthetic NV12 frames: ONE launch of the fused
crop+resize+colour kernel converting `--batch` (default 64) independent frames
(tsvpp_convert_batch).  Default workload = BASELINE.json's metric: 1920x1080 NV12 -> 1280x720
BILINEAR -> BGR24 PLANAR fp32 (normalised).  Inputs are resident in HBM before the timed region;
the batch rotates over enough buffer sets that the working set is > 512 MiB (Infinity Cache is 256 MiB).

Timing: W warm-up steps plus a TIME-BASED warm-up (untimed steps until the device has worked for
`--warmup-ms`, default 40 ms: it needs ~25 ms of continuous work to settle its clocks), then the timed region of
EXACTLY K steps -- barrier + torch.cuda.synchronize() on both sides, HIP events on the launch stream inside.  A plain
run times that region once (`ms_per_step` = its wall / K).  With `--full` it is run `--repeats` times back to back
(default max(5, ceil(400 / K)): at least 200 timed iterations) and the MEDIAN region is reported (`ms_per_step` =
median wall / K; every repeat is listed in `timing.repeats_ms_per_step`, with `timing.total_timed_steps` and the mean
over all of them).  Max over ranks per repeat.

`--dump-outputs DIR` writes what the last timed step computed (output_arrays: float32, at most 64 MiB) after the timed
region.  The inputs are drawn from fixed seeds and the last timed step always converts buffer set 0, so two builds run
with the same arguments can be compared output for output.

Prints ONE JSON line (rank 0).  N>1: one rank per GPU, launched either by torch.distributed.run (RANK /
WORLD_SIZE in the environment) or by this script itself when `--gpus N` is given without such an environment
(it re-executes itself under torch.distributed.run); frames shard by rank with no data-path collective (weak
scaling); the only collective is a one-off RCCL broadcast of the 8 colour coefficients, verified against the
compiled-in defaults.  With fewer than N GPUs visible it prints a "not measured" line instead of extrapolating.

A plain run does nothing else: set-up, warm-up, the timed steps, the dump, the line.  Besides the timed region a `--full` line carries (world 1): the headline's other resize types and every BASELINE configuration (`config.other_workloads`), the facade leg, the
single-frame latency leg and -- round 6 -- `config.launch_curve`: the headline, C3 and C4 at 1 .. 64 frames per launch (tensor-stream_amd/cpp/vpp_curve.cpp, its own process), the reference's
real calling pattern.  `--workload c5 --consumers 64` makes the step ONE read_many over this rank's share of 64 named consumers of a TensorStreamConverter (C5 as BASELINE words it).

The oracle (oracle/) is touched only as the checker: the parity gate (--full, AFTER the timed region, on frames 0 / 31 / 63 of the
buffer set the last timed step wrote -- the timed launch is the checked launch), `touched_bytes`,
and the `cpu_baseline` leg (--full).  A failure in a side leg (cpu_baseline, other_resize_types, traffic lookup) is
recorded as {"error": ...} inside the line and can never swallow it.
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "tensor-stream_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np

MAX_LAUNCH = 128      # frames per launch (include/tsvpp.h: TSVPP_MAX_BATCH)
MAX_TABLE_LAUNCH = 1024  # ... out of a persistent device-resident frame table (TSVPP_MAX_TABLE_LAUNCH; --table)
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)
METRIC = "1080p NV12→720p BGR24 planar fp32 frames/sec per GPU; achieved HBM GB/s vs roofline"

WORKLOADS = {
    # name: (src_w, src_h, pitch, crop, dst, resize, fourcc, planes, norm)
    "headline": (1920, 1080, 2048, (0, 0, 0, 0), (1280, 720), "BILINEAR", "BGR24", "PLANAR", True),
    # C1 (BASELINE.json configs[0]): the conversion the reference's CPU plumbing case names -- bunny.mp4's 1280x720 NV12 -> RGB24 MERGED uint8 at native size -- on the GPU
    # path, with the CPU oracle beside it (cpu_baseline; swscale itself does not exist in this image).  Frames are synthetic like every bench workload; the real
    # picture of the clip is a parity fixture (tests/test_gpu_bunny.py).
    "c1": (1280, 720, 1280, (0, 0, 0, 0), (0, 0), "NEAREST", "RGB24", "MERGED", False),
    "c2": (1920, 1080, 2048, (0, 0, 0, 0), (0, 0), "NEAREST", "BGR24", "PLANAR", True),
    "c3": (1920, 1080, 2048, (0, 0, 1280, 720), (256, 256), "BILINEAR", "RGB24", "PLANAR", True),
    "c4": (3840, 2160, 3840, (0, 0, 0, 0), (1280, 720), "BICUBIC", "BGR24", "MERGED", False),
    "c5": (3840, 2160, 3840, (0, 0, 0, 0), (640, 360), "AREA", "BGR24", "PLANAR", True),
}
# frames per step and "out of a persistent frame table" when --batch is not given.  C3 moves 1.8 MB per frame and C4 6.9 MB: their 64-frame launches (113 / 442 MB) run at
# 0.64 / 0.64 of the roofline on moved bytes, 0.72 / 0.67 from 512 / 256 frames on (profiles/r05_table_ab.txt, r05_c4_shapes.txt); the headline and the other
# configurations gain nothing (or lose: 1024-frame launches of the headline 0.775 -> 0.711) and keep 64
# C1's frames are small too (4.1 MB): 128 frames per launch -- still the kernarg path -- 0.68 -> 0.73 (profiles/r05_c1_batch.txt); a table adds nothing beyond that
DEFAULT_BATCH = {"c1": (128, False), "c3": (512, True), "c4": (256, True)}
RESIZE = {"NEAREST": 0, "BILINEAR": 1, "BICUBIC": 2, "AREA": 3}
FOURCC = {"Y800": 0, "RGB24": 1, "BGR24": 2, "NV12": 3, "UYVY": 4, "YUV444": 5, "HSV": 6}
PLANES = {"PLANAR": 0, "MERGED": 1}
# sources whose hash stamps a PMC traffic entry (tools/traffic_json.py writes it, lookup_traffic checks it)
KERNEL_SOURCES = ["tensor-stream_amd/csrc/vpp_kernels.hip", "tensor-stream_amd/csrc/vpp_select.hip", "tensor-stream_amd/csrc/vpp_bicubic_r32.hip", "tensor-stream_amd/csrc/vpp_bicubic_r32_core.h", "tensor-stream_amd/csrc/vpp_r32_store.h", "tensor-stream_amd/csrc/vpp_device.h", "tensor-stream_amd/csrc/vpp_bicubic_int.hip", "tensor-stream_amd/csrc/vpp_bilinear.hip", "tensor-stream_amd/csrc/vpp_bilinear_r32.hip",
                  "tensor-stream_amd/csrc/vpp_area_box.hip", "tensor-stream_amd/csrc/vpp_area_stream.hip", "tensor-stream_amd/csrc/vpp_bicubic_cols.hip", "tensor-stream_amd/csrc/vpp_kernels.h", "tensor-stream_amd/csrc/vpp_axis.h",
                  "tensor-stream_amd/csrc/vpp_formats.hip", "tensor-stream_amd/csrc/tsvpp_api.cpp", "tensor-stream_amd/csrc/vpp_bilinear_rows.hip", "tensor-stream_amd/csrc/vpp_point_rn.hip"]


def roi_and_dst(src_w, src_h, crop, dst):
    """Stage selection of VideoProcessor::Convert (reference src/VideoProcessor.cpp:106-135): ROI and output size."""
    cw, ch = crop[2] - crop[0], crop[3] - crop[1]
    roi_w, roi_h = (cw, ch) if (0 < cw < src_w and 0 < ch < src_h) else (src_w, src_h)
    dw, dh = dst if (dst[0] and dst[1]) else (roi_w, roi_h)
    return roi_w, roi_h, dw, dh


def algorithmic_bytes(src_w, src_h, crop, dst, norm, channels=3.0, luma_only=False):
    """ROI_w*ROI_h*3/2 + dst_w*dst_h*channels*sizeof(T) (Y800 does not read the chroma plane)."""
    roi_w, roi_h, dw, dh = roi_and_dst(src_w, src_h, crop, dst)
    return roi_w * roi_h * (2 if luma_only else 3) // 2 + int(dw * dh * channels) * (4 if norm else 1)


def _axis_taps(mode, n_out, n_src, ratio, chroma, area_pattern):
    """Set of source indices (luma samples, or chroma PAIR columns / chroma rows) that the outputs 0..n_out-1 of
    one axis tap with a NON-ZERO weight, from the reference's coordinate formulas in fp32 (src/Resize.cu:242-357,
    160-240; the chroma grid reuses the luma formulas on its own indices).  Only used for the reported
    `touched_bytes`, never for results."""
    f32 = np.float32
    o = np.arange(n_out, dtype=np.float32)
    r = f32(ratio)
    lim = n_src
    taps = []
    if mode == "NONE":
        return np.arange(n_out)
    if mode == "NEAREST":
        taps.append((r * o).astype(np.int64))
    elif mode in ("BILINEAR", "BICUBIC"):
        xf = (o + f32(0.5)) * r - f32(0.5)
        x = np.floor(xf).astype(np.int64)
        w = xf - x.astype(np.float32)
        w = np.where((x < 0) | (x > lim - 1), f32(0), w)
        x = np.clip(x, 0, lim - 1)
        taps.append(x)
        nz = w != 0
        taps.append(x[nz] + 1)
        if mode == "BICUBIC":  # Keys a=-0.75: c0 and c3 vanish only at w == 0
            taps.append(x[nz] - 1)
            taps.append(x[nz] + 2)
    elif mode == "AREA_DOWN":
        x = (r * o).astype(np.int64)
        pat = area_pattern(float(r))
        need = int(np.ceil(float(r)))
        rows = pat[np.arange(n_out) % pat.shape[0], :need]
        for b in range(need):
            taps.append(x[rows[:, b] != 0] + b)
    else:  # AREA_UP, src/Resize.cu:214-240
        x = np.floor(r * o).astype(np.int64)
        fx = (o + f32(1)) - (x + 1).astype(np.float32) / r
        fx = np.where(fx <= 0, f32(0), fx - np.floor(fx))
        taps.append(x)
        taps.append(x[fx != 0] + 1)
    t = np.unique(np.concatenate(taps))
    hi = (n_src // 2 if chroma else n_src) - 1
    return t[(t >= 0) & (t <= hi)]


def touched_bytes(spec):
    """distinct source bytes with a non-zero weight + the output bytes.  Every (row, column)
    combination of the per-axis tap sets is touched, so the count is a product per plane."""
    from oracle import oracle as O
    src_w, src_h, _pitch, crop, dst, rt, fcc, _planes, norm = spec
    roi_w, roi_h, dw, dh = roi_and_dst(src_w, src_h, crop, dst)
    chans = {0: 1.0, 3: 1.5, 4: 2.0}.get(FOURCC[fcc], 3.0)
    out_bytes = int(dw * dh * chans) * (4 if (norm or fcc == "HSV") else 1)
    if (dw, dh) == (roi_w, roi_h):
        mode = "NONE"
    elif rt == "AREA":
        mode = "AREA_DOWN" if (np.float32(roi_w) / np.float32(dw) > 1 and np.float32(roi_h) / np.float32(dh) > 1) else "AREA_UP"
    else:
        mode = rt
    xr, yr = np.float32(roi_w) / np.float32(dw), np.float32(roi_h) / np.float32(dh)
    cols = _axis_taps(mode, dw, roi_w, xr, False, O.area_pattern)
    rows = _axis_taps(mode, dh, roi_h, yr, False, O.area_pattern)
    n = len(cols) * len(rows)
    if fcc != "Y800":
        ccols = _axis_taps(mode, dw // 2, roi_w, xr, True, O.area_pattern)
        crows = _axis_taps(mode, dh // 2, roi_h, yr, True, O.area_pattern)
        n += 2 * len(ccols) * len(crows)
    return int(n) + out_bytes


def cpu_baseline(spec, budget_s=12.0, tight_pitch=False):
    """The CPU oracle (same arithmetic, bit-comparable with the GPU output) on all host cores:
    one frame per thread (frames are independent, exactly as they shard across GPUs), bounded sample."""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import oracle as O
    src_w, src_h, pitch, crop, dst, rt, fcc, planes, norm = spec
    if tight_pitch:
        pitch = src_w
    cores = O.host_cores()
    rng = np.random.default_rng(1)
    y = rng.integers(0, 256, (src_h, pitch), dtype=np.uint8)
    uv = rng.integers(0, 256, (src_h // 2, pitch), dtype=np.uint8)
    kw = dict(crop=crop, dst=dst, resize_type=RESIZE[rt], fourcc=FOURCC[fcc], planes=PLANES[planes],
              normalization=norm, nthreads=1, width=src_w)
    t1 = time.perf_counter()
    O.convert(y, uv, **kw)  # warm-up + single-core time per frame
    per_frame = time.perf_counter() - t1
    deadline = time.perf_counter() + budget_s

    def work(_):
        k = 0
        while True:
            O.convert(y, uv, **kw)  # ctypes releases the GIL during the call
            k += 1
            if time.perf_counter() > deadline:
                return k

    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=cores) as ex:
        n = sum(ex.map(work, range(cores)))
    el = time.perf_counter() - t0
    return {"value": round(n / el, 2), "unit": "frames/s", "cores": cores, "kind": "port",
            "sample": f"{n} frames of the same workload in {el:.1f} s: oracle/vpp_oracle.c, {cores} threads, "
                      f"1 frame per thread ({per_frame * 1e3:.1f} ms per frame on one idle core)",
            # the reference itself never calls sws_* and no libswscale exists in this image
            "swscale": "unavailable in image"}


def facade_leg(dev, n_consumers=64, calls=60, windows=5, warm=150, pool=64):
    """The production entry (TensorStreamConverter, reference tensor_stream/tensor_stream.py:248-291) at BASELINE config C5's shape:
    `n_consumers` consumers of ONE converter on a synthetic 4K source, served by read_many() -- one hand-off and ONE batched launch
    per published frame, every consumer its own tensor.  Outside the timed region; wall-clock rate including the Python host side.

    The source cycles through `pool` DISTINCT 4K frames (64 x 12.4 MB = 796 MB, three times the 256 MiB Infinity Cache), so the frame a call
    converts comes from HBM; its 64 consumers then share it (that IS C5's shape: 64 consumers of one stream) -- 63 of the 64 source reads of a call
    are cache hits.  `hbm_frac` therefore prices the bytes that really move per call (one source frame + 64 outputs); the ROI-formula figure
    (64 x 15.2 MB per call) is reported as `alg_frac` and says how well the host side keeps the GPU fed, not what the HBM does.
    The measured windows run with the cyclic garbage collector frozen and disabled (a full collection is ~40 ms: at ~650 calls per collection it
    used to land in one window of five); every window is listed."""
    import gc
    import torch
    import tensor_stream as ts
    spec = WORKLOADS["c5"]
    r = ts.TensorStreamConverter(f"synthetic://{spec[0]}x{spec[1]}?seed=3&frames=0&fps=100000&pool={pool}", max_consumers=n_consumers, cuda_device=dev,
                                 framerate_mode=ts.FrameRate.FAST)
    r.initialize()
    r.start()
    names = [f"consumer{i}" for i in range(n_consumers)]
    kw = dict(width=spec[4][0], height=spec[4][1], resize_type=RESIZE[spec[5]], pixel_format=FOURCC[spec[6]], planes_pos=PLANES[spec[7]], normalization=spec[8])
    dts = []
    gc_was = gc.isenabled()
    try:
        for _ in range(warm):
            r.read_many(names, **kw)
        torch.cuda.synchronize()
        gc.collect()
        gc.freeze()
        gc.disable()
        for _ in range(windows):
            t0 = time.perf_counter()
            for _ in range(calls):
                r.read_many(names, **kw)
            torch.cuda.synchronize()
            dts.append(time.perf_counter() - t0)
    finally:
        if gc_was:
            gc.enable()
        gc.unfreeze()
        r.stop()
    bpf = algorithmic_bytes(spec[0], spec[1], spec[3], spec[4], spec[8])
    src_bytes = spec[0] * spec[1] * 3 // 2
    moved_per_call = src_bytes + n_consumers * (bpf - src_bytes)  # one source frame from HBM + every consumer's output
    alg = lambda dt: round(n_consumers * calls / dt * bpf / 1e9 / HBM_PEAK_GBS, 4)
    moved = lambda dt: round(calls / dt * moved_per_call / 1e9 / HBM_PEAK_GBS, 4)
    dt = sorted(dts)[len(dts) // 2]
    rate = n_consumers * calls / dt
    return {"entry": "TensorStreamConverter.read_many", "workload": "c5", "consumers": n_consumers, "distinct_source_frames": pool,
            "source_pool_MiB": round(pool * src_bytes / 2**20, 1), "conversions_per_s": round(rate, 1),
            "hbm_frac": moved(dt), "alg_frac": alg(dt), "ms_per_call": round(dt * 1e3 / calls, 4), "windows_alg_frac": [alg(x) for x in dts],
            "note": f"one batched launch per published frame; wall clock incl. the Python host side; median of {windows} windows of {calls} calls after {warm} warm-up "
                    "calls, garbage collector frozen; hbm_frac = (one source frame + 64 outputs) per call: the 64 consumers of a call share their source frame"}


def latency_leg(spec, iters=2000):
    """Single-frame latency of VideoProcessor::Convert through the C++ class (tensor-stream_amd/cpp/vpp_latency.cpp): the only quantity the
    reference publishes is a latency (getFrame 3 +- 3 ms, tests/src/WrapperTests.cpp:303-309).  Its own process, after the timed region."""
    exe = os.path.join(ROOT, "tensor-stream_amd", "lib", "vpp_latency")
    if not os.path.isfile(exe):
        return {"error": "tensor-stream_amd/lib/vpp_latency is not built (make -C tensor-stream_amd/cpp)"}
    src_w, src_h, _pitch, _crop, dst, rt, fcc, planes, norm = spec
    cmd = [exe, str(src_w), str(src_h), str(dst[0]), str(dst[1]), str(RESIZE[rt]), str(FOURCC[fcc]), str(PLANES[planes]), "1" if norm else "0", str(iters)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    if p.returncode != 0 or not lines:
        return {"error": f"vpp_latency exited {p.returncode}: {p.stderr[-200:]}"}
    return json.loads(lines[-1])


def curve_frame(frame_id, pitch, src_h):
    """Pool frame `frame_id` of tensor-stream_amd/cpp/vpp_curve.cpp, regenerated on the host: byte i of plane p = lowbias32(i + id * 0x9E3779B1 + p * 0x85EBCA6B) >> 24."""
    def plane(n, pl):
        x = np.arange(n, dtype=np.uint32) + np.uint32((frame_id * 0x9E3779B1 + pl * 0x85EBCA6B) & 0xFFFFFFFF)
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
        return (x >> np.uint32(24)).astype(np.uint8)
    return plane(pitch * src_h, 0).reshape(src_h, pitch), plane(pitch * src_h // 2, 1).reshape(src_h // 2, pitch)


CURVE_NS = (1, 2, 4, 8, 16, 32, 64)
# consumer shapes of the launch curve: threads x streams per thread (vpp_curve.cpp) -> key in the line
CURVE_MODES = (("1xc", "one_consumer"), ("4xc", "four_consumers"))  # "c": through the context's consumer pool (tsvpp_consumer_next_stream), as VideoProcessor::ConvertInto


def launch_curve_leg(names=("headline", "c3", "c4"), ns=CURVE_NS, modes=CURVE_MODES, target_ms=30.0, inputs_ready=(0, 1), parity=True):
    """the hot path at the launch sizes the reference's calling pattern produces -- ONE frame per Convert (reference
    src/Wrappers/WrapperPython.cpp:265-363) out of a ring of 5-10 frames (include/Decoder.h:19) -- i.e. 1 .. 64 frames per launch, on rotating pools whose moved bytes
    exceed 640 MiB per issuing thread (tensor-stream_amd/cpp/vpp_curve.cpp, its own process, after the timed region).  Per workload and n:
      one_consumer     one named consumer of the context, every launch on its stream (tsvpp_consumer_next_stream, as VideoProcessor::ConvertInto), back to back:
                       the dependent-launch boundary is inside the figure;
      four_consumers   four host threads, each a named consumer with its own stream (the reference's model: one stream per consumer name);
      *_inputs_ready   the same with TSVPP_OPT_INPUTS_READY (include/tsvpp.h): a consumer alternates between two streams and its launches do not wait for their
                       predecessors -- legal for the reference's hand-off (the decoder has finished the frame before getFrame returns it).
    Wall clock from a common start until every stream is synchronised, median of five regions of ~30 ms.
    `frac` = moved bytes per launch / time per launch / 8 TB/s; moved bytes = the ROI formula, or for the sparse samplers (C3, C4) the PMC traffic per frame of the
    profiled launch when that entry is fresh, else the touched bytes (a lower bound).  Every point is checked against the oracle: CRC-32 of the first and the last
    output frame of the last launch (the pool's outputs are overwritten before every point)."""
    import zlib
    exe = os.path.join(ROOT, "tensor-stream_amd", "lib", "vpp_curve")
    if not os.path.isfile(exe):
        return {"error": "tensor-stream_amd/lib/vpp_curve is not built (make -C tensor-stream_amd/cpp)"}
    from oracle import oracle as O
    res = {"n": list(ns), "driver": "tensor-stream_amd/cpp/vpp_curve.cpp", "pool": "> 640 MiB of moved bytes per issuing thread, rotating"}
    for name in names:
        spec = WORKLOADS[name]
        src_w, src_h, pitch, crop, dst, rt, fcc, planes, norm = spec
        bpf = algorithmic_bytes(src_w, src_h, crop, dst, norm)
        wbs = bpf - roi_and_dst(src_w, src_h, crop, dst)[0] * roi_and_dst(src_w, src_h, crop, dst)[1] * 3 // 2
        moved, basis = bpf, "algorithmic bytes (ROI formula)"
        tbs = touched_bytes(spec)
        if tbs < 0.9 * bpf:
            moved, basis = tbs, "touched bytes (sparse sampler: a lower bound of the bytes moved)"
            try:
                fpl = float(DEFAULT_BATCH.get(name, (64, False))[0])
                tr, _why = lookup_traffic(name, fpl, alg_read=(bpf - wbs) * fpl, alg_write=wbs * fpl, touched_read=(tbs - wbs) * fpl)
                if tr:
                    moved, basis = tr / fpl, "PMC traffic per frame of the profiled %d-frame launch" % int(fpl)
            except Exception:  # noqa: BLE001
                pass
        entry = {"workload": name, "moved_bytes_per_frame": int(moved), "basis": basis}
        bad = []
        for ready in inputs_ready:
            cmd = [exe, str(src_w), str(src_h), str(pitch), *(str(c) for c in crop), str(dst[0]), str(dst[1]), str(RESIZE[rt]), str(FOURCC[fcc]), str(PLANES[planes]),
                   "1" if norm else "0", str(int(moved)), ",".join(str(n) for n in ns), ",".join(m for m, _ in modes), str(target_ms), str(ready)]
            pr = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            lines = [l for l in pr.stdout.splitlines() if l.startswith("{")]
            if pr.returncode != 0 or not lines:
                entry["error"] = f"vpp_curve exited {pr.returncode}: {pr.stderr[-300:]}"
                break
            out = json.loads(lines[-1])
            entry["pool_frames_per_thread"] = out["pool_frames_per_thread"]
            for mode, key in modes:
                t, st = mode.split("x")
                pts = [q for q in out["points"] if q["threads"] == int(t) and ((st == "c" and q.get("consumer_pool")) or (st != "c" and not q.get("consumer_pool") and q["streams_per_thread"] == int(st)))]
                pts.sort(key=lambda q: q["n"])
                k = key + ("_inputs_ready" if ready else "")
                entry[k] = {"us_per_launch": [round(q["us_per_launch"], 3) for q in pts],
                            "frac": [round(moved * q["n"] / (q["us_per_launch"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4) for q in pts],
                            "frames_per_s": [round(q["n"] / (q["us_per_launch"] * 1e-6), 1) for q in pts],
                            "host_issue_us_per_launch": [round(q["host_issue_us_per_launch"], 2) for q in pts], "timer": pts[0]["timer"] if pts else None}
                if parity:
                    for q in pts:
                        for c in q["check"]:
                            y, uv = curve_frame(c["frame"], pitch, src_h)
                            ref, _, _ = O.convert(y, uv, crop=crop, dst=dst, resize_type=RESIZE[rt], fourcc=FOURCC[fcc], planes=PLANES[planes], normalization=norm,
                                                  nthreads=min(16, O.host_cores()), width=src_w)
                            if (zlib.crc32(ref.tobytes()) & 0xFFFFFFFF) != c["crc32"]:
                                bad.append(f"{k} n={q['n']} frame {c['frame']}")
        if "error" not in entry:
            entry["parity"] = ("not checked" if not parity else ("MISMATCH vs oracle: " + ", ".join(bad[:6])) if bad else
                               "bit-exact vs oracle (CRC-32 of the first and last output frame of the last launch, every point)")
            if bad:
                for _mode, key in modes:  # a fast wrong kernel is not a measurement
                    for ready in inputs_ready:
                        entry.pop(key + ("_inputs_ready" if ready else ""), None)
        res[name] = entry
    return res


_SHARED_SOURCES = ["tensor-stream_amd/csrc/vpp_device.h", "tensor-stream_amd/csrc/vpp_kernels.h", "tensor-stream_amd/csrc/vpp_axis.h"]
_KERNEL_FILES = [("vpp_bilinear_r32", "vpp_bilinear_r32.hip"), ("vpp_bilinear_up2", "vpp_bilinear_up2.hip"), ("vpp_bilinear_rows", "vpp_bilinear_rows.hip"), ("vpp_point_rn", "vpp_point_rn.hip"),
                 ("vpp_bilinear", "vpp_bilinear.hip"), ("vpp_bicubic_r32", "vpp_bicubic_r32.hip"), ("vpp_bicubic_int", "vpp_bicubic_int.hip"),
                 ("vpp_bicubic_cols", "vpp_bicubic_cols.hip"), ("vpp_area_box", "vpp_area_box.hip"), ("vpp_area_stream", "vpp_area_stream.hip"),
                 ("fmt_", "vpp_formats.hip")]


def kernel_source_files(kernel=None):
    """The sources a PMC traffic entry depends on: the dispatched kernel's translation unit + the shared device headers (kernel =
    the name bench.py prints in roofline.kernel); without a kernel name: every kernel source."""
    if not kernel:
        return list(KERNEL_SOURCES)
    k = kernel.split("::")[-1]
    unit = next((f for prefix, f in _KERNEL_FILES if k.startswith(prefix)), "vpp_kernels.hip")
    extra = {"vpp_bicubic_r32.hip": ["vpp_bicubic_r32_core.h", "vpp_r32_store.h"], "vpp_bilinear_r32.hip": ["vpp_r32_store.h"], "vpp_point_rn.hip": ["vpp_r32_store.h"],
             "vpp_bilinear_up2.hip": ["vpp_bilinear_up2_core.h", "vpp_bicubic_r32_core.h", "vpp_r32_store.h", "vpp_up2.h"]}.get(unit, [])
    return ["tensor-stream_amd/csrc/" + f for f in [unit] + extra] + _SHARED_SOURCES


def kernel_src_hash(kernel=None):
    h = hashlib.sha256()
    for rel in kernel_source_files(kernel):
        with open(os.path.join(ROOT, rel), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def lookup_traffic(workload, frames_per_launch, path=None, kernel=None, alg_read=None, alg_write=None, touched_read=None):
    """HBM bytes per launch from the committed PMC passes (tools/profile.sh -> tools/traffic_json.py).  The counters
    need their own rocprofv3 runs, so this is the last PROFILED value for this workload -- returned only when the entry
    was taken on the kernel that is dispatched now, with that kernel's sources (its translation unit + the shared device
    headers) as they are now (`kernel_src_sha`); a stale entry yields (None, reason).

    An entry must also be PLAUSIBLE as one kernel's traffic (round 3 published a six-kernel blend whose sum happened to land on
    1.005x): with the algorithmic split per launch given (`alg_read`, `alg_write`), the write side must be within 10 % of it and
    the read side between 0.9x and 1.35x of it (tile halos are re-read) -- or, for a sampler that skips source bytes, from 0.9x the touched source
    bytes (`touched_read`, bench.touched_bytes).  Anything else is refused with the numbers in the reason."""
    path = path or os.path.join(ROOT, "profiles", "traffic_latest.json")
    try:
        tr = json.load(open(path)).get(workload)
    except (OSError, ValueError) as e:
        return None, f"no traffic file: {e}"
    if not tr:
        return None, "no PMC entry for this workload"
    if tr.get("frames_per_launch") != frames_per_launch:
        return None, "PMC entry is for another launch size"
    if kernel and tr.get("kernel") and tr["kernel"] != kernel:
        return None, f"stale PMC entry ({tr.get('round')}): it profiled {tr['kernel']}, the launch now dispatches {kernel}"
    want = kernel_src_hash(tr.get("kernel") if tr.get("kernel") else None)
    if tr.get("kernel_src_sha") != want:
        return None, f"stale PMC entry ({tr.get('round')}): kernel sources changed since it was profiled"
    note = ""
    if alg_read is not None and alg_write is not None:
        rd, wr = tr.get("read_bytes"), tr.get("write_bytes")
        if rd is None or wr is None:
            return None, f"PMC entry ({tr.get('round')}) has no read / write split: cannot be checked against the algorithmic split"
        if not 0.9 * alg_write <= wr <= 1.1 * alg_write:
            return None, (f"implausible PMC entry ({tr.get('round')}): {wr} B written per launch, the launch writes {int(alg_write)} B "
                          "(more than 10 % off: not this kernel's traffic)")
        # reads: not below what the launch must touch (-10 %), and at most 1.35x the ROI: kernels whose tiles overlap re-read a halo (the streaming BICUBIC
        # kernel: rows -1 .. +2 around a tile's six, 1.22x; the column kernel 1.13x) -- round 3's six-kernel blend read 1.71x and wrote 0.81x
        lo = 0.9 * (min(touched_read, alg_read) if touched_read is not None else alg_read)
        if not lo <= rd <= 1.35 * alg_read:
            return None, (f"implausible PMC entry ({tr.get('round')}): {rd} B read per launch, algorithmic {int(alg_read)} B"
                          + (f", touched {int(touched_read)} B" if touched_read is not None else "") + " (outside the plausible band)")
        if rd < 0.9 * alg_read:
            note = f"; reads {rd / alg_read:.3f}x the ROI bytes, explained by touched_bytes ({touched_read / alg_read:.3f}x)"
        elif rd > 1.1 * alg_read:
            note = f"; read {rd / alg_read:.3f}x the algorithmic bytes (tile halo re-read) / write {wr / alg_write:.4f}x"
        else:
            note = f"; read {rd / alg_read:.4f}x / write {wr / alg_write:.4f}x the algorithmic split"
    return tr["hbm_bytes_per_launch"], (f"profiles/traffic_latest.json ({tr['round']}, {tr.get('kernel_csv_name') or tr.get('kernel', 'all kernels')}, "
                                        f"{tr.get('dispatches')} dispatches, kernel_src_sha {tr['kernel_src_sha']}): 2*FETCH_SIZE+WRITE_SIZE, KiB{note}")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=0, help="the timed region of --steps steps is run this many times and the median is reported; "
                    "0 = one region (exactly --steps timed steps), or with --full max(5, ceil(400 / steps)): SURVEY.md 8(d) asks for >= 200 timed iterations and a median of 5; "
                    "400 keep the clock ramp of the first ~25 ms out of the median")
    ap.add_argument("--full", action="store_true", help="everything besides the headline figure: the median over --repeats regions, the oracle parity gate, the other resize "
                    "types and BASELINE configurations, the facade / latency / launch-curve legs and the cpu_baseline.  Off: set up, warm up, time --steps steps, print the line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32, "
                    "at most 64 MiB: the whole output, or whole frames plus a fixed seeded sample of it; see output_arrays)")
    ap.add_argument("--batch", type=int, default=None, help="frames per step (one launch per MAX_LAUNCH = 128 frames: tsvpp.h TSVPP_MAX_BATCH; with --table up to 1024 per launch).  "
                    "Default: 64 -- except the small-frame BASELINE configurations C3 (512) and C4 (256), which run out of a persistent frame table (DEFAULT_BATCH)")
    ap.add_argument("--table", action="store_true", help="register every buffer set ONCE in a persistent device-resident frame table (tsvpp_table_*) and convert it with "
                    "tsvpp_convert_table: launches of up to 1024 frames (--batch may then exceed 128 per launch); the pools of a real pipeline come round again the same way")
    ap.add_argument("--workload", default="headline", choices=sorted(WORKLOADS))
    ap.add_argument("--alias", type=int, default=0, help="DIAGNOSTIC (not a measurement of the path): bit 0 = all frames of a launch read one "
                    "input frame, bit 1 = all write one output buffer, so that reads / writes stay in cache; separates issue-bound from memory-bound kernels")
    ap.add_argument("--streams", type=int, default=1, help="DIAGNOSTIC (not the bench line's measurement): issue the steps of a timed region round-robin on N HIP streams -- "
                    "independent batches of N consumers: one launch's drain overlaps the next one's fill; avg_launch_ms is then wall time per launch, not a launch's duration")
    ap.add_argument("--resize", default=None, choices=sorted(RESIZE), help="override the resize type")
    ap.add_argument("--sets", type=int, default=3, help="rotating buffer sets")
    ap.add_argument("--custom", default=None, help="ad-hoc workload SRCWxSRCH:DSTWxDSTH:RESIZE:FOURCC:PLANES:NORM[:L,T,R,B crop], e.g. 1920x1080:224x224:BILINEAR:RGB24:PLANAR:1")
    ap.add_argument("--per-call", type=int, default=0, help="frames per C-ABI call (default: the whole batch); 1 = the reference's one Convert per frame")
    ap.add_argument("--graph", action="store_true", help="capture a step's calls in a hipGraph and replay it (launch-bound small calls)")
    ap.add_argument("--tight-pitch", action="store_true", help="source pitch = width instead of width rounded up to 256 bytes")
    ap.add_argument("--cpu-budget", type=float, default=12.0, help="seconds of CPU work for the cpu_baseline sample")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-others", action="store_true", help="skip the NEAREST/BICUBIC/AREA side measurements of the headline")
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--warmup-ms", type=float, default=40.0, help="time-based warm-up after the --warmup steps: untimed steps until the device has worked this long (clock ramp)")
    ap.add_argument("--consumers", type=int, default=0, help="C5 AS BASELINE.json WORDS IT (\"64 concurrent consumers, 8x MI355X\"): the step is ONE TensorStreamConverter.read_many over "
                    "consumers / world NAMED consumers of this rank's own converter (synthetic 4K source, one pooled stream per consumer name, reference src/VideoProcessor.cpp:98-104) "
                    "instead of a C-ABI batch over pre-built descriptors; --workload c5 --consumers 64 --gpus N.  consumers must be a multiple of the world size")
    ap.add_argument("--curve-only", default=None, help="run only the launch-curve leg (1 .. 64 frames per launch, tensor-stream_amd/cpp/vpp_curve.cpp) for these workloads, "
                    "comma separated (e.g. headline,c3,c4), print its JSON and exit")
    ap.add_argument("--no-pin", action="store_true", help="N > 1: do not pin the rank to the CPUs local to its GPU")
    args = ap.parse_args(argv)
    if args.dump_outputs and args.consumers:
        ap.error("--dump-outputs needs a C-ABI workload: with --consumers the frame a step converts follows the producer thread's clock, so two runs are not comparable")
    return args


DUMP_BYTES = 64 << 20       # --dump-outputs: the files of one run, in all
DUMP_SAMPLE = 4 << 20       # elements of the seeded sample of an output larger than DUMP_BYTES (16 MiB as float32)
DUMP_SEED = 20240611


def output_arrays(out, frames=None):
    """What a caller of the timed path receives -- `out`, the (B, ...) output tensor of one step -- as float32 numpy arrays of at most DUMP_BYTES in all.
    An output that fits is returned whole (`output`).  A larger one gives `output_frames` (whole frames `frames`, default first / middle / last of the
    batch, as many as fit beside the sample; their indices in `output_frame_index`) and `output_sample` (DUMP_SAMPLE elements of the flattened
    output at sorted indices drawn from a generator seeded with DUMP_SEED: the same positions in every run of the same arguments)."""
    n = out.numel()
    if n * 4 <= DUMP_BYTES:
        return {"output": out.float().cpu().numpy()}
    B = out.shape[0]
    per_frame = n // B
    room = DUMP_BYTES - DUMP_SAMPLE * 4 - (1 << 20)
    if frames is None:
        frames = sorted({0, B // 2 - 1 if B > 2 else 0, B - 1})
    frames = list(frames)[: max(0, room // (per_frame * 4))]
    arrays = {}
    if frames:
        arrays["output_frames"] = out[frames].float().cpu().numpy()
        arrays["output_frame_index"] = np.array(frames, dtype=np.float64)
    idx = np.unique(np.random.default_rng(DUMP_SEED).integers(0, n, size=min(n, DUMP_SAMPLE), dtype=np.int64))
    import torch
    flat = out.reshape(-1)
    arrays["output_sample"] = flat[torch.from_numpy(idx).to(flat.device)].float().cpu().numpy()
    return arrays


def dump_outputs(directory, arrays):
    os.makedirs(directory, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(directory, k + ".npy"), a)
    return sorted(arrays)


def resolve_spec(args):
    """(spec tuple, workload name) after --custom / --resize / --tight-pitch."""
    spec = list(WORKLOADS[args.workload])
    name = args.workload
    if args.custom:
        a = args.custom.split(":")
        sw, sh = (int(x) for x in a[0].split("x"))
        dw, dh = (int(x) for x in a[1].split("x"))
        crop = tuple(int(x) for x in a[6].split(",")) if len(a) > 6 else (0, 0, 0, 0)   # optional 7th field: the crop box left,top,right,bottom
        spec = [sw, sh, (sw + 255) // 256 * 256, crop, (dw, dh), a[2], a[3], a[4], a[5] == "1"]
        name = "custom"
    if args.resize:
        spec[5] = args.resize
    if args.tight_pitch:
        spec[2] = spec[0]
    return tuple(spec), name


def metric_name(name, resize_override):
    return METRIC if (name == "headline" and not resize_override) else f"{name}{'/' + resize_override if resize_override else ''} frames/sec"


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn(args, argv):
    """`python bench.py --gpus N` without a torch.distributed environment: check that N GPUs are visible and re-execute
    under torch.distributed.run, one rank per GPU (reference README.md:193-196: one instance per GPU)."""
    stub = os.environ.get("TSVPP_BENCH_STUB") == "1"
    visible = args.gpus
    if not stub:
        import torch
        visible = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if visible < args.gpus:
        spec, name = resolve_spec(args)
        print(json.dumps({"metric": metric_name(name, args.resize), "value": None, "unit": "frames/s", "n_gpus": args.gpus,
                          "n_gpus_visible": visible, "status": f"not measured: {args.gpus} GPUs requested, {visible} visible (nothing is extrapolated)",
                          "steps": args.steps, "warmup": args.warmup, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                          "data": "synthetic", "config": {"workload": name}}), flush=True)
        return 0
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    # The port is chosen by binding port 0 and closing the socket: another process can take it before the rendezvous binds it.  A launch that
    # dies WITHOUT having printed the line (rendezvous failures do: nothing has been measured yet) is retried on a fresh port, twice at most;
    # the child's stdout is held back so that a failed attempt can never leave a second line behind.
    rc, out = 1, ""
    for attempt in range(3):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
        rc, out = p.returncode, p.stdout
        if rc == 0 or '{"metric"' in out or '{"error"' in out:  # (an error line is an answer too: set-up failed on some rank, retrying cannot help)
            break
        print(f"bench.py: launch attempt {attempt + 1} of {args.gpus} ranks exited {rc} without a line; retrying on another port", file=sys.stderr, flush=True)
    sys.stdout.write(out)
    sys.stdout.flush()
    return rc


class _StubWork:
    def __init__(self, args, batch=None):
        self.B = batch or args.batch
        self.frames_per_launch = float(min(self.B, MAX_LAUNCH))
        self.launches_per_step = (self.B + MAX_LAUNCH - 1) // MAX_LAUNCH

    def issue(self, i, stream):
        time.sleep(0.0005)


class StubEngine:
    """TSVPP_BENCH_STUB=1 (CPU tests of the launch / rendezvous / reduction plumbing only): no GPU, no kernels; a step is
    a short sleep.  The line it produces is marked `"data": "stub"` and is never a measurement."""

    def __init__(self, args, spec, rank):
        self.args = args
        self.frames_per_launch = float(min(args.batch, MAX_LAUNCH))
        self.launches_per_step = (args.batch + MAX_LAUNCH - 1) // MAX_LAUNCH
        self.ws_mib = 0.0
        self.parity = "stub"
        self.graphs = False
        self.cur_stream = 0
        self.n_sets = 1

    def step(self, i):
        time.sleep(0.0005)

    def last_output(self, last_step):
        """A stand-in for the output of a step (the stub converts nothing): deterministic, so the --dump-outputs plumbing is testable without a GPU."""
        import torch
        return torch.arange(self.args.batch * 3 * 16, dtype=torch.float32).reshape(self.args.batch, 3, 4, 4) / 255.0

    def sync(self):
        pass

    def timed(self, steps, first, work=None):
        t0 = time.perf_counter()
        for i in range(steps):
            self.step(first + i)
        dt = time.perf_counter() - t0
        return dt * 1e3, dt  # "device" ms, host issue s

    def side_work(self, spec, sets=2, batch=None, table=False):
        return _StubWork(self.args, batch)

    def close(self):
        pass


class FacadeEngine:
    """--consumers C: the production entry as the engine of the timed region.  Each rank owns one TensorStreamConverter on a synthetic source of the workload's size
    (a pool of distinct frames three times the Infinity Cache, uploaded once) with C / world named consumers; a step = one read_many(names) = one hand-off under one
    lock + ONE batched launch + one output tensor, every consumer its own view (tensor_stream/tensor_stream.py).  StubFacadeEngine is its CPU twin (launch plumbing tests)."""

    def __init__(self, args, spec, rank, world, dev, dist):
        import torch
        import tensor_stream as ts
        from tensor_stream import parallel
        self.torch, self.ts, self.dev, self.rank, self.args, self.spec = torch, ts, dev, rank, args, spec
        src_w, src_h, pitch, crop, dst, rt, fcc, planes, norm = spec
        if args.consumers % world:
            raise RuntimeError(f"--consumers {args.consumers} is not a multiple of the world size {world}")
        self.n = args.consumers // world
        self.names = [f"consumer{rank * self.n + i}" for i in range(self.n)]  # global consumer ids: consumer c lives on rank c // (C / world)
        self.pool = max(8, -(-(768 << 20) // (src_w * src_h * 3 // 2)))
        self.seed = 300 + rank
        self.conv = ts.TensorStreamConverter(f"synthetic://{src_w}x{src_h}?seed={self.seed}&frames=0&fps=100000&pool={self.pool}", max_consumers=self.n, cuda_device=dev,
                                             framerate_mode=ts.FrameRate.FAST)
        self.conv.initialize()
        self.coeffs = parallel.broadcast_coeffs(self.conv._vpp, dist)
        self.coeff_broadcast = parallel.last_broadcast_info()
        self.conv.start()
        self.kw = dict(width=dst[0], height=dst[1], resize_type=RESIZE[rt], crop_coords=crop, pixel_format=FOURCC[fcc], planes_pos=PLANES[planes], normalization=norm)
        self.fp = ts.FrameParameters(**self.kw)
        self.frames_per_launch = float(self.n)
        self.launches_per_step = 1
        self.ws_mib = self.pool * src_w * src_h * 1.5 / 2**20
        self.parity = "skipped"
        self.graphs = []
        self.extra_streams = []
        self.cur_stream = torch.cuda.current_stream(dev).cuda_stream
        self.last = None
        self.n_sets = 1

    def step(self, i):
        self.last = self.conv.read_many(self.names, **self.kw)

    def sync(self):
        self.torch.cuda.synchronize()

    def timed(self, steps, first, work=None):
        torch = self.torch
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        ev0.record()
        for i in range(steps):
            self.step(first + i)
        ev1.record()
        host_issue = time.perf_counter() - t0
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1), host_issue

    def check_parity(self, last_step, work=None):
        """One more read_many with its frame index: the first and the last consumer's tensors against the oracle's conversion of that pool frame."""
        from oracle import oracle as O
        from tensor_stream.sources import open_source
        src_w, src_h, pitch, crop, dst, rt, fcc, planes, norm = self.spec
        tensors, index = self.conv.read_many(self.names, return_index=True, **self.kw)
        self.torch.cuda.synchronize()
        src = open_source(f"synthetic://{src_w}x{src_h}?seed={self.seed}&frames=0&pool={self.pool}")
        y, uv = src.pool[(index - 1) % self.pool]
        ref, _, _ = O.convert(y, uv, crop=crop, dst=dst, resize_type=RESIZE[rt], fourcc=FOURCC[fcc], planes=PLANES[planes], normalization=norm, nthreads=min(16, O.host_cores()))
        ok = all(np.array_equal(t.cpu().numpy().ravel().view(np.uint8), ref.view(np.uint8)) for t in (tensors[0], tensors[-1]))
        return ok, (f"bit-exact vs oracle (consumers {self.names[0]} / {self.names[-1]} of one read_many after the timed region, frame {index})" if ok else "MISMATCH vs oracle")

    def kernel_name(self):
        try:
            dsc = self.ts.vpp.describe(self.fp, self.spec[0], self.spec[1], pitch=self.spec[0], n_frames=int(self.n))
            return "tsvpp::" + str(dsc.get("kernel", "?"))
        except Exception as e:  # noqa: BLE001
            return f"tsvpp::? ({type(e).__name__}: {e})"

    def side_work(self, spec, sets=2, batch=None, table=False):
        raise RuntimeError("no side legs in --consumers mode")

    def close(self):
        self.conv.stop()


class StubFacadeEngine(StubEngine):
    """TSVPP_BENCH_STUB=1 --consumers C: C / world named consumers per rank, a step is a short sleep (tests of the sharding / reduction plumbing at world 8)."""

    def __init__(self, args, spec, rank, world):
        if args.consumers % world:
            raise RuntimeError(f"--consumers {args.consumers} is not a multiple of the world size {world}")
        self.n = args.consumers // world
        self.names = [f"consumer{rank * self.n + i}" for i in range(self.n)]
        args.batch = self.n
        super().__init__(args, spec, rank)


class GpuWork:
    """One workload resident in HBM: `sets` rotating buffer sets of B synthetic frames (distinct per frame / set / rank)
    and the prebuilt batch descriptors (a step is then one C-ABI call per `per_call` frames)."""

    def __init__(self, eng, spec, B, sets, seed, alias=0, per_call=0, table=False):
        torch, ts, vpp = eng.torch, eng.ts, eng.vpp
        src_w, src_h, pitch, crop, dst, rt, fcc, planes, norm = spec
        self.spec, self.B, self.torch = spec, B, torch
        self.fp = ts.FrameParameters(width=dst[0], height=dst[1], crop_coords=crop, resize_type=RESIZE[rt],
                                     pixel_format=FOURCC[fcc], planes_pos=PLANES[planes], normalization=norm)
        vpp.prepare(self.fp, src_w, src_h, n_frames=B)  # tables + scratch for this batch size: the timed region allocates nothing
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.sets = []
        for _ in range(sets):
            ys = torch.randint(0, 256, (B, src_h, pitch), dtype=torch.uint8, device="cuda", generator=g)
            uvs = torch.randint(0, 256, (B, src_h // 2, pitch), dtype=torch.uint8, device="cuda", generator=g)
            out = vpp._alloc(self.fp.parameters, src_w, src_h, B)
            if alias & 1:   # diagnostic: every frame of the set reads frame 0 (reads stay in L2 / Infinity Cache)
                ys, uvs = ys[:1].expand(B, -1, -1), uvs[:1].expand(B, -1, -1)
            if alias & 2:   # diagnostic: every frame writes frame 0's buffer (writes combine in L2)
                out = out[:1].expand(B, *([-1] * (out.dim() - 1)))
            self.sets.append((ys, uvs, out))
        self.ws_mib = sum(a.numel() * a.element_size() for s in self.sets for a in s) / 2**20
        # descriptor arrays are built once per buffer set; a step is then a single C-ABI call
        F = per_call if 0 < per_call < B else B
        self.batches = [[vpp.make_batch(ys[k:k + F], uvs[k:k + F], self.fp, out=out[k:k + F], width=src_w) for k in range(0, B, F)]
                        for (ys, uvs, out) in self.sets]
        self.launches_per_step = ((F + MAX_LAUNCH - 1) // MAX_LAUNCH) * (B // F) + ((B % F + MAX_LAUNCH - 1) // MAX_LAUNCH)
        self.tables = None
        if table:  # the same buffer sets, registered once: a step is ONE tsvpp_convert_table call over the whole set
            self.tables = [vpp.make_table(ys, uvs, self.fp, out=out, width=src_w) for (ys, uvs, out) in self.sets]
            _, _, dw, dh = roi_and_dst(src_w, src_h, crop, dst)
            cap = max(MAX_LAUNCH, min(MAX_TABLE_LAUNCH, ((1 << 31) // 256) // max(1, ((dw + 63) // 64) * ((dh + 3) // 4))))  # tsvpp_api.cpp: convert_impl
            two_pass = fcc in ("UYVY", "YUV444") and "pass2" in str(ts.describe(self.fp, src_w, src_h, pitch=pitch, n_frames=min(B, MAX_LAUNCH)))
            if two_pass:
                cap = MAX_LAUNCH
            self.launches_per_step = (B + cap - 1) // cap
        self.frames_per_launch = B / self.launches_per_step
        self.vpp = vpp

    def parity(self, O, set_index=0, frames=None):
        """Frames `frames` (default: first / middle / last of the batch) of buffer set `set_index` AS THE TIMED LAUNCHES LEFT THEM against the
        oracle, bit for bit.  Nothing is launched here: the dispatcher's choice of kernel, tile shape and rows per thread depends on the
        number of frames in a launch, so only the output of the timed launch configuration itself proves the timed configuration
        (VERDICT r03 weak #2).  Returns (ok, frames checked)."""
        src_w, src_h, pitch, crop, dst, rt, fcc, planes, norm = self.spec
        ys, uvs, out = self.sets[set_index % len(self.sets)]
        if frames is None:
            frames = sorted({0, self.B // 2 - 1 if self.B > 2 else 0, self.B - 1})
        self.torch.cuda.synchronize()
        for k in frames:
            ref, _, _ = O.convert(ys[k].cpu().numpy(), uvs[k].cpu().numpy(), crop=crop, dst=dst, resize_type=RESIZE[rt],
                                  fourcc=FOURCC[fcc], planes=PLANES[planes], normalization=norm, nthreads=min(16, O.host_cores()), width=src_w)
            got = out[k].cpu().numpy().ravel()
            if not np.array_equal(got.view(np.uint8), ref.view(np.uint8)):
                return False, frames
        return True, frames

    def issue(self, i, stream):
        if self.tables is not None:
            self.vpp.run_table(self.tables[i % len(self.tables)], stream=stream)
            return
        for b in self.batches[i % len(self.batches)]:
            self.vpp.run_batch(b, stream)


class GpuEngine:
    def __init__(self, args, spec, rank, dev, dist):
        import torch
        import tensor_stream as ts
        from tensor_stream import parallel
        self.torch, self.ts, self.dev, self.rank, self.args = torch, ts, dev, rank, args
        src_w, src_h, pitch, crop, dst, rt, fcc, planes, norm = spec
        self.spec = spec
        self.vpp = ts.VideoProcessor(device=dev, max_consumers=8)
        # the one collective of the path: rank 0's colour coefficient block -> every rank (RCCL over xGMI)
        self.coeffs = parallel.broadcast_coeffs(self.vpp, dist)
        self.coeff_broadcast = parallel.last_broadcast_info()
        B = args.batch
        self.work = GpuWork(self, spec, B, args.sets, 1234 + rank, alias=args.alias, per_call=args.per_call, table=getattr(args, "table", False))
        self.fp = self.work.fp
        self.ws_mib = self.work.ws_mib
        self.launches_per_step = self.work.launches_per_step
        self.frames_per_launch = self.work.frames_per_launch
        self.n_sets = len(self.work.sets)  # step i converts buffer set i % n_sets (graphs: one per set)

        self.parity = "skipped"  # filled in by check_parity() AFTER the timed region, on the timed launches' own output

        self.cur_stream = torch.cuda.current_stream(dev).cuda_stream
        self.extra_streams = [torch.cuda.Stream() for _ in range(max(0, getattr(args, "streams", 1) - 1))]  # --streams N (diagnostic)
        self.graphs = []
        if args.graph:  # one graph per buffer set, captured on a side stream, replayed on the current one
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                for i in range(len(self.work.batches)):
                    self.work.issue(i, side.cuda_stream)
            torch.cuda.synchronize()
            for i in range(len(self.work.batches)):
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=side):
                    self.work.issue(i, side.cuda_stream)
                self.graphs.append(gr)

    def check_parity(self, last_step, work=None):
        """The parity gate of the line: frames 0 / B/2-1 / B-1 of the buffer set the LAST TIMED STEP wrote, against the oracle.
        The timed launches are the checked launches; a mismatch is fatal (exit 2, no line)."""
        from oracle import oracle as O
        w = work or self.work
        ok, frames = w.parity(O, set_index=last_step % len(w.sets))
        rt = w.spec[5]
        txt = (f"bit-exact vs oracle (frames {'/'.join(str(k) for k in frames)} of the timed launch, full size)" if ok else "MISMATCH vs oracle")
        if ok and rt == "BICUBIC":  # the oracle's pow(w,2)/pow(w,3) are the exact square / correctly rounded cube
            txt += " (BICUBIC at non-dyadic weights is oracle-defined: the reference's pow() is library-dependent)"
        return ok, txt

    def kernel_name(self):
        """The kernel the timed launches dispatch (host-side dry run of the same selection: tsvpp_describe)."""
        src_w, src_h, pitch = self.spec[0], self.spec[1], self.spec[2]
        try:
            dsc = self.ts.vpp.describe(self.fp, src_w, src_h, pitch=pitch, n_frames=int(min(self.args.batch, MAX_LAUNCH)))
            return "tsvpp::" + str(dsc.get("kernel", "?"))
        except Exception as e:
            return f"tsvpp::? ({type(e).__name__}: {e})"

    def last_output(self, last_step):
        """The output tensor step `last_step` wrote: its buffer set's (B, ...) output, as a caller of tsvpp_convert_batch receives it."""
        return self.work.sets[last_step % self.n_sets][2]

    def step(self, i):
        if self.graphs:
            self.graphs[i % len(self.graphs)].replay()
        else:
            self.work.issue(i, self.cur_stream)

    def sync(self):
        self.torch.cuda.synchronize()

    def timed(self, steps, first, work=None):
        """K steps between two HIP events on torch's current stream == the stream convert_batch launches on.
        Returns (device ms between the events, host seconds spent issuing)."""
        torch = self.torch
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        ev0.record()
        if self.extra_streams and work is None:  # --streams N: step k on stream k mod N, all forked from / joined into the current stream
            n = len(self.extra_streams) + 1
            for st in self.extra_streams:
                st.wait_event(ev0)
            for i in range(steps):
                k = (first + i) % n
                self.work.issue(first + i, self.cur_stream if k == 0 else self.extra_streams[k - 1].cuda_stream)
            for st in self.extra_streams:
                e = torch.cuda.Event()
                e.record(st)
                torch.cuda.current_stream().wait_event(e)
        elif work is None:
            for i in range(steps):
                self.step(first + i)
        else:
            for i in range(steps):
                work.issue(first + i, self.cur_stream)
        ev1.record()
        host_issue = time.perf_counter() - t0
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1), host_issue

    def side_work(self, spec, sets=2, batch=None, table=False):
        """A second workload on the same context (other resize types of the headline, the 4K configurations): its own buffers."""
        # enough rotating buffer sets that the leg's working set is >= 768 MiB, three times the Infinity Cache (C1's 64-frame set is 265 MB: two sets would half-fit)
        B = batch or self.args.batch
        src_w, src_h, pitch, crop, dst, _rt, fcc, _pl, norm = spec
        _, _, dw, dh = roi_and_dst(src_w, src_h, crop, dst)
        per_set = B * (pitch * src_h * 3 // 2 + int(dw * dh * {0: 1.0, 3: 1.5, 4: 2.0}.get(FOURCC[fcc], 3.0)) * (4 if (norm or fcc == "HSV") else 1))
        sets = min(6, max(sets, -(-(768 << 20) // per_set)))
        return GpuWork(self, spec, B, sets, 4321 + self.rank, table=table)

    def close(self):
        self.vpp.Close()


def pin_to_gpu_numa(dev):
    """Best effort: restrict this rank to the CPUs local to its GPU's PCIe root (the >= 7.5x target at 8 GPUs dies on host
    launch overhead, nothing else).  Returns a short description for the JSON line; never raises."""
    try:
        import torch
        p = torch.cuda.get_device_properties(dev)
        bdf = "%04x:%02x:%02x.0" % (int(getattr(p, "pci_domain_id", 0)), int(p.pci_bus_id), int(getattr(p, "pci_device_id", 0)))
        path = f"/sys/bus/pci/devices/{bdf.lower()}/local_cpulist"
        cpus = set()
        for part in open(path).read().strip().split(","):
            if not part:
                continue
            a, _, b = part.partition("-")
            cpus.update(range(int(a), int(b or a) + 1))
        allowed = os.sched_getaffinity(0)
        want = cpus & allowed
        if not want:
            return f"{bdf}: local CPUs outside this process's cpuset (left unpinned, {len(allowed)} CPUs)"
        if want != allowed:
            os.sched_setaffinity(0, want)
        return f"{bdf}: {len(want)} local CPUs of {len(allowed)} allowed"
    except Exception as e:
        return f"unpinned ({type(e).__name__}: {e})"


def run(args):
    stub = os.environ.get("TSVPP_BENCH_STUB") == "1"
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    spec, name = resolve_spec(args)
    src_w, src_h, pitch, crop, dst, rt, fcc, planes, norm = spec
    if args.batch is None:  # per-workload default (DEFAULT_BATCH); an explicit --batch is taken as given
        args.batch, tbl = DEFAULT_BATCH.get(name if not (args.resize or args.per_call or args.graph) else "", (64, False))
        args.table = args.table or tbl
    dist = None
    out_fd = None
    backend = None
    # ---- set-up, time-boxed.  The driver's SCALE run is the first time this code meets 8 real GPUs: a rank that dies or hangs in ANY set-up step
    # (rendezvous, RCCL communicator, NUMA pinning, the 2.6 GiB buffer fill, the coefficient broadcast) must end the job with ONE {"error": ...} line and a non-zero exit
    # code, never with seven ranks parked in a barrier.  Every step is timed and logged to stderr with the rank; the per-rank totals travel in the line (`setup_s`).
    setup_limit = float(os.environ.get("TSVPP_BENCH_SETUP_TIMEOUT", "300"))
    setup_log = []

    def log(msg):
        print(f"[bench.py rank {rank}/{world}] {msg}", file=sys.stderr, flush=True)

    def fail_line(why, code=3):
        """The job cannot be measured: rank 0 says so on stdout (one JSON line), every rank on stderr; exit without waiting for anybody."""
        log(f"SET-UP FAILED: {why}")
        if rank == 0:
            line = json.dumps({"error": f"set-up failed: {why}", "metric": metric_name(name, args.resize), "value": None, "unit": "frames/s", "n_gpus": world,
                               "steps": args.steps, "warmup": args.warmup, "setup_log": setup_log})
            try:
                os.write(out_fd if out_fd is not None else 1, (line + "\n").encode())
            except OSError:
                pass
        os._exit(code)

    import signal
    import threading
    # rank 0 reports first (it owns the line); the other ranks give it five seconds, then leave too
    watchdog = threading.Timer(setup_limit + (0.0 if rank == 0 else 5.0),
                               lambda: fail_line(f"rank {rank} did not finish set-up within {setup_limit:.0f} s (last step: {setup_log[-1][0] if setup_log else 'none'})"))
    watchdog.daemon = True
    watchdog.start()
    # a rank that dies outright makes the launcher SIGTERM the others: rank 0 still says why there is no measurement
    old_term = None
    try:
        old_term = signal.signal(signal.SIGTERM, lambda *_: fail_line("terminated by the launcher during set-up (another rank died: see its stderr)", code=4))
    except ValueError:  # not the main thread (in-process tests)
        pass

    def step_of(label, fn):
        t_s = time.perf_counter()
        setup_log.append([label, None])
        log(f"set-up: {label} ...")
        r = fn()
        setup_log[-1][1] = round(time.perf_counter() - t_s, 3)
        log(f"set-up: {label} done in {setup_log[-1][1]:.3f} s")
        return r

    inject = os.environ.get("TSVPP_BENCH_FAIL", "")  # tests: "<rank>:<step>:<raise|hang|exit>" makes that rank fail in that set-up step

    def injected(label):
        if not inject:
            return
        r_, s_, how = inject.split(":")
        if int(r_) == rank and s_ == label:
            if how == "hang":
                time.sleep(10 * setup_limit)
            if how == "exit":
                os._exit(9)
            raise RuntimeError(f"injected failure in {label}")

    t_setup = time.perf_counter()
    eng = None
    affinity = None
    setup_error = None
    try:
        # world == 1 still takes the collective path under torch.distributed.run (`--nproc-per-node=1`) or TSVPP_BENCH_FORCE_DIST=1:
        # the RCCL plumbing is exercised on a one-GPU box (tests/test_bench_gpu.py) before an 8-GPU node ever sees it
        if world > 1 or os.environ.get("TSVPP_BENCH_FORCE_DIST") == "1" or "TORCHELASTIC_RUN_ID" in os.environ:
            # RCCL prints a version banner on stdout: keep stdout for the ONE JSON line (everything else goes to stderr)
            sys.stdout.flush()
            out_fd = os.dup(1)
            os.dup2(2, 1)
            import datetime
            import torch.distributed as dist_mod
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29511")
            tmo = datetime.timedelta(seconds=max(30.0, setup_limit))

            def init_pg():
                injected("rendezvous")
                if stub:
                    dist_mod.init_process_group("gloo", rank=rank, world_size=world, timeout=tmo)
                else:
                    import torch
                    torch.cuda.set_device(local)
                    dist_mod.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local), timeout=tmo)
            backend = "gloo" if stub else "nccl"
            step_of("rendezvous", init_pg)
            dist = dist_mod
        if stub:
            def make_stub():
                injected("engine")
                return StubFacadeEngine(args, spec, rank, world) if args.consumers else StubEngine(args, spec, rank)
            eng = step_of("engine", make_stub)
        else:
            import torch
            dev = local if dist is not None else 0
            torch.cuda.set_device(dev)
            if dist is not None and not args.no_pin:
                affinity = step_of("numa-pin", lambda: pin_to_gpu_numa(dev))

            def make_engine():
                injected("engine")
                if args.consumers:
                    return FacadeEngine(args, spec, rank, world, dev, dist)
                return GpuEngine(args, spec, rank, dev, dist)  # context, coefficient broadcast (the one collective), buffer fill, descriptor tables
            eng = step_of("engine", make_engine)
    except Exception as e:  # noqa: BLE001 -- anything: the other ranks must learn about it
        setup_error = f"rank {rank}: {type(e).__name__}: {e}"
        log(f"set-up error: {setup_error}")
    # every rank tells every rank whether it is ready: a failed rank takes part in this ONE collective (if it still can) so that the others leave together
    if dist is not None:
        try:
            import torch
            flag = torch.tensor([0.0 if setup_error else 1.0], dtype=torch.float64, device="cpu" if stub else "cuda")
            step_of("ready-check", lambda: dist.all_reduce(flag, op=dist.ReduceOp.MIN))
            if flag.item() < 0.5 and not setup_error:
                setup_error = "another rank failed its set-up (see its stderr)"
        except Exception as e:  # noqa: BLE001
            setup_error = setup_error or f"rank {rank}: ready-check failed: {type(e).__name__}: {e}"
    if setup_error:
        fail_line(setup_error)
    watchdog.cancel()
    if old_term is not None:
        signal.signal(signal.SIGTERM, old_term)
    setup_s = round(time.perf_counter() - t_setup, 3)
    log(f"set-up complete in {setup_s:.3f} s")

    if args.consumers:
        args.batch = eng.n  # frames per step = this rank's consumers
    B = args.batch

    def bytes_of(sp):
        chans = {0: 1.0, 3: 1.5, 4: 2.0}.get(FOURCC[sp[6]], 3.0)
        return algorithmic_bytes(sp[0], sp[1], sp[3], sp[4], sp[8] or sp[6] == "HSV", chans, luma_only=(sp[6] == "Y800"))

    bytes_per_frame = bytes_of(spec)
    _rw, _rh, _dw, _dh = roi_and_dst(src_w, src_h, crop, dst)
    write_bytes_per_frame = int(_dw * _dh * {0: 1.0, 3: 1.5, 4: 2.0}.get(FOURCC[fcc], 3.0)) * (4 if (norm or fcc == "HSV") else 1)

    def barrier():
        if dist is not None:
            dist.barrier()

    def reduce_max(vals):
        if dist is None:
            return vals
        import torch
        t = torch.tensor(vals, dtype=torch.float64, device="cpu" if stub else "cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return t.tolist()

    def gather(val):
        """One float per rank -> list (rank order) on every rank."""
        if dist is None:
            return [val]
        import torch
        t = torch.zeros(world, dtype=torch.float64, device="cpu" if stub else "cuda")
        t[rank] = val
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return t.tolist()

    def region(steps, first, work=None):
        """One timed region of exactly `steps` steps: barrier + synchronize on both sides, max over ranks."""
        barrier()
        eng.sync()
        t0 = time.perf_counter()
        dev_ms, host_issue = eng.timed(steps, first, work) if work is not None else eng.timed(steps, first)  # ends with a device synchronize
        barrier()
        wall = time.perf_counter() - t0
        mine = (wall, dev_ms, host_issue)
        return tuple(reduce_max(list(mine))), mine

    for i in range(args.warmup):
        eng.step(i)
    first = args.warmup
    # Time-based warm-up: the device needs ~25 ms of continuous work to settle its clocks (profiles/r02_bench_driver_cmd.json, first
    # version: regions of 20 steps ran 0.167, 0.182, 0.163, 0.158, 0.156, 0.150, 0.148 ... ms per step).  Untimed steps until
    # `--warmup-ms` of device work have passed, so that no timed region sits on the ramp.
    extra = 0
    if args.warmup_ms > 0:
        t_w = time.perf_counter()
        eng.sync()
        while (time.perf_counter() - t_w) * 1e3 < args.warmup_ms and extra < 100000:
            for _ in range(8):
                eng.step(first)
                first += 1
                extra += 1
            eng.sync()
    reps, mine_reps = [], []
    n_rep = args.repeats if args.repeats > 0 else (max(5, -(-400 // max(1, args.steps))) if args.full else 1)
    # A few more untimed steps so that the last timed step converts buffer set 0 whatever the time-based warm-up ran: --dump-outputs then
    # writes the same frames in every run of the same arguments (the sets keep rotating in order, so no timed step finds its set in cache)
    while (first + n_rep * args.steps - 1) % eng.n_sets:
        eng.step(first)
        first += 1
        extra += 1
    eng.sync()
    for _ in range(n_rep):
        r, mine = region(args.steps, first)
        first += args.steps
        reps.append(r)
        mine_reps.append(mine)
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, output_arrays(eng.last_output(first - 1)))
        log(f"--dump-outputs: {', '.join(dumped)} -> {args.dump_outputs}")
    # Parity gate (--full): the output the LAST TIMED STEP left in its buffer set against the oracle (rank 0; the other ranks run the same code
    # on their own frames).  After the timed region, so the oracle's CPU time is never inside it.
    parity_fail = False
    if not stub and rank == 0:
        if not args.full:
            eng.parity = "not checked (the oracle parity gate runs with --full)"
        elif args.no_parity:
            eng.parity = "skipped (--no-parity)"
        elif args.alias:
            eng.parity = "skipped (aliased diagnostic buffers)"
        else:
            ok, eng.parity = eng.check_parity(first - 1)
            parity_fail = not ok
    if parity_fail:
        print(json.dumps({"error": "parity gate failed on the timed launch's own output", "workload": name}), file=sys.stderr, flush=True)
        os._exit(2)  # no line at all: a fast wrong kernel is not a measurement (os._exit: the other ranks sit in a barrier)
    # per-rank rate of the median repeat (min / max over ranks), N > 1 only
    order = sorted(range(len(reps)), key=lambda k: reps[k][0])
    med = order[len(order) // 2]
    wall, dev_ms, host_issue = reps[med]
    per_rank = None
    if dist is not None:
        rates = gather(B * args.steps / mine_reps[med][0])
        issue = gather(mine_reps[med][2] * 1e3 / args.steps)
        # every rank's own roofline fraction (its launch stream's HIP events): a slow GPU or a host-bound rank shows here, not in the max-over-ranks wall clock
        fracs = gather(bytes_per_frame * eng.frames_per_launch / (mine_reps[med][1] / (args.steps * eng.launches_per_step) * 1e-3) / 1e9 / HBM_PEAK_GBS if mine_reps[med][1] > 0 else 0.0)
        per_rank = {"min_frames_per_s": round(min(rates), 1), "max_frames_per_s": round(max(rates), 1),
                    "frames_per_s": [round(x, 1) for x in rates], "roofline_frac": [round(x, 4) for x in fracs],
                    "host_issue_ms_per_step": [round(x, 4) for x in issue],
                    "setup_s": [round(x, 3) for x in gather(setup_s)], "rank0_setup_steps": setup_log,
                    "backend": backend, "rank0_affinity": affinity}

    # Side measurements (outside the timed region, every rank takes part, same barrier / max-over-ranks bracket): the
    # headline's other three resize types (BASELINE.json's metric names none: SURVEY.md 8d "report all four") and the 4K
    # configurations C4 / C5 (north_star: "1080p and 4K ... at 1/2/4/8 GPUs").
    def all_ranks_ok(ok):
        """A side leg runs on every rank or on none: a rank that failed to set it up (an allocation, say) must not leave the others in a barrier."""
        if dist is None:
            return ok
        import torch
        t = torch.tensor([1.0 if ok else 0.0], dtype=torch.float64, device="cpu" if stub else "cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return bool(t.item() > 0.5)

    def side(sp, steps=20, wl_name=None):
        w, err = None, None
        try:
            sb, stab = DEFAULT_BATCH.get(wl_name, (None, False)) if wl_name else (None, False)
            w = eng.side_work(sp, batch=sb, table=stab)
        except Exception as e:
            err = f"{type(e).__name__}: {e}"
        if not all_ranks_ok(w is not None):
            return {"error": err or "another rank could not set this leg up"}
        try:
            # the device idles while rank 0 runs the oracle of the previous leg's parity check: each side leg starts with its own time-based
            # warm-up (the clock ramp, see --warmup-ms), or its 20 steps would sit on the ramp (first run of round 4: BICUBIC 0.54 instead of 0.63)
            t_w = time.perf_counter()
            k = 0
            while k < 3 or (args.warmup_ms > 0 and (time.perf_counter() - t_w) * 1e3 < args.warmup_ms and k < 100000):
                for _ in range(4):
                    w.issue(k, eng.cur_stream)
                    k += 1
                eng.sync()
            (sw, sdev, _), _ = region(steps, 0, w)
            bpf = bytes_of(sp)
            ms = sdev / (steps * w.launches_per_step)
            r = {"frames_per_s": round(w.B * steps * world / sw, 1), "avg_launch_ms": round(ms, 5), "frames_per_launch": w.frames_per_launch,
                 "hbm_frac": round(bpf * w.frames_per_launch / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
            if rank == 0 and wl_name:  # sparse samplers are priced on the bytes they move (see roofline.frac_basis), never > 1
                tbs = touched_bytes(sp)
                if tbs < 0.9 * bpf:
                    wbs = int(roi_and_dst(sp[0], sp[1], sp[3], sp[4])[2] * roi_and_dst(sp[0], sp[1], sp[3], sp[4])[3] * 3) * (4 if sp[8] else 1)
                    trs, _ = lookup_traffic(wl_name, w.frames_per_launch, alg_read=(bpf - wbs) * w.frames_per_launch, alg_write=wbs * w.frames_per_launch,
                                            touched_read=(tbs - wbs) * w.frames_per_launch)
                    moved = trs if trs else tbs * w.frames_per_launch
                    r["roi_frac"] = r["hbm_frac"]
                    r["hbm_frac"] = round(moved / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                    r["frac_basis"] = "PMC traffic" if trs else "touched bytes (lower bound of the bytes moved)"
            if rank == 0 and not args.no_parity and not stub:
                ok, r["parity"] = eng.check_parity(steps - 1, w)
                if not ok:
                    r = {"error": "MISMATCH vs oracle on the timed launch's own output", "avg_launch_ms": r["avg_launch_ms"]}
            del w
            return r
        except Exception as e:  # a side leg must never swallow the line
            return {"error": f"{type(e).__name__}: {e}"}

    others, other_wl = None, None
    if args.full and (not stub or dist is not None) and name == "headline" and not args.resize and not args.no_others and not args.consumers:
        others = {}
        for rname in ("NEAREST", "BICUBIC", "AREA"):
            sp = list(spec)
            sp[5] = rname
            others[rname] = side(tuple(sp))
        other_wl = {}
        for wl in ("c1", "c2", "c3", "c4", "c5"):  # every BASELINE configuration rides along in the default line (C3 / C4 out of persistent frame tables: DEFAULT_BATCH)
            other_wl[wl] = side(WORKLOADS[wl], wl_name=wl)

    if rank == 0:
        frames = B * args.steps * world
        kernel_ms = dev_ms / (args.steps * eng.launches_per_step)  # avg launch duration from HIP events
        fpl = eng.frames_per_launch
        achieved = bytes_per_frame * fpl / (kernel_ms * 1e-3) / 1e9
        total_steps = args.steps * len(reps)
        mean_wall = sum(r[0] for r in reps) / total_steps
        res = {
            "metric": metric_name(name, args.resize),
            "value": round(frames / wall, 1), "unit": "frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "warmup_steps_total": args.warmup + extra,  # `warmup` echoes W; the time-based warm-up (--warmup-ms) runs untimed steps on top of it
            "ms_per_step": round(wall * 1e3 / args.steps, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32" if norm else "u8", "data": "stub" if stub else "synthetic",
            "config": {"workload": f"{src_w}x{src_h} NV12 (pitch {pitch}) crop{list(crop)} -> {dst[0] or src_w}x{dst[1] or src_h} "
                                   f"{rt if dst[0] else 'no-resize'} -> {fcc} {planes} {'fp32 /255' if norm else 'uint8'}",
                       "name": name, "frames_per_step": B, "frames_per_launch": fpl, "hip_graph": bool(eng.graphs), "frame_table": bool(getattr(args, "table", False)),
                       "buffer_sets": args.sets, "working_set_MiB": round(eng.ws_mib, 1), "sharding": f"frames/{world} ranks, no data collective",
                       "parity": eng.parity},
            "timing": {"repeats": len(reps), "reported": "median repeat (max over ranks per repeat)",
                       "total_timed_steps": total_steps, "mean_ms_per_step": round(mean_wall * 1e3, 4),
                       "max_ms_per_step": round(max(r[0] for r in reps) * 1e3 / args.steps, 4),
                       "warmup_steps_total": args.warmup + extra, "warmup_ms": args.warmup_ms, "setup_s": setup_s,
                       "repeats_ms_per_step": [round(r[0] * 1e3 / args.steps, 4) for r in reps],
                       "repeats_avg_launch_ms": [round(r[1] / (args.steps * eng.launches_per_step), 5) for r in reps]},
            "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": None,
                         "kernel": eng.kernel_name() if not stub else "stub", "bytes_per_frame": bytes_per_frame,
                         "avg_launch_ms": round(kernel_ms, 5), "host_issue_ms_per_step": round(host_issue * 1e3 / args.steps, 4)},
        }
        if args.consumers:
            # the rank's consumers convert the SAME published frame (that IS C5's shape: consumers of one stream): its source bytes leave HBM once per step, the rest are cache hits --
            # `frac` (ROI formula per conversion) says how well the entry keeps the GPU fed, `shared_source_frac` prices the bytes that really move (one source frame + every output)
            src_b = bytes_per_frame - write_bytes_per_frame
            res["roofline"]["shared_source_frac"] = round((src_b + eng.n * write_bytes_per_frame) / (kernel_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
            res["config"]["consumers"] = {"total": args.consumers, "per_rank": eng.n, "entry": "TensorStreamConverter.read_many (one batched launch per published frame)",
                                          "names_rank0": [eng.names[0], eng.names[-1]], "sharding": "consumer c -> rank c // (consumers / world): each rank its own converter, source and stream pool"}
        if per_rank:
            res["per_rank"] = per_rank
        if dist is not None and not stub:
            res["config"]["coeff_broadcast"] = eng.coeff_broadcast
        if args.alias:  # not a measurement of the path: the frames of a launch share buffers
            res["data"] = "DIAGNOSTIC: aliased buffers (--alias %d)" % args.alias
        if args.streams > 1:  # not the contract's measurement: launches of several streams overlap, avg_launch_ms / roofline are wall time per launch
            res["data"] = "DIAGNOSTIC: steps issued round-robin on %d streams (--streams): roofline figures are per launch of WALL time, not launch durations" % args.streams
        rf = res["roofline"]
        rf["write_bytes_per_frame"] = write_bytes_per_frame
        tb = None
        try:  # touched_bytes: distinct source bytes with a non-zero weight + output bytes
            tb = touched_bytes(spec)
            rf["touched_bytes"] = tb
            rf["touched_frac"] = round(tb * fpl / (kernel_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        except Exception as e:
            rf["touched_bytes"] = {"error": f"{type(e).__name__}: {e}"}
        tr = None
        try:
            tr, why = lookup_traffic(name if not args.resize else (args.resize.lower() if name == "headline" else ""), fpl, kernel=rf["kernel"],
                                     alg_read=(bytes_per_frame - write_bytes_per_frame) * fpl, alg_write=write_bytes_per_frame * fpl,
                                     touched_read=(tb - write_bytes_per_frame) * fpl if tb is not None else None)
            rf["traffic"] = tr
            rf["traffic_source"] = why
            if tr:  # the fraction of the peak on the bytes the launch actually moved
                rf["traffic_frac"] = round(tr / (kernel_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        except Exception as e:
            rf["traffic_source"] = f"error: {type(e).__name__}: {e}"
        # A sampler that skips source bytes (C3: BILINEAR at 5 x 2.8, C4: BICUBIC at ratio 3 = a point sample of a third of the rows)
        # moves far fewer bytes than the ROI formula counts; priced on the ROI its "fraction" exceeds 1 (round 3 printed 1.33).  For
        # those launches `achieved` / `frac` are on the bytes REALLY moved -- the PMC traffic when a fresh entry exists, else the touched
        # bytes (a lower bound of the traffic: whole cache lines are fetched) -- and the ROI-formula figure stays as `roi_frac`.
        if tb is not None and tb < 0.9 * bytes_per_frame:
            rf["roi_achieved"], rf["roi_frac"] = rf["achieved"], rf["frac"]
            moved = tr if tr else tb * fpl
            rf["achieved"] = round(moved / (kernel_ms * 1e-3) / 1e9, 1)
            rf["frac"] = round(rf["achieved"] / HBM_PEAK_GBS, 4)
            rf["frac_basis"] = ("PMC traffic per launch (sparse sampler: the ROI formula counts source bytes the kernel never fetches)" if tr else
                                "touched bytes (sparse sampler, no fresh PMC entry: a lower bound of the bytes moved)")
        else:
            rf["frac_basis"] = "algorithmic bytes (ROI formula, SURVEY.md 8d)"
        if others is not None and world == 1 and not stub:
            try:
                res["config"]["facade"] = facade_leg(0)
            except Exception as e:
                res["config"]["facade"] = {"error": f"{type(e).__name__}: {e}"}
            try:
                res["config"]["latency"] = latency_leg(spec)
            except Exception as e:
                res["config"]["latency"] = {"error": f"{type(e).__name__}: {e}"}
            try:
                res["config"]["launch_curve"] = launch_curve_leg()
            except Exception as e:
                res["config"]["launch_curve"] = {"error": f"{type(e).__name__}: {e}"}
        if others is not None:
            res["config"]["other_resize_types"] = others
        if other_wl is not None:
            res["config"]["other_workloads"] = other_wl
        # (round 6) N > 1 lines carry it too: rank 0 measures it here, after every timed region, while the other ranks wait in the final barrier
        if dumped is not None:
            res["config"]["dump_outputs"] = dumped
        if args.full and not args.no_cpu_baseline:
            try:
                res["cpu_baseline"] = cpu_baseline(spec, budget_s=(min(args.cpu_budget, 0.3) if stub else args.cpu_budget), tight_pitch=args.tight_pitch)
            except Exception as e:
                res["cpu_baseline"] = {"error": f"{type(e).__name__}: {e}", "swscale": "unavailable in image"}
        if out_fd is not None:
            sys.stdout.flush()
            os.write(out_fd, (json.dumps(res) + "\n").encode())
        else:
            print(json.dumps(res), flush=True)
    eng.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse_args(argv)
    if args.curve_only:
        print(json.dumps(launch_curve_leg(tuple(args.curve_only.split(",")), parity=not args.no_parity)), flush=True)
        return 0
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return spawn(args, argv)
    return run(args)


if __name__ == "__main__":
    sys.exit(main())
