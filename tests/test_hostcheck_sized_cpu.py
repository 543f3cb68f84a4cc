"""CPU: the host side of tsvpp_convert_rois_sized under AddressSanitizer + UndefinedBehaviorSanitizer, against the stub HIP runtime of tests/hostcheck/.

tests/hostcheck/sized.mk includes the existing Makefile and adds one link rule: hc_sized, a stand-alone program (its own main) from the same sanitized objects of
the library and stub_hip.o.  It sends the seeded requests of tests/test_rois_sized_cpu.py's exact-cover test, a request of 97 boxes and three tensor forms through
describe and convert -- all outputs aligned, none, mixed (the two-class split) --, once on a capturing stream and once with the next allocation failing.  Launches are
recorded and range-checked by the stub, never executed.  Nothing is preloaded, nothing runs through Python under a sanitizer, no device code is built."""
import os
import re
import struct
import subprocess

import numpy as np

import rois_sized_util as U

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HC = os.path.join(HERE, "hostcheck")
EXE = os.path.join(ROOT, "tensor-stream_amd", "lib", "hostcheck", "asan", "hc_sized")


def _hex(v):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(np.float32(v))))[0]


def _line(frames, rois, rt, fcc, planes, norm, dtype=-1, mean=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0), seed=0):
    rng = np.random.default_rng(seed)
    out = ["sized", rt, fcc, planes, int(norm), dtype, *[_hex(m) for m in mean], *[_hex(s) for s in scale], len(frames)]
    for f in frames:
        out += [f[0], f[1], f[2]]
    out.append(len(rois))
    for r in rois:
        out += [*r, int(rng.integers(0, 2))]
    return " ".join(str(v) for v in out)


def _lines():
    flavours = U.FLAVOURS
    for s in range(20):  # the requests of test_every_workgroup_has_exactly_one_tile
        frames, rois = U.seeded_request(9000 + s)
        fcc, planes, norm = flavours[s % len(flavours)]
        yield _line(frames, rois, s % 3, fcc, planes, norm, seed=s)
    frames, rois = U.seeded_request(9100, n=97, max_side=64)  # three launches of a class, or four of two
    yield _line(frames, rois, U.BILINEAR, U.RGB24, U.MERGED, False, seed=97)
    for dtype, (fcc, planes) in enumerate([(U.BGR24, U.PLANAR), (U.Y800, U.MERGED), (U.RGB24, U.PLANAR)]):
        frames, rois = U.seeded_request(9200 + dtype)
        yield _line(frames, rois, U.BICUBIC, fcc, planes, True, dtype=dtype, mean=(0.485, 0.456, 0.406), scale=(4.0, 4.5, 5.0), seed=dtype)


def test_rois_sized_under_asan_ubsan(tmp_path):
    r = subprocess.run(["make", "-s", "-C", HC, "-f", "sized.mk", "-j16", "sized"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, f"tests/hostcheck/sized.mk does not build:\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    path = tmp_path / "sized_requests.txt"
    lines = list(_lines())
    assert len(lines) == 24
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["timeout", "-k", "5", "300", EXE, str(path)], capture_output=True, text=True, timeout=330)
    tail = (r.stdout[-2000:] + "\n" + r.stderr[-12000:]).strip()
    assert r.returncode == 0, f"hc_sized ended with status {r.returncode}:\n{tail}"
    assert re.search(r"hc_sized: \d+ assertions, 0 failed", r.stderr) and "hc_sized: 24 requests, 3 of them tensor forms" in r.stderr, tail
