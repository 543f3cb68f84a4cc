"""CPU: the host library under sanitizers, against a stub HIP runtime (tests/hostcheck/).

libtsvpp's host side (every translation unit of csrc/Makefile's SRCS, compiled host-only: no device code) and the VideoProcessor adapter are built twice -- with
AddressSanitizer + UndefinedBehaviorSanitizer and with ThreadSanitizer -- and linked with tests/hostcheck/stub_hip.cpp, a CPU stand-in for the 23 runtime functions
and 5 registration hooks the library needs, into three stand-alone programs.  Launches are recorded and checked, never executed; "device" memory is heap memory the
sanitizer watches.  Nothing here needs a GPU, nothing is loaded into Python under a sanitizer.

  hc_requests   one thread: every selection signature of tests/dispatch_grid.py, chunk 0 of every family of tests/tile_fuzz.py and a handful of remap / mesh requests
                through describe, convert, the replay hit, the other alignment class, a frame table, prepare and trim; the helper entry points and their refusals;
                allocation failures at every depth
  hc_threads    eight threads doing what include/tsvpp.h allows concurrently (ThreadSanitizer, and again under AddressSanitizer)
  hc_capture    the library's behaviour on a stream that is being captured into a graph

The requests come from the generators the suite already has: this file writes them into a text file the driver reads."""
import os
import re
import struct
import subprocess
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HC = os.path.join(HERE, "hostcheck")
OUT = os.path.join(ROOT, "tensor-stream_amd", "lib", "hostcheck")

# include/tsvpp.h's host side calls these and no other function of the runtime (tests/hostcheck/stub_hip.cpp implements exactly them)
RUNTIME = {"hipLaunchKernel", "hipExtLaunchKernel", "hipGetLastError", "hipGetErrorString", "hipGetDevice", "hipSetDevice", "hipGetDeviceCount",
           "hipGetDevicePropertiesR0600", "hipStreamCreate", "hipStreamDestroy", "hipStreamSynchronize", "hipStreamIsCapturing", "hipMalloc", "hipFree",
           "hipHostMalloc", "hipHostFree", "hipMemcpy", "hipMemcpyAsync", "hipMemset", "hipEventCreateWithFlags", "hipEventDestroy", "hipEventRecord",
           "hipEventSynchronize"}
HOOKS = {"__hipRegisterFatBinary", "__hipRegisterFunction", "__hipUnregisterFatBinary", "__hipPushCallConfiguration", "__hipPopCallConfiguration"}
IS_RUNTIME = re.compile(r"^(hip[A-Z]\w*|__hip(?!_fatbin)\w+)$")


@pytest.fixture(scope="module")
def built():
    """both flavours, at most 16 jobs; the seconds it took"""
    t0 = time.perf_counter()
    r = subprocess.run(["make", "-s", "-C", HC, "-j16"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, f"tests/hostcheck does not build:\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    seconds = time.perf_counter() - t0
    print(f"hostcheck: both flavours built in {seconds:.1f} s")
    return seconds


def _run(exe, *args, limit):
    """the driver as a child process under its own time limit; its report in the assertion message"""
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "5", str(limit), exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=limit + 30)
    seconds = time.perf_counter() - t0
    tail = (r.stdout[-2000:] + "\n" + r.stderr[-12000:]).strip()
    print(f"{os.path.basename(exe)} ({os.path.basename(os.path.dirname(exe))}): {seconds:.1f} s\n" + "\n".join(tail.splitlines()[-4:]))
    assert r.returncode == 0, f"{exe} {' '.join(str(a) for a in args)} ended with status {r.returncode} after {seconds:.1f} s:\n{tail}"
    return r


# ---- the request file ---------------------------------------------------------------------------------------------------------------------------------------------

def _hex(v):
    """the bits of v as a float32, eight hex digits"""
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(np.float32(v))))[0]


def _hex_bits(a):
    return " ".join("%08x" % b for b in np.ascontiguousarray(a, np.float32).view(np.uint32).ravel())


def _plain_lines():
    import dispatch_grid as G
    for sig in sorted(G.signatures()):
        src, crop, dst, rt, fcc, planes, norm, n, aligned = G.representative(sig)
        yield "plain " + " ".join(str(int(v)) for v in (*src, *crop, *dst, rt, fcc, planes, norm, n, aligned))


def _tile_lines():
    import tensor_util as T
    import tile_fuzz as F
    for family in F.FAMILIES:
        for call in F.cases(family, 0):
            fcc, planes, norm = call["flavour"]
            if call["tensor"] is None:
                dtype, mean, scale = -1, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
            else:
                dtype, (mean, std) = T.CODE[call["tensor"][0]], T.SPECS[call["tensor"][1]]
                scale = T.scales(std)
            abc = call.get("pad") or call.get("border") or (-1, -1, -1)
            out = ["tile", family, call["rt"], fcc, planes, int(bool(norm)), dtype, *[_hex(m) for m in mean], *[_hex(s) for s in scale], *call["dst"], *abc,
                   int(call["placement"] != "unaligned"), len(call["frames"])]
            for f in call["frames"]:
                out += [f["w"], f["h"], f["pitch_y"], f["pitch_uv"], f["off_y"], f["off_uv"]]
            starts, total = F.slot_starts(call)
            out += [total, len(call["items"])]
            for start, item in zip(starts, call["items"]):
                out += [start, item[0]]
                if family in ("rois", "rois_area"):
                    out += list(item[1:])
                elif family == "letterbox":
                    out += [0, 0, 0, 0, 0] if item[1] is None else [1, *item[1]]
                else:
                    out += [_hex(v) for v in item[1:]]
            yield " ".join(str(v) for v in out)


def _map_lines():
    """a handful: every kind of map / mesh of the GPU tests' sets on one small geometry, with and without pitch padding, an LDS hint, a border, a Y800 output"""
    import mesh_util as M
    import remap_util as R
    w, h, dw, dh = 96, 64, 48, 32
    for i, (name, xy) in enumerate(sorted(R.map_set(w, h, dw, dh, seed=3).items())):
        fcc, planes, norm = ((1, 0, 1), (2, 1, 0), (0, 0, 0))[i % 3]
        border = (-1, -1, -1) if i % 2 else (16, 128, 128)
        pitch = 0 if i % 3 else 8 * dw + 48
        yield f"remap {w} {h} {dw} {dh} {fcc} {planes} {norm} {border[0]} {border[1]} {border[2]} {pitch} {2048 * (i % 2)} {1 + 16 * (i % 3)} {xy.size} " + _hex_bits(xy)
    for i, cell in enumerate(((4, 4), (16, 8), (32, 32))):
        rows, cols = M.dims(dw, dh, cell)
        for j, (name, mesh) in enumerate(sorted(M.mesh_set(w, h, dw, dh, cell, seed=5).items())):
            fcc, planes, norm = ((1, 0, 1), (0, 0, 1), (2, 1, 0))[j % 3]
            border = (-1, -1, -1) if j % 2 else (0, 128, 128)
            pitch = 0 if (i + j) % 2 else 8 * cols + 16
            assert mesh.shape == (rows, cols, 2), (mesh.shape, rows, cols)
            yield (f"mesh {w} {h} {dw} {dh} {M.log2(cell[0])} {M.log2(cell[1])} {fcc} {planes} {norm} {border[0]} {border[1]} {border[2]} {pitch} {1024 * (j % 2)} "
                   f"{1 + 33 * (j % 2)} {mesh.size} " + _hex_bits(mesh))


@pytest.fixture(scope="module")
def request_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("hostcheck") / "requests.txt"
    counts = {}
    with open(path, "w") as f:
        for gen in (_plain_lines, _tile_lines, _map_lines):
            for line in gen():
                f.write(line + "\n")
                counts[line.split(" ", 1)[0]] = counts.get(line.split(" ", 1)[0], 0) + 1
    print(f"hostcheck: request file {counts}")
    assert counts["plain"] >= 1000 and counts["tile"] == 5 * 24 and counts["remap"] >= 8 and counts["mesh"] >= 12, counts
    return str(path)


# ---- the tests ------------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_stub_implements_exactly_what_the_library_calls(built):
    """the undefined hip* symbols of the sanitized objects are the stub's list: a new HIP call in the library fails the drivers' link, and this test says which"""
    srcs = re.search(r"^SRCS := (.*)$", open(os.path.join(ROOT, "tensor-stream_amd", "csrc", "Makefile")).read(), re.M).group(1).split()
    assert len(srcs) >= 37, srcs
    for flavour in ("asan", "tsan"):
        objs = [os.path.join(OUT, flavour, "obj", os.path.splitext(s)[0] + ".o") for s in srcs]
        undefined = subprocess.run(["nm", "-u", *objs], capture_output=True, text=True, check=True).stdout
        wanted = {m for m in (line.split()[-1] for line in undefined.splitlines() if line.strip().startswith("U ")) if IS_RUNTIME.match(m)}
        defined = subprocess.run(["nm", "--defined-only", os.path.join(OUT, flavour, "obj", "stub_hip.o")], capture_output=True, text=True, check=True).stdout
        have = {m for m in (line.split()[-1] for line in defined.splitlines() if " T " in line) if IS_RUNTIME.match(m)}
        assert wanted == have, f"{flavour}: the library calls {sorted(wanted - have)} which the stub lacks; the stub implements {sorted(have - wanted)} which nobody calls"
        assert have == RUNTIME | HOOKS, (sorted(have - RUNTIME - HOOKS), sorted((RUNTIME | HOOKS) - have))


def test_requests_under_asan_ubsan(built, request_file):
    r = _run(os.path.join(OUT, "asan", "hc_requests"), request_file, limit=600)
    assert re.search(r"hc_requests: \d+ assertions, 0 failed", r.stderr), r.stderr[-2000:]


def test_capture_under_asan_ubsan(built):
    r = _run(os.path.join(OUT, "asan", "hc_capture"), limit=120)
    assert re.search(r"hc_capture: \d+ assertions, 0 failed", r.stderr), r.stderr[-2000:]


@pytest.mark.parametrize("flavour", ["tsan", "asan"])
def test_threads(built, flavour):
    r = _run(os.path.join(OUT, flavour, "hc_threads"), 2000, limit=240)
    assert re.search(r"hc_threads: \d+ assertions, 0 failed", r.stderr), r.stderr[-2000:]
