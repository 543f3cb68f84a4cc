"""CPU: the host side of tsvpp_convert_warp_bicubic and tsvpp_convert_perspective_bicubic under AddressSanitizer + UndefinedBehaviorSanitizer, against the stub
HIP runtime of tests/hostcheck/.

tests/hostcheck/coord_bicubic.mk includes the existing Makefile and adds one link rule: hc_coord_bicubic, a stand-alone program (its own main) from the same
sanitized objects of the library, the VideoProcessor adapter and stub_hip.o.  It sends its requests -- both calls, plain and with a tensor spec, 33 outputs (two
launches), frames down to 4 x 2, a narrow output -- through describe and convert, on a capturing stream and with an allocation failing at every depth (the paths
allocate nothing), through every refusal, through the footprint exports, and through the adapter's four methods, which must launch what the entry points launch.
Launches are recorded and range-checked by the stub, never executed.  Nothing is preloaded, nothing runs through Python under a sanitizer, no device code is built."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HC = os.path.join(HERE, "hostcheck")
EXE = os.path.join(ROOT, "tensor-stream_amd", "lib", "hostcheck", "asan", "hc_coord_bicubic")


def test_coord_bicubic_under_asan_ubsan():
    r = subprocess.run(["make", "-s", "-C", HC, "-f", "coord_bicubic.mk", "-j16", "coord_bicubic"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, f"tests/hostcheck/coord_bicubic.mk does not build:\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    r = subprocess.run(["timeout", "-k", "5", "300", EXE], capture_output=True, text=True, timeout=330)
    tail = (r.stdout[-2000:] + "\n" + r.stderr[-12000:]).strip()
    assert r.returncode == 0, f"hc_coord_bicubic ended with status {r.returncode}:\n{tail}"
    assert re.search(r"hc_coord_bicubic: \d+ assertions, 0 failed", r.stderr) and "hc_coord_bicubic: 9 requests, 4 through the adapter" in r.stderr, tail
