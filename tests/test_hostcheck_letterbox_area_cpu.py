"""CPU: the host side of tsvpp_convert_letterbox_area under AddressSanitizer + UndefinedBehaviorSanitizer, against the stub HIP runtime of tests/hostcheck/.

tests/hostcheck/letterbox_area.mk includes the existing Makefile and adds one link rule: hc_letterbox_area, a stand-alone program (its own main) from the same
sanitized objects of the library, the VideoProcessor adapter and stub_hip.o.  It sends its requests -- plain and tensor forms, 33 frames, the caller's rectangles,
a narrow canvas -- through describe and convert, on a capturing stream and with an allocation failing at every depth (the path allocates nothing), through every
refusal, and through the adapter's two methods, which must launch what the entry point launches.  Launches are recorded and range-checked by the stub, never
executed.  Nothing is preloaded, nothing runs through Python under a sanitizer, no device code is built."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HC = os.path.join(HERE, "hostcheck")
EXE = os.path.join(ROOT, "tensor-stream_amd", "lib", "hostcheck", "asan", "hc_letterbox_area")


def test_letterbox_area_under_asan_ubsan():
    r = subprocess.run(["make", "-s", "-C", HC, "-f", "letterbox_area.mk", "-j16", "letterbox_area"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, f"tests/hostcheck/letterbox_area.mk does not build:\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    r = subprocess.run(["timeout", "-k", "5", "300", EXE], capture_output=True, text=True, timeout=330)
    tail = (r.stdout[-2000:] + "\n" + r.stderr[-12000:]).strip()
    assert r.returncode == 0, f"hc_letterbox_area ended with status {r.returncode}:\n{tail}"
    assert re.search(r"hc_letterbox_area: \d+ assertions, 0 failed", r.stderr) and "hc_letterbox_area: 7 requests, 3 through the adapter" in r.stderr, tail
