"""CPU: the fifteen tile methods of the VideoProcessor adapter under AddressSanitizer + UndefinedBehaviorSanitizer, against the stub HIP runtime of tests/hostcheck/.

tests/hostcheck/adapter.mk includes the existing Makefile and adds one link rule: hc_adapter, a stand-alone program (its own main) from the sanitized objects of the
library, stub_hip.o, stub_hip_vp.o and VideoProcessor.o, as hc_threads links them.  For every method it compares the stub's launch log with the one of the
tsvpp_convert_* entry point called directly -- on the consumer's FIRST stream, with the same frames, items, parameters, spec, border or pad, and outputs --, then
sends every request the method's own guard refuses (VREADER_ERROR, no launch) and the one the library refuses (its status, unchanged), and ends with Close() leaving
nothing behind.  Launches are recorded and range-checked by the stub, never executed.  Nothing is preloaded, nothing runs through Python under a sanitizer, no device
code is built."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HC = os.path.join(HERE, "hostcheck")
EXE = os.path.join(ROOT, "tensor-stream_amd", "lib", "hostcheck", "asan", "hc_adapter")


def test_tile_methods_under_asan_ubsan():
    r = subprocess.run(["make", "-s", "-C", HC, "-f", "adapter.mk", "-j16", "adapter"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, f"tests/hostcheck/adapter.mk does not build:\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    r = subprocess.run(["timeout", "-k", "5", "300", EXE], capture_output=True, text=True, timeout=330)
    tail = (r.stdout[-2000:] + "\n" + r.stderr[-12000:]).strip()
    assert r.returncode == 0, f"hc_adapter ended with status {r.returncode}:\n{tail}"
    assert re.search(r"hc_adapter: \d+ assertions, 0 failed", r.stderr), tail
