"""What the tests of the C++ check programs (tensor-stream_amd/cpp/vpp_*.cpp, tests/test_cpp_*_gpu.py) share: the frame file a program reads, and one run of a
program.  The assertions stay with the tests."""
import subprocess


def write_nv12(path, y, uv):
    """The file a check program reads: the luma rows at their pitch, then the chroma rows."""
    with open(path, "wb") as f:
        f.write(y.tobytes())
        f.write(uv.tobytes())


def run_check(args):
    """Runs a check program.  Returns its return code, its output lines that begin with a digit -- one per output: index, CRC, bytes and whatever the program
    appends -- split into fields, and the ends of stdout and stderr for an assertion's message."""
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    lines = [ln.split() for ln in r.stdout.splitlines() if ln and ln[0].isdigit()]
    return r.returncode, lines, (r.stdout[-1000:], r.stderr[-2000:])
