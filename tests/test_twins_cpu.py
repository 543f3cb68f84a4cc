"""No GPU: `vpp_twins --host` (tensor-stream_amd/cpp/vpp_twins.cpp) -- the host compile of csrc's AREA weight generator (roi_area_step, roi_area_weight) and of
the jump-start search (lb_area_period, lb_area_chain_start), built with csrc's flags outside the library, against the C ABI the CPU tests pin to the oracle
(tsvpp_roi_area_rows, tsvpp_letterbox_area_rows): 213 scales, raw bits.  The mode touches no HIP runtime call; tests/test_cpp_twins_gpu.py runs the device half."""
import os

from cpp_check import run_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tensor-stream_amd", "lib", "vpp_twins")
SCALES, SUBSETS, ROWS, FIRSTS = 13 + 200, 3, 32, 12
HOST_GROUPS = {"host_weights": SCALES * SUBSETS * ROWS, "host_period": SCALES * FIRSTS * 2}  # name -> cases


def groups(stdout):
    """name -> (cases, mismatches, first mismatch) of the program's lines"""
    out = {}
    for ln in stdout.splitlines():
        parts = ln.split(" ", 3)
        if len(parts) == 4 and parts[1].isdigit() and parts[2].isdigit():  # (run_check hands over the end of the output: its first line may be cut)
            out[parts[0]] = (int(parts[1]), int(parts[2]), parts[3])
    return out


def test_the_host_compile_matches_the_c_abi():
    assert os.path.exists(EXE), "vpp_twins not built (python -c 'import __graft_entry__ as g; g.build()')"
    rc, _, tails = run_check([EXE, "--host"])
    got = groups(tails[0])
    assert rc == 0 and set(got) == set(HOST_GROUPS), (rc, *tails)
    for name, cases in HOST_GROUPS.items():
        assert got[name] == (cases, 0, "-"), (name, got[name])
