"""GPU: `vpp_twins` (tensor-stream_amd/cpp/vpp_twins.cpp), once -- the DEVICE compile of csrc's AREA weight generator and of the jump-start search, which the rest
of the suite sees only through 8-bit outputs, against the host compile and the C ABI, raw bits: every RoiAreaRow record of 4096 indices of 213 scales, the
expanded rows at indices 0, 1000 and 4064, lb_area_period's ballot search on every lane of a full wave at twelve first indices up to 65535, and the rows a chain
begun at the device's own jump start produces against the chain from 0."""
import os

import pytest

from cpp_check import run_check
from test_twins_cpu import EXE, FIRSTS, HOST_GROUPS, ROWS, SCALES, SUBSETS, groups

pytestmark = pytest.mark.gpu

INDICES = 4096
GROUPS = dict(HOST_GROUPS, gen_rows=SCALES * INDICES, gen_weights=SCALES * SUBSETS * ROWS, period=SCALES * FIRSTS,
              jump_rows=SCALES * ((FIRSTS - 1) * ROWS + 1))  # (first = 65535 has one row in front of the header's limit of 65536)


def test_the_device_compile_matches_the_host_and_the_c_abi():
    assert os.path.exists(EXE), "vpp_twins not built (python -c 'import __graft_entry__ as g; g.build()')"
    rc, _, tails = run_check([EXE])
    got = groups(tails[0])
    assert rc == 0 and set(got) == set(GROUPS), (rc, *tails)
    for name, cases in GROUPS.items():
        assert got[name] == (cases, 0, "-"), (name, got[name])
