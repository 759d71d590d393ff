"""Static instruction accounting of k_brent's Brent loop (tools/isa_mix.py; cross-compiles to gfx950 assembly, no GPU).

Guards what shortening the evaluation's serial path removed ("k_brent in detail"): inside the Brent
loop no kernel argument is re-loaded -- the only scalar load left is the log10 table entry's, one dependent
s_load_dwordx4 from constant memory, in the flavours that keep that form (the QUAD kernels read the entry from LDS: no
scalar load at all) -- the loop's static VALU count stays at or below the value recorded when the path was shortened,
and the kernels keep every value in registers.  The earlier path (-DPM_SERIAL_V0=1) held 355 VALU and
three scalar loads (A.itmax, A.precision, the table entry) in the headline instantiation's loop with this toolchain."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# instantiation: the Brent loop's static VALU count of the build that shortened the path (the cap)
VALU_CAP = {"headline": 344, "plain128": 368}


@pytest.fixture(scope="module")
def mixes():
    isa_mix = pytest.importorskip("isa_mix")
    if not os.path.exists(isa_mix.HIPCC):
        pytest.skip("hipcc not available")
    return {n: isa_mix.account(isa_mix.NAMES[n], []) for n in VALU_CAP}


@pytest.mark.parametrize("name", sorted(VALU_CAP))
def test_brent_loop_reloads_no_argument(mixes, name):
    loads = mixes[name]["brent_loop"]["s_load_lines"]
    # the table entry: two doubles at a computed address (never the kernel-argument segment, s[0:1])
    assert len(loads) <= 1, loads
    for l in loads:
        assert re.match(r"s_load_dwordx4 s\[\d+:\d+\], s\[(\d+):\d+\], 0x0$", l) and not re.search(r", s\[0:1\],", l), l


@pytest.mark.parametrize("name", sorted(VALU_CAP))
def test_brent_loop_valu_count_and_no_scratch(mixes, name):
    m = mixes[name]
    assert m["markers_neutral"], "the PM_ISA_MARK markers changed the instruction mix"
    assert m["brent_loop"]["valu"] <= VALU_CAP[name], (name, m["brent_loop"])
    assert m["resources"]["scratch"] == 0, m["resources"]
