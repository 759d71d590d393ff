"""The device numeric primitives, each alone on one block, against long double references on the host
(tests/native/num_check.hip, built by __graft_entry__.build()): pos_div within a bit-pattern step of the IEEE quotient;
log10_mant / log10_mant_u / log10_mant_pair within 2^-53 + 1 ulp at the table boundaries and ten exponents; the DPP wave
product and sum (one-hot lanes, 2^-256, a zero lane); block_logprod's double buffer at every block size; the family
quartic at all-255 / all-0 PL bytes in every fam_poly4 variant; lane_poly_r / lane_poly_top at x = 0.0001 and 0.9999 with
16 all-255 slots, five- and four-coefficient forms; es_poly_eval against es_poly_eval_r bit for bit; the Brent state
machine against the reference's loop bit for bit.  The bounds are derived in num_check.hip beside each section."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "build", "num_check")
SECTIONS = ["div", "log", "wave", "block", "quartic", "poly", "espoly", "brent"]


@pytest.mark.gpu
@pytest.mark.parametrize("section", SECTIONS)
def test_device_primitive_holds_its_bound(section):
    assert os.path.exists(EXE), "build num_check first (__graft_entry__.build())"
    r = subprocess.run([EXE, section], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert f"num_check {section}: " in r.stdout and " 0 mismatches" in r.stdout
