"""Device-free checks of the per-person de novo posteriors: the CLI's argument errors (raised while the command line is
parsed: before the pedigree is read or an engine created), the CPU driver's refusal of the flag, the pm_person_dn
layout and the new symbols under an unchanged ABI version, and the register-resident founder / nuclear instantiation
of k_person_dn read from the built gfx950 code object."""
import ctypes as C
import subprocess

import pytest

import polymutt_amd as pm
from conftest import EXAMPLE
from test_cpu_kernel_resources import _resources

BASE = ["-p", "test.ped", "-d", "test.dat", "-g", "test.gif", "--out_vcf"]


@pytest.mark.parametrize("extra,message", [
    (["--denovo_carriers", "2"], "--denovo_carriers needs --denovo"),
    (["--denovo", "--in_vcf", "testvcf.in.vcf.gz", "--denovo_carriers", "2"], "--denovo_carriers is not available with --in_vcf"),
    (["--denovo", "--denovo_carriers", "0"], "--denovo_carriers takes a person count from 1 to 8"),
    (["--denovo", "--denovo_carriers=9"], "--denovo_carriers takes a person count from 1 to 8"),
])
def test_cli_argument_errors(built, tmp_path, extra, message):
    out = tmp_path / "out.vcf"
    r = subprocess.run([pm.BIN_PATH] + BASE + [str(out)] + extra, cwd=EXAMPLE, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, r.stdout[-1000:] + r.stderr[-1000:]
    assert "FATAL ERROR" in r.stdout and message in r.stdout, r.stdout[-1000:]
    assert not out.exists()


def test_cpu_evaluator_refuses_the_flag(cpu_driver, tmp_path):
    """The host driver on another evaluator (the CPU oracle's) ends with the SiteEvaluator default's message."""
    out = tmp_path / "out.vcf"
    r = subprocess.run([cpu_driver] + BASE + [str(out), "--denovo", "--denovo_carriers", "2"], cwd=EXAMPLE,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--denovo_carriers needs the GPU engine" in r.stdout, r.stdout[-1000:]


def test_abi_and_layout(built):
    lib = pm.load_library()
    assert lib.pm_abi_version() == 8   # additive: callers detect the feature by the symbols
    dt = pm.PERSON_DN_DTYPE
    assert dt is pm.engine.PERSON_DN_DTYPE and dt.itemsize == 16
    assert [dt.fields[f][1] for f in ("person", "fa_g", "mo_g", "kid_g", "pad", "pp")] == [0, 4, 5, 6, 7, 8]
    for name in ("pm_engine_set_denovo_carriers", "pm_engine_denovo_carriers"):
        assert name in pm.engine.EXPORTS and hasattr(C.CDLL(pm.LIB_PATH), name)


def test_person_kernel_keeps_founder_and_nuclear_families_in_registers():
    res = _resources()
    k = "void k_person_dn<false>(DevArgs, PersonDnArgs)"
    assert k in res and "void k_person_dn<true>(DevArgs, PersonDnArgs)" in res, [n for n in res if "person_dn" in n]
    assert int(res[k]["private_segment_fixed_size"]) == 0, res[k]
