"""Device-free checks of de novo calling from VCF input: the new symbol under an unchanged ABI version, the Python method,
the CLI's argument errors (raised while the command line is parsed: before the pedigree is read or an engine created), the
CPU driver's refusal of the flag, and the register-resident de novo Brent and finalize kernels read from the built gfx950
code object."""
import ctypes as C
import subprocess

import pytest

import polymutt_amd as pm
from conftest import EXAMPLE
from test_cpu_kernel_resources import _resources

BASE = ["-p", "test.ped", "-d", "test.dat", "--out_vcf"]

# config 5 (2000 mixed trio / quad families, 4000+ terms) runs the 256-thread de novo Brent kernel; small pedigrees the
# one-wave one
VDN_KERNELS = [
    "void k_vdn_brent<256>(DevArgs, VdnArgs)",
    "void k_vdn_brent<64>(DevArgs, VdnArgs)",
    "k_finalize_vdn(DevArgs)",
]


def test_symbol_and_method(built):
    lib = pm.load_library()
    assert lib.pm_abi_version() == 8   # additive: callers detect the feature by the symbol
    assert "pm_engine_set_vcf_denovo" in pm.engine.EXPORTS and hasattr(C.CDLL(pm.LIB_PATH), "pm_engine_set_vcf_denovo")
    assert callable(getattr(pm.Engine, "set_vcf_denovo"))


@pytest.mark.parametrize("extra,message", [
    (["-g", "test.gif", "--vcf_denovo"], "--vcf_denovo needs --in_vcf"),
    (["-g", "test.gif", "--denovo", "--vcf_denovo"], "--vcf_denovo needs --in_vcf"),
    (["--denovo", "--in_vcf", "testvcf.in.vcf.gz", "--denovo_families", "2"], "--denovo_families is not available with --in_vcf"),
    (["--denovo", "--in_vcf", "testvcf.in.vcf.gz", "--denovo_carriers", "2"], "--denovo_carriers is not available with --in_vcf"),
    (["--denovo", "--vcf_denovo", "--in_vcf", "testvcf.in.vcf.gz", "--denovo_carriers", "2"],
     "--denovo_carriers is not available with --in_vcf"),
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
    r = subprocess.run([cpu_driver] + BASE + [str(out), "--in_vcf", "testvcf.in.vcf.gz", "--vcf_denovo"], cwd=EXAMPLE,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "not supported by this evaluator" in r.stdout, r.stdout[-1000:]


def test_vcf_denovo_kernels_do_not_spill():
    res = _resources()
    for k in VDN_KERNELS:
        assert k in res, [n for n in res if "vdn" in n]
        assert int(res[k]["private_segment_fixed_size"]) == 0, (k, res[k])
