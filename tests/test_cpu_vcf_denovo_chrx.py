"""Device-free checks of de novo calling on chrX VCF records: the new symbol under an unchanged ABI version, the Python
method, the CLI's argument error (raised while the command line is parsed), the CPU driver's refusal of the flag, the
register-resident k_vdn_brent_x kernels read from the built gfx950 code object -- and the numpy reference that
tests/test_gpu_vcf_denovo_chrx.py judges the engine with, pinned here against the CPU oracle's standard chrX objective
(both mutation matrices the identity) and made to see its own planted events.

Which oracle entry pins which shapes: pmo_poly_loglik / pmo_objective evaluate the GLF-path objective, which gives a
nuclear family its closed form on chrX; vcf_mode peels those families there, and the two differ by ~1e-8 relative.  So
the GLF-path entries are compared on the shapes that are peeled on both paths (ext10, roof, roof2, extmix) and on
founders-only families (single); every shape, nuclear ones included, is compared with the oracle's vcf_mode site
evaluation (varllk[1] and varfreq[1] of pmo_site on a chrX section), which is the objective D is defined by.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import polymutt_amd as pm
import oracle_binding
from chrx_reference import three
from conftest import EXAMPLE
from oracle_binding import Oracle
from parity import FLAT_RTOL, FREQ_ATOL, LLK_RTOL
from test_cpu_kernel_resources import _resources
from test_gpu_vcf_denovo_chrx import dataset

BASE = ["-p", "test.ped", "-d", "test.dat", "--out_vcf"]
VDNX_KERNELS = ["void k_vdn_brent_x<256>(DevArgs, VdnXArgs)", "void k_vdn_brent_x<64>(DevArgs, VdnXArgs)"]


def test_symbol_and_method(built):
    lib = pm.load_library()
    assert lib.pm_abi_version() == 8   # additive: callers detect the feature by the symbol
    assert "pm_engine_set_vcf_denovo_chrx" in pm.engine.EXPORTS and hasattr(C.CDLL(pm.LIB_PATH), "pm_engine_set_vcf_denovo_chrx")
    assert callable(getattr(pm.Engine, "set_vcf_denovo_chrx"))


@pytest.mark.parametrize("extra", [
    ["--in_vcf", "testvcf.in.vcf.gz", "--vcf_denovo_chrX"],
    ["--in_vcf", "testvcf.in.vcf.gz", "--chrX", "1", "--vcf_denovo_chrX", "--denovo"],
])
def test_cli_argument_error(built, tmp_path, extra):
    """Raised while the command line is parsed: before the pedigree is read or an engine created (no GPU here)."""
    out = tmp_path / "out.vcf"
    r = subprocess.run([pm.BIN_PATH] + BASE + [str(out)] + extra, cwd=EXAMPLE, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, r.stdout[-1000:] + r.stderr[-1000:]
    assert "FATAL ERROR" in r.stdout and "--vcf_denovo_chrX needs --vcf_denovo" in r.stdout, r.stdout[-1000:]
    assert not out.exists()


def test_cpu_evaluator_refuses_the_flag(cpu_driver, tmp_path):
    out = tmp_path / "out.vcf"
    r = subprocess.run([cpu_driver] + BASE + [str(out), "--in_vcf", "testvcf.in.vcf.gz", "--chrX", "1", "--vcf_denovo",
                                              "--vcf_denovo_chrX"], cwd=EXAMPLE, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "not supported by this evaluator" in r.stdout, r.stdout[-1000:]


def test_chrx_kernels_do_not_spill():
    res = _resources()
    for k in VDNX_KERNELS:
        assert k in res, [n for n in res if "vdn" in n]
        assert int(res[k]["private_segment_fixed_size"]) == 0, (k, res[k])


@pytest.mark.parametrize("shape,nfam,nsites,glf_path", [("ext10", 1, 32, True), ("roof2", 1, 8, True), ("extmix", 5, 32, True),
                                                        ("single", 12, 32, True), ("mixed", 31, 32, False),
                                                        ("trio", 3, 32, False)])
def test_reference_matches_oracle_standard_chrx(built, tmp_path_factory, shape, nfam, nsites, glf_path):
    """The reference's enumeration with both mutation matrices the identity is the oracle's standard chrX objective:
    its maximum, its maximiser and its value at a fixed frequency.  The figures are printed before the assertions."""
    ped, block, refalt, planted, rv, models = dataset(tmp_path_factory, shape, nfam, nsites)
    par = pm.Params.defaults(vcf_mode=1)
    ora = Oracle(ped.view, par)
    ora.begin_section(pm.PM_CHR_X)
    L = oracle_binding.lib()
    res, _ = ora.run(block, np.zeros(block.shape[:2], np.uint32), refalt)   # vcf_mode: every family with offspring peeled
    assert (res["status"] == 0).all()
    err = np.abs(res["varllk"][:, 1] - rv[:, 2])
    print(f"{shape}/{nfam} vcf_mode site: max |D_r - D_o| / |D_o| = {(err / np.abs(res['varllk'][:, 1])).max():.3g}")
    assert (err <= LLK_RTOL * np.abs(res["varllk"][:, 1])).all()
    flat = err / np.maximum(np.abs(rv[:, 2]), 1e-300) <= FLAT_RTOL
    div = np.abs(res["varfreq"][:, 1] - rv[:, 3]) > FREQ_ATOL
    assert not (div & ~flat).any()
    if not glf_path:
        return
    worst = 0.0
    for i in range(len(refalt)):
        a1, a2, _ = three(refalt[i])
        site = np.ascontiguousarray(block[i])
        mn, ev = C.c_double(0), C.c_int32(0)
        o_max = L.pmo_poly_loglik(ora.h, site.ctypes.data, a1, a2, 0, C.byref(mn), C.byref(ev))
        o_fix = -ora.objective(site, a1, a2, 0.3, 0)
        r_fix = models[i].loglik(0.3, False)
        worst = max(worst, abs(o_max - rv[i, 2]) / abs(o_max), abs(o_fix - r_fix) / abs(o_fix))
        assert abs(o_max - rv[i, 2]) <= LLK_RTOL * abs(o_max), (i, o_max, rv[i, 2])
        assert abs(o_fix - r_fix) <= LLK_RTOL * abs(o_fix), (i, o_fix, r_fix)
    print(f"{shape}/{nfam} pmo_poly_loglik / pmo_objective: worst relative difference {worst:.3g}")


def test_reference_sees_its_plants(built, tmp_path_factory):
    """dataset() asserts, on the reference alone, that the largest planted DQ exceeds 3; here also that an unplanted site
    stays far below and that a founders-only pedigree has no mutation term at all."""
    ped, block, refalt, planted, rv, models = dataset(tmp_path_factory, "quad", 5)
    dq = rv[:, 0] - rv[:, 2]
    rest = np.setdiff1d(np.arange(len(dq)), planted)
    print("quad/5 reference DQ: planted", dq[planted], "largest elsewhere", dq[rest].max())
    assert dq[planted].max() > 3 and dq[rest].max() < 0.5
    ped, block, refalt, planted, rv, models = dataset(tmp_path_factory, "single", 12)
    assert not planted and (np.abs(rv[:, 0] - rv[:, 2]) <= LLK_RTOL * 2 * np.abs(rv[:, 2])).all()


def test_reference_is_sex_aware(built, tmp_path_factory):
    """A hemizygous-reference son of an alternate-allele father: Mendelian for the reference on X; and a daughter of the
    same parents with the same data is not."""
    from test_gpu_vcf_denovo_chrx import _one_family_block, _reference_dq
    refalts = np.array([1 | (3 << 4), 1 | (2 << 4)], np.uint8)
    ped = dataset(tmp_path_factory, "trio", 3)[0]
    son = _reference_dq(ped, _one_family_block(ped, 0, 2, refalts), refalts, None)
    ped = dataset(tmp_path_factory, "mixed", 31)[0]
    daughter = _reference_dq(ped, _one_family_block(ped, 1, 3, refalts), refalts, None)
    print("reference DQ: son", son[:, 1], "daughter", daughter[:, 1])
    assert (son[:, 1] < 0.5).all() and (daughter[:, 1] > 3).all()
